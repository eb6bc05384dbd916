"""The Python surface of the five KV-cache libraries, held against goldens recorded from the commit before the five bindings, the four
front-end functions and the five build rules were folded into one of each (_cabi_ext.py, flash.py, build.py):

    tests/golden/kv_python_bindings.txt     CPU: EXPORTED_SYMBOLS of every _cabi_* module, the argtypes / restype bind() leaves on every symbol
                                            of the loaded library, and what workspace_bytes_kv / workspace_bytes_paged return
    tests/golden/kv_python_errors_cpu.txt   CPU: exception class and text of every check forward_kv / forward_paged / forward_kv_fp8 /
                                            forward_paged_fp8 make before they look at the device, with window_left None and 5
    tests/golden/kv_python_errors_gpu.txt   GPU: the same for every check after that one, down to the calls that pass Python and are refused by
                                            the library (FlashAttnError with the text of that library's own fa_*_last_error)

Every walked call raises (asserted here and by the recorder), so no call of the two walks launches a kernel.  Most calls break one thing; the few
that break two name the check that answers first.  A bad ``window_left`` is never combined with a second fault: it is the one check whose place
differed between the bf16 and the fp8 entries before (it now comes first in all four).  On CPU tensors it would always be combined with the
device check, so the bad windows are walked on device tensors for the four entries and on the two workspace queries on the CPU.

Re-record (after a change that is MEANT to move a prototype, a workspace size, a message or the order of two checks):
    python flashattention.c_amd/build.py && python -m tests.test_kv_python_surface --record
on a machine with a GPU; without one the GPU golden is left as it is.
"""
import os
import sys

import pytest
import torch

import flashattention_c_amd as fa
from flashattention_c_amd import _cabi_kv, _cabi_kv8, _cabi_kvw, _cabi_kvw8, _cabi_paged
from tests.conftest import GOLDEN_DIR

BINDINGS = os.path.join(GOLDEN_DIR, "kv_python_bindings.txt")
ERRORS_CPU = os.path.join(GOLDEN_DIR, "kv_python_errors_cpu.txt")
ERRORS_GPU = os.path.join(GOLDEN_DIR, "kv_python_errors_gpu.txt")
MODULES = (("kv", _cabi_kv), ("paged", _cabi_paged), ("kv8", _cabi_kv8), ("kvw", _cabi_kvw), ("kvw8", _cabi_kvw8))
# (name, paged?, fp8?)
ENTRIES = (("forward_kv", False, False), ("forward_paged", True, False), ("forward_kv_fp8", False, True), ("forward_paged_fp8", True, True))
WINDOWS = (None, 5)
BF16, F16, F32, F8, U8, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn, torch.uint8, torch.int32, torch.int64
BIG_WINDOW = 4096   # a window that hides nothing of 1024 keys: the windowed plan still splits them, so there is scratch to be one byte short of


def binding_rows():
    """[(label, value)]: the symbols and prototypes of the five bindings, then the two workspace queries"""
    rows = []
    for tag, mod in MODULES:
        L = mod.lib()
        rows.append((f"{tag} EXPORTED_SYMBOLS", ",".join(mod.EXPORTED_SYMBOLS)))
        for sym in mod.EXPORTED_SYMBOLS:
            f = getattr(L, sym)
            rows.append((f"{tag} {sym}", f"({','.join(t.__name__ for t in f.argtypes)}) -> {f.restype.__name__}"))
    for nk in (1024, 64):
        for wl in (None, 0, 100, 1 << 30):
            for odt in (BF16, F32):
                rows.append((f"workspace_bytes_kv(2, 4, 1, {nk}, 64) window_left={wl} {odt}", str(fa.workspace_bytes_kv(2, 4, 1, nk, 64, out_dtype=odt, window_left=wl))))
                rows.append((f"workspace_bytes_paged(2, 2, 2, 1, {nk}, 64) window_left={wl} {odt}",
                             str(fa.workspace_bytes_paged(2, 2, 2, 1, nk, 64, out_dtype=odt, window_left=wl))))
    return rows


def _call(name, paged, spec):
    """the entry on the tensors of `spec` (q, k, v and, paged, t: the block table); every other key is a keyword argument"""
    spec = dict(spec)
    args = [spec.pop(n) for n in (("q", "k", "v", "t") if paged else ("q", "k", "v"))]
    return getattr(fa, name)(*args, **spec)


def _good(paged, fp8, dev, nk=64, d=64):
    """q (8, 1, d); a cache (2, nk, d), or pools (8, 16, 2, d) under a table (2, nk / 16): 2 sequences x 2 heads, group 2"""
    cdt = F8 if fp8 else BF16
    spec = dict(q=torch.zeros((8, 1, d), dtype=BF16, device=dev))
    for n in ("k", "v"):
        spec[n] = torch.zeros((8, 16, 2, d) if paged else (2, nk, d), dtype=cdt, device=dev)
    if paged:
        spec["t"] = torch.zeros((2, nk // 16), dtype=I32, device=dev)
    return spec


def cpu_cases(paged, fp8):
    """[(label, what to replace in the good call)]: one call per check that runs before the device check, on CPU tensors"""
    C = F8 if fp8 else BF16
    cshape = (8, 16, 2, 64) if paged else (2, 64, 64)

    def z(shape, dt=C):
        return torch.zeros(shape, dtype=dt)

    cases = [(f"{n} is not a tensor", {n: None}) for n in (("q", "k", "v", "t") if paged else ("q", "k", "v"))]
    cases.append(("q is 2-D", dict(q=z((8, 64), BF16))))
    if paged:
        cases += [("pools are 2-D", dict(k=z((8, 64)), v=z((8, 64)))), ("pools are 5-D", dict(k=z((8, 16, 2, 1, 64)), v=z((8, 16, 2, 1, 64)))),
                  ("v_pool has another shape", dict(v=z((8, 16, 1, 64)))), ("v_pool has other strides", dict(v=z((8, 16, 2, 128))[..., :64]))]
    else:
        cases += [("k is 2-D", dict(k=z((2, 64)))), ("v is 4-D", dict(v=z((2, 64, 1, 64)))), ("v has another shape", dict(v=z((2, 65, 64))))]
    cases.append(("v has another dtype", dict(v=z(cshape, F16))))
    for dt in (F16, F32):
        cases.append((f"everything is {dt}", dict(q=z((8, 1, 64), dt), k=z(cshape, dt), v=z(cshape, dt))))
        if fp8:
            cases.append((f"q is {dt}", dict(q=z((8, 1, 64), dt))))
    if fp8:
        cases += [("the caches are uint8", dict(k=z(cshape, U8), v=z(cshape, U8))), ("v is uint8", dict(v=z(cshape, U8)))]
    cases.append(("everything is on the CPU", {}))
    # two faults: the first check answers
    cases += [("q is not a tensor, k is float32", dict(q=None, k=z(cshape, F32))),
              ("v has another shape, everything is float16", dict(q=z((8, 1, 64), F16), k=z(cshape, F16), v=z(cshape[:-1] + (128,), F16))),
              ("q is 2-D, everything is on the CPU and float32", dict(q=z((8, 64), F32), k=z(cshape, F32), v=z(cshape, F32)))]
    return cases


def gpu_cases(paged, fp8, wl, dev):
    """[(label, what to replace in the good call, raised by the library?)]: one call per check from the device check on"""
    C = F8 if fp8 else BF16
    lens = "seq_lens" if paged else "kv_lens"

    def z(shape, dt=C):
        return torch.zeros(shape, dtype=dt, device=dev)

    def cshape(d=64):
        return (8, 16, 2, d) if paged else (2, 64, d)

    cases = [("head dim of q is 128", dict(q=z((8, 1, 128), BF16)))]
    cases += [(f"head dim {d}", dict(q=z((8, 1, d), BF16), k=z(cshape(d)), v=z(cshape(d)))) for d in (32, 96)]
    cases += [("7 query slabs", dict(q=z((7, 1, 64), BF16))), ("no query slab", dict(q=z((0, 1, 64), BF16))), ("no query row", dict(q=z((8, 0, 64), BF16)))]
    if paged:
        cases += [("no sequence", dict(t=z((0, 4), I32))), ("no table column", dict(t=z((2, 0), I32))), ("no page", dict(k=z((0, 16, 2, 64)), v=z((0, 16, 2, 64)))),
                  ("no head", dict(k=z((8, 16, 0, 64)), v=z((8, 16, 0, 64))))]
    else:
        cases += [("no cache slab", dict(k=z((0, 64, 64)), v=z((0, 64, 64)))), ("no cache row", dict(k=z((2, 0, 64)), v=z((2, 0, 64))))]
    cases += [("kv_len 0", dict(kv_len=0)), ("kv_len capacity + 1", dict(kv_len=65)),
              (f"{lens} is a list", {lens: [64, 64]}), (f"{lens} is int64", {lens: z((2,), I64)}), (f"{lens} has 3 entries", {lens: z((3,), I32)}),
              (f"{lens} is on the CPU", {lens: torch.zeros((2,), dtype=I32)}), (f"{lens} is strided", {lens: z((4,), I32)[::2]}),
              ("out_dtype float16", dict(out_dtype=F16)), ("out has another shape", dict(out=z((8, 2, 64), BF16))),
              ("out is bfloat16 under out_dtype float32", dict(out=z((8, 1, 64), BF16), out_dtype=F32)), ("out is strided", dict(out=z((8, 1, 128), BF16)[..., ::2])),
              ("workspace is int8", dict(workspace=z((1 << 16,), torch.int8)))]
    big = None if wl is None else BIG_WINDOW
    need = fa.workspace_bytes_paged(2, 2, 2, 1, 1024, 64, window_left=big) if paged else fa.workspace_bytes_kv(2, 4, 1, 1024, 64, window_left=big)
    assert need > 0
    long = _good(paged, fp8, dev, nk=1024)
    cases.append((f"workspace one byte short of {need} (1024 keys, window_left={big})", dict(long, workspace=z((need - 1,), U8), window_left=big)))
    if paged:
        cases += [("last stride 2", dict(k=z((8, 16, 2, 128))[..., ::2], v=z((8, 16, 2, 128))[..., ::2])),
                  ("head stride 64 + 4", dict(k=z((8, 16, 2, 68))[..., :64], v=z((8, 16, 2, 68))[..., :64])),
                  ("table is int64", dict(t=z((2, 4), I64))), ("table is 1-D", dict(t=z((8,), I32))), ("table is strided", dict(t=z((2, 8), I32)[:, ::2]))]
        if fp8:   # the 16-bit pools take this one: test_the_bf16_pools_take_a_stride_of_8_elements_more
            cases.append(("head stride 64 + 8", dict(k=z((8, 16, 2, 72))[..., :64], v=z((8, 16, 2, 72))[..., :64])))
    cases.append(("kv_len 0, out has another shape", dict(kv_len=0, out=z((8, 2, 64), BF16))))
    cases = [c + (False,) for c in cases]
    # what passes Python and is refused by the library's validator, before any launch
    cases.append(("scale 0", dict(scale=0.0), True))
    if fp8:
        cases += [("k_scale -1", dict(k_scale=-1.0), True), ("v_scale inf", dict(v_scale=float("inf")), True)]
    return cases


def _raised(label, fn, *args, **kw):
    try:
        fn(*args, **kw)
    except (TypeError, ValueError, _cabi_kv.FlashAttnError) as e:
        return (label, type(e).__name__, str(e))
    raise AssertionError(f"{label}: the call did not raise")


def walk_cpu():
    """[(label, exception class, text)] of every bad call that needs no device"""
    rows = []
    for name, paged, fp8 in ENTRIES:
        for wl in WINDOWS:
            for label, change in cpu_cases(paged, fp8):
                rows.append(_raised(f"{name} window_left={wl} | {label}", _call, name, paged, {**_good(paged, fp8, "cpu"), "window_left": wl, **change}))
    for wl in (-1, True, 1.5):
        rows.append(_raised(f"workspace_bytes_kv | window_left={wl!r}", fa.workspace_bytes_kv, 2, 4, 1, 64, 64, window_left=wl))
        rows.append(_raised(f"workspace_bytes_paged | window_left={wl!r}", fa.workspace_bytes_paged, 2, 2, 2, 1, 64, 64, window_left=wl))
    assert len({r[0] for r in rows}) == len(rows)
    return rows


def walk_gpu():
    """[(label, exception class, text)] of every bad call on device tensors"""
    dev = torch.device("cuda", 0)
    rows = []
    for name, paged, fp8 in ENTRIES:
        for wl in WINDOWS:
            for label, change, by_library in gpu_cases(paged, fp8, wl, dev):
                row = _raised(f"{name} window_left={wl} | {label}", _call, name, paged, {**_good(paged, fp8, dev), "window_left": wl, **change})
                if by_library:   # the text of this library's own thread-local error, not an empty one read from another library
                    assert row[1] == "FlashAttnError" and len(row[2].split(": ", 1)[1]) > 10, row
                else:
                    assert row[1] != "FlashAttnError", row
                rows.append(row)
        for wl in (-1, True, 1.5):
            rows.append(_raised(f"{name} | window_left={wl!r}", _call, name, paged, dict(_good(paged, fp8, dev), window_left=wl)))
    assert len({r[0] for r in rows}) == len(rows)
    return rows


def _read(path):
    return [tuple(ln.split("\t")) for ln in open(path).read().splitlines() if ln and not ln.startswith("#")]


def _same(have, want):
    assert [r[0] for r in have] == [r[0] for r in want]
    diff = [f"{h[0]}\n    recorded: {w[1:]}\n    now:      {h[1:]}" for h, w in zip(have, want) if tuple(h) != tuple(w)]
    assert not diff, "\n".join(diff)


def test_the_bindings_and_the_workspace_queries_are_the_recorded_ones():
    have = binding_rows()
    _same(have, _read(BINDINGS))
    assert sum(len(m.EXPORTED_SYMBOLS) for _, m in MODULES) == 7 + 6 + 7 + 9 + 9
    sizes = {r[0]: int(r[1]) for r in have if r[0].startswith("workspace_bytes")}
    assert len(sizes) == 32
    for k, v in sizes.items():   # 1024 keys are split when the window hides none of them, 64 keys (or a window of 64) never
        if ", 64, 64)" in k or "window_left=0 " in k:
            assert v == 0, k
        elif "window_left=None" in k or f"window_left={1 << 30}" in k:
            assert v > 0, k


def test_every_check_before_the_device_answers_with_the_recorded_exception():
    have = walk_cpu()
    _same(have, _read(ERRORS_CPU))
    assert len(have) > 100 and all(r[2] for r in have)


@pytest.mark.gpu
def test_every_check_on_device_tensors_answers_with_the_recorded_exception():
    have = walk_gpu()
    _same(have, _read(ERRORS_GPU))
    assert len(have) > 200 and all(r[2] for r in have)


@pytest.mark.gpu
@pytest.mark.parametrize("window_left", WINDOWS)
def test_the_bf16_pools_take_a_stride_of_8_elements_more(window_left):
    """what the fp8 pools refuse ("head stride 64 + 8": 8 bytes there, 16 here): accepted, never copied, and the result of the dense pool"""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    q = torch.randn((8, 1, 64), generator=g).to(BF16).to(dev)
    wide = torch.randn((2, 8, 16, 2, 72), generator=g).to(BF16).to(dev)
    k, v = wide[0][..., :64], wide[1][..., :64]
    assert k.stride() == (16 * 2 * 72, 2 * 72, 72, 1)
    table = torch.tensor([[5, 1, 7, 2], [0, 6, 3, 4]], dtype=I32, device=dev)
    o = fa.forward_paged(q, k, v, table, True, kv_len=50, scale=0.125, window_left=window_left)
    ref = fa.forward_paged(q, k.contiguous(), v.contiguous(), table, True, kv_len=50, scale=0.125, window_left=window_left)
    assert torch.isfinite(o.float()).all() and o.abs().max() > 0 and torch.equal(o, ref)


def _write(path, what, rows):
    assert not any("\t" in f or "\n" in f for r in rows for f in r)
    with open(path, "w") as f:
        f.write(f"# {what} of tests/test_kv_python_surface.py, tab-separated.\n"
                "# Re-record: python flashattention.c_amd/build.py && python -m tests.test_kv_python_surface --record   (the GPU file: on a machine with a GPU)\n")
        for r in rows:
            f.write("\t".join(r) + "\n")
    print(f"{len(rows)} rows -> {path}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    _write(BINDINGS, "(symbols or prototype or bytes) of every binding and workspace query", binding_rows())
    _write(ERRORS_CPU, "(exception class, text) of every bad call on CPU tensors", walk_cpu())
    if torch.cuda.is_available():
        _write(ERRORS_GPU, "(exception class, text) of every bad call on device tensors", walk_gpu())
    else:
        print(f"no GPU: {ERRORS_GPU} left as it is")
