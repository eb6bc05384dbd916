"""GPU: the result BITS of the three KV-cache libraries (fa_kv_forward, fa_paged_forward, fa_kv8_forward, fa_kv8_paged_forward): sha256 of the
raw bytes of o and of lse per case against tests/golden/kv_output_digests.txt, recorded on the commit before the decode loops and merges
of the three libraries were folded into shared headers (csrc/fa_kv_decode_core.h, fa_kv_combine_kernel.h).  A change of those headers that
is meant to leave the arithmetic alone must leave every digest alone.

Cases -- the smallest that reach every path; each runs without a workspace (one share) and with one (the plan's shares, merged):
    base   bh_kv 2, group 4, nq 3 (12 packed rows: less than a tile), nk 1000 with lengths [777, 0] -- a ragged row tile and a slab without
           a key -- where the plan gives S = 3;  d in {64, 128} x causal x output dtype
    tiles  d 128: group 8, nq 5, nk 600, no lengths: 40 rows = two tiles, one straddling heads under causal; unsplit it is 10 blocks, so
           waves 0-1 take three steps and waves 2-3 two
    one    d 128: bh_kv 1, group 1, nq 1, nk 64: one block, three idle waves
over the bf16 contiguous cache, the bf16 paged cache, the fp8 contiguous and the fp8 paged cache (k_scale 0.5, v_scale 0.37); paged with pages
of 16 and of 256 rows behind a shuffled table.  Inputs come from a CPU torch.Generator with a fixed seed.

Re-record on a GPU (after a change that is MEANT to move result bits, with the reason in the commit message):
    python -m tests.test_gpu_kv_bits --record [path, default tests/golden/kv_output_digests.txt]
"""
import ctypes
import functools
import hashlib
import os
import sys

import pytest
import torch

from flashattention_c_amd import _cabi_kv, _cabi_kv8, _cabi_paged
from tests.conftest import GOLDEN_DIR
from tests.kv8_reference import quantize

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(GOLDEN_DIR, "kv_output_digests.txt")
BF16, BF16_F32 = _cabi_kv.FA_DTYPE_BF16, _cabi_kv.FA_DTYPE_BF16_OUT_F32
SCALE, KS, VS = 0.125, 0.5, 0.37

# name: (batch, heads_kv, group, nq, nk, lens per sequence)
SHAPES = {"base": (2, 1, 4, 3, 1000, (777, 0)), "tiles": (1, 2, 8, 5, 600, None), "one": (1, 1, 1, 1, 64, None)}
CACHES = ("kv", "paged16", "paged256", "kv8", "kv8paged16", "kv8paged256")


def cases():
    for shape, ds in (("base", (64, 128)), ("tiles", (128,)), ("one", (128,))):
        for d in ds:
            for cache in CACHES:
                for causal in (0, 1):
                    for odt in ("bf16", "f32"):
                        for ws in ("unsplit", "ws"):
                            yield f"{shape}-d{d}-{cache}-{'causal' if causal else 'full'}-{odt}-{ws}"


@functools.lru_cache(maxsize=None)
def inputs(shape, d, fp8, page):
    """q, (k, v) or (k_pool, v_pool, table), lens on the device; the pools hold the rows of the contiguous cache behind a shuffled table"""
    batch, H, group, nq, nk, lens = SHAPES[shape]
    g = torch.Generator().manual_seed(20240 + d + (7 if fp8 else 0))
    dev = torch.device("cuda", 0)
    q = torch.randn(batch * H * group, nq, d, generator=g).to(torch.bfloat16)
    k, v = (torch.randn(batch * H, nk, d, generator=g) for _ in range(2))
    k, v = ((quantize(t, 1.0).view(torch.uint8) if fp8 else t.to(torch.bfloat16).view(torch.int16)) for t in (k, v))   # as integers: plain copies below
    lens_d = torch.tensor(lens, dtype=torch.int32).to(dev) if lens else None
    if not page:
        return q.to(dev), tuple(t.to(dev) for t in (k, v)), lens_d
    per_seq = -(-nk // page)
    order = torch.randperm(batch * per_seq + 3, generator=g)
    table = order[:batch * per_seq].reshape(batch, per_seq).to(torch.int32)
    pools = []
    for t in (k, v):
        pool = torch.randint(1, 100, (len(order), page, H, d), generator=g).to(t.dtype)   # page tails and spare pages: finite values nobody may use
        for b in range(batch):
            for p in range(per_seq):
                rows = min(page, nk - p * page)
                pool[table[b, p], :rows] = t[b * H:(b + 1) * H, p * page:p * page + rows].transpose(0, 1)
        pools.append(pool.to(dev))
    return q.to(dev), (*pools, table.to(dev)), lens_d


def run(case):
    """(o, lse) of one case, through the C entry itself: whether a launch splits is decided by the workspace it is given"""
    shape, d, cache, causal, odt, ws = case.split("-")
    batch, H, group, nq, nk, _ = SHAPES[shape]
    d, causal, fp8 = int(d[1:]), int(causal == "causal"), cache.startswith("kv8")
    page = int(cache.split("paged")[1]) if "paged" in cache else 0
    q, kv, lens_d = inputs(shape, d, fp8, page)
    dt = BF16_F32 if odt == "f32" else BF16
    o = torch.zeros(q.shape, dtype=torch.float32 if odt == "f32" else torch.bfloat16, device=q.device)
    lse = torch.zeros(q.shape[:2], dtype=torch.float32, device=q.device)
    L = _cabi_kv8.lib() if fp8 else _cabi_paged.lib() if page else _cabi_kv.lib()
    need = int(_cabi_kv.lib().fa_kv_workspace_bytes(batch * H, group, nq, nk, d, causal, dt))   # the three libraries share one plan
    assert (need > 0) == (shape != "one")
    if shape == "base":
        assert _cabi_kv.lib().fa_kv_splits_for(batch * H, group, nq, nk, d, causal, dt) == 3
    wsp = torch.zeros(max(need, 256), dtype=torch.uint8, device=q.device) if ws == "ws" else None
    tail = (causal, dt, wsp.data_ptr() if wsp is not None else None, wsp.numel() if wsp is not None else 0,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    scales = (SCALE, KS, VS) if fp8 else (SCALE,)
    lens_p = lens_d.data_ptr() if lens_d is not None else None
    if page:
        kp, vp, table = kv
        c = _cabi_paged.FaPagedCache(kp.data_ptr(), vp.data_ptr(), kp.shape[0], page, kp.stride(0), kp.stride(1), kp.stride(2), table.data_ptr(),
                                     table.shape[1], lens_p)
        fn, err = (L.fa_kv8_paged_forward, L.fa_kv8_last_error) if fp8 else (L.fa_paged_forward, L.fa_paged_last_error)
        rc = fn(q.data_ptr(), ctypes.byref(c), o.data_ptr(), lse.data_ptr(), batch, H, group, nq, nk, d, *scales, *tail)
    else:
        fn, err = (L.fa_kv8_forward, L.fa_kv8_last_error) if fp8 else (L.fa_kv_forward, L.fa_kv_last_error)
        rc = fn(q.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), o.data_ptr(), lse.data_ptr(), batch * H, group, nq, nk, nk, lens_p, d, *scales, *tail)
    assert rc == 0, err()
    torch.cuda.synchronize()
    return o, lse


def digests(case):
    o, lse = run(case)
    raw = lambda t: t.cpu().contiguous().view(torch.uint8).numpy().tobytes()   # noqa: E731
    return hashlib.sha256(raw(o)).hexdigest(), hashlib.sha256(raw(lse)).hexdigest()


@functools.lru_cache(maxsize=None)
def golden():
    return {ln.split()[0]: tuple(ln.split()[1:]) for ln in open(GOLDEN).read().splitlines() if ln and not ln.startswith("#")}


def test_the_golden_names_exactly_these_cases():
    assert sorted(golden()) == sorted(cases()) and len(golden()) == 192


@pytest.mark.parametrize("case", list(cases()))
def test_result_bits_are_the_recorded_ones(case):
    have, want = digests(case), golden()[case]
    print(case, "o", have[0][:16], "lse", have[1][:16])
    assert have[1] == want[1], f"{case}: the bits of lse moved"
    assert have[0] == want[0], f"{case}: the bits of o moved"
    if case.startswith("base"):   # the slab without a key: zeros and -inf, whatever the digest says
        o, lse = run(case)
        assert not o[o.shape[0] // 2:].any() and bool((lse[lse.shape[0] // 2:] == float("-inf")).all())


def record(path=GOLDEN):
    rows = [(c, *digests(c)) for c in cases()]
    with open(path, "w") as f:
        f.write("# sha256 of the raw bytes of o and of lse per case of tests/test_gpu_kv_bits.py (which says how to re-record): <case> <o> <lse>\n")
        for r in rows:
            f.write(" ".join(r) + "\n")
    print(f"{len(rows)} cases -> {path}")


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit(__doc__)
    record(*sys.argv[2:3])
