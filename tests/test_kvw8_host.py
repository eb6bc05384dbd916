"""CPU: the sliding-window fp8 KV-cache library (include/flashattn_amd_kvw8.h, libflashattn_amd_kvw8.so) without a device: the header against
the binding and the exports, every inherited and new check of the host side through ctypes (no call reaches a launch, no pointer is
dereferenced), the plan -- that of libflashattn_amd_kvw.so for the same arguments -- and the code objects of its kernels held against their
unwindowed twins in libflashattn_amd_kv8.so (not against a snapshot)."""
import ctypes
import os
import re

import pytest

from flashattention_c_amd import _cabi_kv8, _cabi_kvw, _cabi_kvw8
from tests import codeobj
from tests.test_kvw_host import GRID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, BF16_F32, F32 = _cabi_kvw8.FA_DTYPE_BF16, _cabi_kvw8.FA_DTYPE_BF16_OUT_F32, _cabi_kvw8.FA_DTYPE_F32
INVALID, UNSUPPORTED = 1, 2
A = 0x7f0000000000   # pointers that are never dereferenced: validation comes before any device call
G = 1 << 30
BAD_SCALES = [0.0, -1.0, float("inf"), float("-inf"), float("nan")]


# ---- the ABI ----
def test_header_binding_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "flashattn_amd_kvw8.h")).read()
    declared = set(re.findall(r"\b(fa_kvw8_\w+)\(", text.split("#define FLASHATTN_AMD_KVW8_ABI_VERSION")[1]))
    assert declared == set(_cabi_kvw8.EXPORTED_SYMBOLS), declared ^ set(_cabi_kvw8.EXPORTED_SYMBOLS)
    L = _cabi_kvw8.lib()
    for s in _cabi_kvw8.EXPORTED_SYMBOLS:
        assert getattr(L, s) is not None
    assert L.fa_kvw8_version().startswith(b"flashattn_amd_kvw8 abi 1 gfx950 ")
    exported = os.popen(f"nm -D --defined-only {_cabi_kvw8.LIB_PATH}").read()
    names = set(re.findall(r" T (fa_\w+)", exported))
    assert names == set(_cabi_kvw8.EXPORTED_SYMBOLS), names ^ set(_cabi_kvw8.EXPORTED_SYMBOLS)   # self-contained: no fa_kv8_* / fa_kvw_* symbol
    assert not re.search(r" T fa_kv8_| T fa_kvw_| T fa_kv_| T fa_paged_", exported)
    for words in ("window_left > 2^24", "attention sinks", "soft-capping", "per-head or per-token scales", "flashattn_amd_kv8.h", "flashattn_amd_kvw.h"):
        assert words in text, words
    import flashattention_c_amd as fa
    import inspect
    for name in ("forward_kv_fp8", "forward_paged_fp8"):
        assert inspect.signature(getattr(fa, name)).parameters["window_left"].default is None


# ---- errors: contiguous ----
Q, K, V, O, LSE, LENS, WS = A, A + 1 * G, A + 2 * G, A + 3 * G, A + 4 * G, A + 4 * G + (1 << 20), A + 5 * G


def contiguous(**kw):
    a = dict(q=Q, k=K, v=V, o=O, lse=None, B=2, group=4, nq=1, nk=4096, cap=4096, lens=None, d=128, scale=1.0, k_scale=0.5, v_scale=2.0, causal=1,
             dtype=BF16, window=1023, ws=None, ws_bytes=0)
    assert set(kw) <= set(a)
    a.update(kw)
    L = _cabi_kvw8.lib()
    rc = L.fa_kvw8_forward(a["q"], a["k"], a["v"], a["o"], a["lse"], a["B"], a["group"], a["nq"], a["nk"], a["cap"], a["lens"], a["d"], a["scale"],
                           a["k_scale"], a["v_scale"], a["causal"], a["dtype"], a["window"], a["ws"], a["ws_bytes"], None)
    return rc, L.fa_kvw8_last_error().decode()


def test_contiguous_errors_reach_their_code_and_text():
    L = _cabi_kvw8.lib()
    need = L.fa_kvw8_workspace_bytes(2, 4, 1, 4096, 128, 1, BF16, 1023)
    assert need > 0
    slab = 4096 * 128   # bytes of one K/V slab: an element is one byte
    for kw, code, words in [
            (dict(window=-1), INVALID, "window_left = -1 must be >= 0"),
            (dict(window=-(1 << 31)), INVALID, "must be >= 0"),
            (dict(dtype=F32), UNSUPPORTED, "FA_DTYPE_F32 is not supported: q and o are as in fa_kv_forward"),
            (dict(dtype=7), INVALID, "unknown dtype 7"),
            (dict(d=96), UNSUPPORTED, "head dim 96 is not supported: 64 or 128"),
            (dict(q=None), INVALID, "null pointer: q, k8, v8 and o are required"),
            (dict(nk=0), INVALID, "bh_kv, group, nq and nk must be >= 1"),
            (dict(nk=4097), INVALID, "nk = 4097 exceeds capacity = 4096"),
            (dict(cap=1 << 25), UNSUPPORTED, "must stay below 2^32 bytes"),
            (dict(scale=0.0), INVALID, "scale must be finite and non-zero"),
            *[(dict(k_scale=s), INVALID, "k_scale must be finite and > 0") for s in BAD_SCALES],
            *[(dict(v_scale=s), INVALID, "v_scale must be finite and > 0") for s in BAD_SCALES],
            (dict(scale=1e30, k_scale=1e30), INVALID, "scale * k_scale must be finite and non-zero in fp32"),
            (dict(scale=1e-30, k_scale=1e-30), INVALID, "scale * k_scale must be finite and non-zero in fp32"),
            (dict(ws=WS, ws_bytes=need - 1), INVALID, f"is too small: fa_kvw8_workspace_bytes() = {need}"),
            (dict(ws=WS, ws_bytes=1), INVALID, "is too small"),
            (dict(o=Q), INVALID, "o overlaps q, k8 or v8"),
            (dict(o=K + slab), INVALID, "o overlaps q, k8 or v8"),
            (dict(lse=V + 2 * slab - 4), INVALID, "lse overlaps q, k8, v8 or o"),
            (dict(ws=V, ws_bytes=need), INVALID, "the workspace overlaps a tensor of the call"),
            (dict(lens=WS + 512, ws=WS, ws_bytes=need), INVALID, "the workspace overlaps a tensor of the call"),
            (dict(q=Q + 8), INVALID, "q, k8, v8, o must be 16-byte aligned"),
            (dict(k=K + 8), INVALID, "q, k8, v8, o must be 16-byte aligned"),
            (dict(v=V + 8), INVALID, "q, k8, v8, o must be 16-byte aligned"),
            (dict(lse=LSE + 2), INVALID, "lse must be 4-byte aligned"),
            (dict(lens=LENS + 1), INVALID, "kv_lens must be 4-byte aligned"),
            (dict(ws=WS + 128, ws_bytes=need), INVALID, "workspace must be 256-byte aligned")]:
        rc, text = contiguous(**kw)
        assert rc == code and words in text, (kw, rc, text)
    # the window is checked behind the scales and in front of the plan: a call wrong in both reports the scale
    assert "k_scale" in contiguous(k_scale=0.0, window=-1)[1] and "window_left" in contiguous(window=-1, ws=WS, ws_bytes=1)[1]
    assert L.fa_kvw8_workspace_bytes(2, 4, 1, 4096, 128, 1, BF16, 100) == 0   # a window the plan does not split under needs no workspace
    # the queries answer 0 / NULL to what the forward rejects
    for args in [(2, 4, 1, 4096, 128, 1, BF16, -1), (2, 4, 1, 4096, 96, 1, BF16, 5), (2, 4, 1, 4096, 128, 1, F32, 5), (0, 4, 1, 4096, 128, 1, BF16, 5),
                 (2, 4, 1, (1 << 24) + 1, 128, 1, BF16, 5)]:
        assert L.fa_kvw8_workspace_bytes(*args) == 0 and L.fa_kvw8_splits_for(*args) == 0
        assert L.fa_kvw8_paged_workspace_bytes(args[0], 1, *args[1:]) == 0 and L.fa_kvw8_paged_splits_for(args[0], 1, *args[1:]) == 0
        for page in (0, 64):
            assert L.fa_kvw8_kernel_name_for(*args[:-1], page, args[-1]) is None
    for page in (8, 24, 1 << 17, -16):
        assert L.fa_kvw8_kernel_name_for(2, 4, 1, 4096, 128, 1, BF16, page, 5) is None
    assert L.fa_kvw8_kernel_name_for(2, 4, 1, 4096, 128, 1, BF16, 0, 5) == L.fa_kvw8_kernel_name_for(2, 4, 1, 4096, 128, 1, BF16, 16, 5) == b"fa_kvw8_decode_kernel"


# ---- errors: paged.  2 sequences x 2 heads, (pages, page, H, d) pools of 64 pages of 64 rows ----
POOL_K, POOL_V, TABLE, LENS_P, OP, LSE_P = A + 1 * G, A + 2 * G, A + 3 * G, A + 3 * G + (1 << 20), A + 4 * G, A + 6 * G


def paged(**kw):
    a = dict(q=Q, o=OP, lse=None, cache=True, B=2, heads_kv=2, group=4, nq=1, nk=2048, d=128, scale=1.0, k_scale=0.5, v_scale=2.0, causal=1, dtype=BF16,
             window=1023, ws=None, ws_bytes=0)
    f = dict(k_pool=POOL_K, v_pool=POOL_V, num_pages=64, page_size=64, page_stride=64 * 2 * 128, row_stride=2 * 128, head_stride=128, block_table=TABLE,
             max_pages=32, seq_lens=LENS_P)
    assert set(kw) <= set(a) | set(f)
    a.update({k: v for k, v in kw.items() if k in a})
    f.update({k: v for k, v in kw.items() if k in f})
    cache = ctypes.byref(_cabi_kvw8.FaPagedCache(**f)) if a["cache"] else None
    L = _cabi_kvw8.lib()
    rc = L.fa_kvw8_paged_forward(a["q"], cache, a["o"], a["lse"], a["B"], a["heads_kv"], a["group"], a["nq"], a["nk"], a["d"], a["scale"], a["k_scale"],
                                 a["v_scale"], a["causal"], a["dtype"], a["window"], a["ws"], a["ws_bytes"], None)
    return rc, L.fa_kvw8_last_error().decode()


def test_paged_errors_reach_their_code_and_text():
    L = _cabi_kvw8.lib()
    need = L.fa_kvw8_paged_workspace_bytes(2, 2, 4, 1, 2048, 128, 1, BF16, 1023)
    assert need > 0 and need == L.fa_kvw8_workspace_bytes(4, 4, 1, 2048, 128, 1, BF16, 1023)
    page_bytes = 64 * 2 * 128
    for kw, code, words in [
            (dict(window=-1), INVALID, "window_left = -1 must be >= 0"),
            (dict(dtype=F32), UNSUPPORTED, "FA_DTYPE_F32 is not supported: q and o are as in fa_kv_forward"),
            (dict(d=96), UNSUPPORTED, "head dim 96 is not supported: 64 or 128"),
            (dict(cache=False), INVALID, "null pointer: q, cache and o are required"),
            (dict(block_table=None), INVALID, "null pointer: k_pool, v_pool and block_table are required"),
            (dict(heads_kv=0), INVALID, "batch, heads_kv, group, nq and nk must be >= 1"),
            (dict(page_size=24), UNSUPPORTED, "page_size 24 is not supported"),
            (dict(nk=2049), INVALID, "nk = 2049 exceeds max_pages * page_size = 2048"),
            (dict(scale=float("nan")), INVALID, "scale must be finite and non-zero"),
            *[(dict(k_scale=s), INVALID, "k_scale must be finite and > 0") for s in BAD_SCALES],
            *[(dict(v_scale=s), INVALID, "v_scale must be finite and > 0") for s in BAD_SCALES],
            (dict(scale=1e30, k_scale=1e30), INVALID, "scale * k_scale must be finite and non-zero in fp32"),
            (dict(ws=WS, ws_bytes=need - 1), INVALID, f"is too small: fa_kvw8_paged_workspace_bytes() = {need}"),
            (dict(o=POOL_K + 40 * page_bytes), INVALID, "o overlaps q, a pool"),
            (dict(o=TABLE), INVALID, "o overlaps q, a pool"),
            (dict(lse=LENS_P + 4), INVALID, "lse overlaps q, a pool, the block table, seq_lens or o"),
            (dict(ws=POOL_V, ws_bytes=need), INVALID, "the workspace overlaps a tensor of the call"),
            (dict(k_pool=POOL_K + 8), INVALID, "q, k_pool, v_pool, o must be 16-byte aligned"),
            (dict(block_table=TABLE + 2), INVALID, "block_table and seq_lens must be 4-byte aligned"),
            (dict(row_stride=2 * 128 + 8), INVALID, "must be multiples of 16 elements (16 bytes)"),   # a multiple of 8: not enough
            (dict(page_stride=64 * 2 * 128 + 8), INVALID, "must be multiples of 16 elements (16 bytes)"),
            (dict(head_stride=12), INVALID, "must be multiples of 16 elements (16 bytes)"),
            (dict(page_size=65536, max_pages=1, row_stride=65536, page_stride=1 << 32, heads_kv=1, head_stride=0, B=4), UNSUPPORTED, "must stay below 2^32 bytes"),
            (dict(ws=WS + 128, ws_bytes=need), INVALID, "workspace must be 256-byte aligned")]:
        rc, text = paged(**kw)
        assert rc == code and words in text, (kw, rc, text)
    assert L.fa_kvw8_paged_splits_for(2, 2, 4, 1, 2048, 128, 1, BF16, -1) == 0 and L.fa_kvw8_paged_workspace_bytes(2, 2, 4, 1, 2048, 128, 1, BF16, -1) == 0


# ---- the plan ----
def test_the_plan_is_the_windowed_16_bit_librarys_for_the_same_arguments():
    L, W = _cabi_kvw8.lib(), _cabi_kvw.lib()
    split = 0
    for bh, g, nq, nk in GRID:
        for w in (0, 1, 63, 64, 255, 1000, 4095, 30000, nk - 1, 1 << 24):
            for d, causal, dt in ((128, 1, BF16), (64, 0, BF16_F32)):
                S = L.fa_kvw8_splits_for(bh, g, nq, nk, d, causal, dt, w)
                assert 1 <= S <= 64 and S == W.fa_kvw_splits_for(bh, g, nq, nk, d, causal, dt, w), (bh, g, nq, nk, d, w)
                need = L.fa_kvw8_workspace_bytes(bh, g, nq, nk, d, causal, dt, w)
                assert need == W.fa_kvw_workspace_bytes(bh, g, nq, nk, d, causal, dt, w) and (need > 0) == (S > 1)
                split += S > 1
                # the paged queries: the contiguous ones at bh_kv = batch * heads_kv
                for H in (1, 2):
                    if bh % H == 0:
                        assert L.fa_kvw8_paged_splits_for(bh // H, H, g, nq, nk, d, causal, dt, w) == S
                        assert L.fa_kvw8_paged_workspace_bytes(bh // H, H, g, nq, nk, d, causal, dt, w) == need
    assert split > 100
    for bh in (1, 8, 1024):   # a short window on a long cache does not split
        assert L.fa_kvw8_splits_for(bh, 8, 1, 65536, 128, 1, BF16, 255) == 1 and L.fa_kvw8_workspace_bytes(bh, 8, 1, 65536, 128, 1, BF16, 255) == 0
    assert _cabi_kv8.lib().fa_kv8_splits_for(1, 8, 1, 65536, 128, 1, BF16) == 64 and L.fa_kvw8_splits_for(1, 8, 1, 65536, 128, 1, BF16, 4095) > 1


# ---- the code objects ----
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    out = {}
    for tag, path in (("kvw8", _cabi_kvw8.LIB_PATH), ("kv8", _cabi_kv8.LIB_PATH)):
        assert os.path.exists(path), "build the libraries first (python flashattention.c_amd/build.py)"
        ks = codeobj.kernels_of(path, str(tmp_path_factory.mktemp("co_" + tag)))
        dis = {}
        for co in sorted({k.code_object for k in ks.values()}):
            cur = None
            for ln in codeobj.disassemble(co).splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
                if m:
                    cur = dis.setdefault(m.group(1), [])
                elif cur is not None and ln.startswith("\t"):
                    ins, _, tail = ln.partition("//")
                    if tail.strip():
                        cur.append((int(tail.split(":")[0], 16), ins.strip()))
        out[tag] = {k.name: (k, [i for _, i in dis[k.mangled]], dis[k.mangled]) for k in ks.values()}
    return out


COUNTED = ("v_mfma", "global_load", "ds_read", "ds_write", "v_exp", "v_cvt_pk", "s_barrier")


def _profile(k, body):
    assert len(body) > 10, k.name
    counts = {p: sum(1 for ins in body if ins.split()[0].startswith(p)) for p in COUNTED}
    # LDS stores, not store instructions: the merge's (m, l) pair leaves hipcc as two ds_write_b32 or as one ds_write2st64_b32, as the register
    # allocation falls (in the unwindowed library: two in the contiguous d = 64 kernels, one in the paged ones)
    counts["ds_write"] += sum(1 for ins in body if ins.split()[0].startswith("ds_write2"))
    counts["ds_write instructions"] = sum(1 for ins in body if ins.split()[0].startswith("ds_write"))
    vmcnt = sorted(int(n) for ins in body if ins.startswith("s_waitcnt") for n in re.findall(r"vmcnt\((\d+)\)", ins))
    return dict(lds=k.lds, vmcnt=vmcnt, **counts)


def _occupancy(regs):
    """waves per SIMD the 512 registers of a lane allow (allocated in steps of 8)"""
    return 512 // ((regs + 7) // 8 * 8)


def _waits_in_the_loop(listing):
    """the vmcnt(N) immediates inside the decode loop: the spans of the backward branches that enclose matrix instructions (the loop is unrolled
    by two: a conditional exit behind the first step, the branch back behind the second)"""
    addr = [a for a, _ in listing]
    inside = set()
    for i, (a, ins) in enumerate(listing):
        m = re.match(r"s_c?branch\w*\s+(\d+)$", ins)
        if not m or int(m.group(1)) < 0x8000:
            continue
        target = a + 4 + (int(m.group(1)) - 0x10000) * 4
        j = addr.index(target)
        if any(x.startswith("v_mfma") for _, x in listing[j:i]):
            inside.update(range(j, i))
    assert inside
    return sorted(int(n) for i in inside if listing[i][1].startswith("s_waitcnt") for n in re.findall(r"vmcnt\((\d+)\)", listing[i][1]))


def test_every_windowed_kernel_keeps_the_profile_of_its_unwindowed_twin(kernels):
    """The window adds selects and clamps to a step, nothing else: the same LDS and the same matrix, load, LDS read, LDS store (a ds_write2 is
    two, see _profile), exponential, conversion and barrier counts as the kernel of libflashattn_amd_kv8.so with the same <D, CAUSAL, OUT_F32, PAGED>, no scratch, and no fewer waves
    per SIMD.

    Registers: a code object's vgpr_count is the lane's whole allocation in the unified file, accumulation registers included (agpr_count
    names the part of it that they take; the sum of the two exceeds 512 for half the unwindowed d = 128 kernels).  It is what must stay within 512
    and what bounds the waves per SIMD.

    vmcnt: hipcc does not give the windowed kernels the waits of their twins -- the prologues differ (docs/kv_window_fp8.md has both lists) -- so
    the lists are printed and what is held is what keeps the look-ahead: no vmcnt(0) the twin lacks, and every wait inside the loop leaves at
    least the loads of one block outstanding (2 K pieces per 16 columns and D / 16 V pieces: 3 D / 16) -- the next block's."""
    mine = {n: kb for n, kb in kernels["kvw8"].items() if "_decode_kernel<" in n}
    assert len(mine) == 16 and len(kernels["kvw8"]) == 16 + sum(1 for n in kernels["kvw8"] if "combine" in n), sorted(kernels["kvw8"])
    assert sum(1 for n in kernels["kvw8"] if "combine" in n) == 2
    bad = []
    for name, (k, body, listing) in sorted(mine.items()):
        m = re.match(r"void fa::fa_kvw8_decode_kernel<(\d+), (true|false), (true|false), (true|false)>\(fa::Kvw8Params\)$", name)
        assert m, name
        per_block = 3 * int(m.group(1)) // 16
        twin_name = f"void fa::fa_kv8_decode_kernel<{m.group(1)}, {m.group(2)}, {m.group(3)}, {m.group(4)}>(fa::Kv8Params)"
        tk, tbody, tlisting = kernels["kv8"][twin_name]
        assert k.scratch == 0 and tk.scratch == 0, name
        have, want = _profile(k, body), _profile(tk, tbody)
        loop, tloop = _waits_in_the_loop(listing), _waits_in_the_loop(tlisting)
        print(f"{name}: registers {k.vgprs} of which accumulation {k.agprs} (twin {tk.vgprs}, {tk.agprs}), instructions {len(body)} (twin {len(tbody)})\n"
              f"    windowed {have}\n    twin     {want}\n    vmcnt inside the loop: windowed {loop}\n                           twin     {tloop}")
        bad += [f"{name}\n    {f}: {want[f]} -> {have[f]}" for f in want if f not in ("vmcnt", "ds_write instructions") and have[f] != want[f]]
        assert have["ds_write instructions"] <= want["ds_write instructions"], name
        assert k.agprs <= k.vgprs <= 512 and tk.agprs <= tk.vgprs <= 512, name
        assert _occupancy(k.vgprs) >= _occupancy(tk.vgprs), (name, k.vgprs, tk.vgprs)
        assert have["vmcnt"].count(0) <= want["vmcnt"].count(0), (name, have["vmcnt"], want["vmcnt"])
        assert len(loop) >= 2 and min(loop) == per_block, (name, loop, tloop)
    assert not bad, "\n".join(bad)
