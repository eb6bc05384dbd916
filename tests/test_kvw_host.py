"""CPU: the sliding-window KV-cache library (include/flashattn_amd_kvw.h, libflashattn_amd_kvw.so) without a device: the fp64 reference
tests/kvw_reference.py pinned to tests/kv_reference.py, the header against the binding and the exports, every new or inherited check of the
host side through ctypes (no call reaches a launch, no pointer is dereferenced), the plan over the window's span, and the code objects of
its kernels held against their unwindowed counterparts in libflashattn_amd_kv.so / libflashattn_amd_paged.so (not against a snapshot)."""
import ctypes
import os
import re

import numpy as np
import pytest

from flashattention_c_amd import _cabi_kv, _cabi_kvw, _cabi_paged
from tests import codeobj
from tests.kv_reference import attention_kv
from tests.kvw_reference import attention_kvw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, BF16_F32, F32 = _cabi_kvw.FA_DTYPE_BF16, _cabi_kvw.FA_DTYPE_BF16_OUT_F32, _cabi_kvw.FA_DTYPE_F32
INVALID, UNSUPPORTED = 1, 2
A = 0x7f0000000000   # pointers that are never dereferenced: validation comes before any device call
G = 1 << 30


def rnd(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape)


# ---- the reference ----
@pytest.mark.parametrize("causal", [False, True])
def test_reference_without_a_window_is_attention_kv(causal):
    bh_kv, group, nq, nk, d = 3, 2, 5, 37, 8
    q, k, v = rnd(1, bh_kv * group, nq, d), rnd(2, bh_kv, nk, d), rnd(3, bh_kv, nk, d)
    for lens in (None, [37, 4, 0]):
        want = attention_kv(q, k, v, lens, causal, 0.3)
        for w in (nk - 1, nk, 1 << 24):
            got = attention_kvw(q, k, v, lens, causal, 0.3, w)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (lens, w)


@pytest.mark.parametrize("causal", [False, True])
def test_reference_of_one_row_is_attention_kv_on_the_slice(causal):
    bh_kv, group, nk, d = 2, 3, 50, 8
    q, k, v = rnd(4, bh_kv * group, 1, d), rnd(5, bh_kv, nk, d), rnd(6, bh_kv, nk, d)
    for w in (0, 1, 7, 48, 49):
        got = attention_kvw(q, k, v, None, causal, 0.5, w)
        lo = max(0, nk - 1 - w)
        want = attention_kv(q, k[:, lo:], v[:, lo:], None, causal, 0.5)
        assert np.allclose(got[0], want[0], rtol=0, atol=1e-14) and np.allclose(got[1], want[1], rtol=0, atol=1e-14), w


def test_reference_with_window_zero_causal_returns_the_last_value_row():
    bh_kv, group, nk, d = 3, 2, 20, 8
    q, k, v = rnd(7, bh_kv * group, 1, d), rnd(8, bh_kv, nk, d), rnd(9, bh_kv, nk, d)
    lens = [20, 7, 1]
    k[1, 7:], v[1, 7:], k[0, :19], v[0, :19] = np.nan, np.nan, np.nan, np.nan   # rows no query sees are never used
    o, lse = attention_kvw(q, k, v, lens, True, 1.0, 0)
    for s, n in enumerate(lens):
        for g in range(group):
            assert np.array_equal(o[s * group + g, 0], v[s, n - 1])
            assert abs(lse[s * group + g, 0] - np.dot(q[s * group + g, 0], k[s, n - 1])) < 1e-14   # one key: its score (summed in another order)


# ---- the ABI ----
def test_header_binding_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "flashattn_amd_kvw.h")).read()
    declared = set(re.findall(r"\b(fa_kvw_\w+)\(", text.split("#define FLASHATTN_AMD_KVW_ABI_VERSION")[1]))
    assert declared == set(_cabi_kvw.EXPORTED_SYMBOLS), declared ^ set(_cabi_kvw.EXPORTED_SYMBOLS)
    L = _cabi_kvw.lib()
    for s in _cabi_kvw.EXPORTED_SYMBOLS:
        assert getattr(L, s) is not None
    assert L.fa_kvw_version().startswith(b"flashattn_amd_kvw abi 1 gfx950")
    exported = os.popen(f"nm -D --defined-only {_cabi_kvw.LIB_PATH}").read()
    names = set(re.findall(r" T (fa_\w+)", exported))
    assert names == set(_cabi_kvw.EXPORTED_SYMBOLS), names ^ set(_cabi_kvw.EXPORTED_SYMBOLS)   # self-contained: no fa_kv_* / fa_paged_* symbol
    assert "fp8" in text and "window_left > 2^24" in text


# ---- errors: contiguous ----
Q, K, V, O, LSE, LENS, WS = A, A + 1 * G, A + 2 * G, A + 3 * G, A + 4 * G, A + 4 * G + (1 << 20), A + 5 * G


def contiguous(**kw):
    a = dict(q=Q, k=K, v=V, o=O, lse=None, B=2, group=4, nq=1, nk=4096, cap=4096, lens=None, d=128, scale=1.0, causal=1, dtype=BF16, window=1023,
             ws=None, ws_bytes=0)
    assert set(kw) <= set(a)
    a.update(kw)
    L = _cabi_kvw.lib()
    rc = L.fa_kvw_forward(a["q"], a["k"], a["v"], a["o"], a["lse"], a["B"], a["group"], a["nq"], a["nk"], a["cap"], a["lens"], a["d"], a["scale"],
                          a["causal"], a["dtype"], a["window"], a["ws"], a["ws_bytes"], None)
    return rc, L.fa_kvw_last_error().decode()


def test_contiguous_errors_reach_their_code_and_text():
    L = _cabi_kvw.lib()
    need = L.fa_kvw_workspace_bytes(2, 4, 1, 4096, 128, 1, BF16, 1023)
    assert need > 0
    slab = 4096 * 128 * 2
    for kw, code, words in [
            (dict(window=-1), INVALID, "window_left = -1 must be >= 0"),
            (dict(window=-(1 << 31)), INVALID, "must be >= 0"),
            (dict(dtype=F32), UNSUPPORTED, "FA_DTYPE_F32 is not supported: caches are 16-bit"),
            (dict(dtype=7), INVALID, "unknown dtype 7"),
            (dict(d=96), UNSUPPORTED, "head dim 96 is not supported: 64 or 128"),
            (dict(q=None), INVALID, "null pointer: q, k, v and o are required"),
            (dict(nk=0), INVALID, "bh_kv, group, nq and nk must be >= 1"),
            (dict(nk=4097), INVALID, "nk = 4097 exceeds capacity = 4096"),
            (dict(scale=0.0), INVALID, "scale must be finite and non-zero"),
            (dict(ws=WS, ws_bytes=need - 1), INVALID, f"is too small: fa_kvw_workspace_bytes() = {need}"),
            (dict(ws=WS, ws_bytes=1), INVALID, "is too small"),
            (dict(o=Q), INVALID, "o overlaps q, k or v"),
            (dict(o=K + slab), INVALID, "o overlaps q, k or v"),
            (dict(lse=V + 2 * slab - 4), INVALID, "lse overlaps q, k, v or o"),
            (dict(ws=V, ws_bytes=need), INVALID, "the workspace overlaps a tensor of the call"),
            (dict(lens=WS + 512, ws=WS, ws_bytes=need), INVALID, "the workspace overlaps a tensor of the call"),
            (dict(q=Q + 8), INVALID, "q, k, v, o must be 16-byte aligned"),
            (dict(v=V + 8), INVALID, "q, k, v, o must be 16-byte aligned"),
            (dict(lse=LSE + 2), INVALID, "lse must be 4-byte aligned"),
            (dict(lens=LENS + 1), INVALID, "kv_lens must be 4-byte aligned"),
            (dict(ws=WS + 128, ws_bytes=need), INVALID, "workspace must be 256-byte aligned")]:
        rc, text = contiguous(**kw)
        assert rc == code and words in text, (kw, rc, text)
    # a window the plan does not split under needs no workspace: the same small one is then accepted by the plan (and rejected for nothing else
    # before the launch, which this test must not reach -- so only the query is asked)
    assert L.fa_kvw_workspace_bytes(2, 4, 1, 4096, 128, 1, BF16, 100) == 0
    # the queries answer 0 / NULL to what the forward rejects
    for args in [(2, 4, 1, 4096, 128, 1, BF16, -1), (2, 4, 1, 4096, 96, 1, BF16, 5), (2, 4, 1, 4096, 128, 1, F32, 5), (0, 4, 1, 4096, 128, 1, BF16, 5)]:
        assert L.fa_kvw_workspace_bytes(*args) == 0 and L.fa_kvw_splits_for(*args) == 0 and L.fa_kvw_kernel_name_for(*args) is None
    assert L.fa_kvw_kernel_name_for(2, 4, 1, 4096, 128, 1, BF16, 5) == b"fa_kvw_decode_kernel"


# ---- errors: paged.  2 sequences x 2 heads, (pages, page, H, d) pools of 64 pages of 64 rows ----
POOL_K, POOL_V, TABLE, LENS_P, OP, LSE_P = A + 1 * G, A + 2 * G, A + 3 * G, A + 3 * G + (1 << 20), A + 4 * G, A + 6 * G


def paged(**kw):
    a = dict(q=Q, o=OP, lse=None, cache=True, B=2, heads_kv=2, group=4, nq=1, nk=2048, d=128, scale=1.0, causal=1, dtype=BF16, window=1023, ws=None, ws_bytes=0)
    f = dict(k_pool=POOL_K, v_pool=POOL_V, num_pages=64, page_size=64, page_stride=64 * 2 * 128, row_stride=2 * 128, head_stride=128, block_table=TABLE,
             max_pages=32, seq_lens=LENS_P)
    assert set(kw) <= set(a) | set(f)
    a.update({k: v for k, v in kw.items() if k in a})
    f.update({k: v for k, v in kw.items() if k in f})
    cache = ctypes.byref(_cabi_kvw.FaPagedCache(**f)) if a["cache"] else None
    L = _cabi_kvw.lib()
    rc = L.fa_kvw_paged_forward(a["q"], cache, a["o"], a["lse"], a["B"], a["heads_kv"], a["group"], a["nq"], a["nk"], a["d"], a["scale"], a["causal"],
                                a["dtype"], a["window"], a["ws"], a["ws_bytes"], None)
    return rc, L.fa_kvw_last_error().decode()


def test_paged_errors_reach_their_code_and_text():
    L = _cabi_kvw.lib()
    need = L.fa_kvw_paged_workspace_bytes(2, 2, 4, 1, 2048, 128, 1, BF16, 1023)
    assert need > 0 and need == L.fa_kvw_workspace_bytes(4, 4, 1, 2048, 128, 1, BF16, 1023)
    page_bytes = 64 * 2 * 128 * 2
    for kw, code, words in [
            (dict(window=-1), INVALID, "window_left = -1 must be >= 0"),
            (dict(dtype=F32), UNSUPPORTED, "FA_DTYPE_F32 is not supported: caches are 16-bit"),
            (dict(d=96), UNSUPPORTED, "head dim 96 is not supported: 64 or 128"),
            (dict(cache=False), INVALID, "null pointer: q, cache and o are required"),
            (dict(block_table=None), INVALID, "null pointer: k_pool, v_pool and block_table are required"),
            (dict(heads_kv=0), INVALID, "batch, heads_kv, group, nq and nk must be >= 1"),
            (dict(page_size=24), UNSUPPORTED, "page_size 24 is not supported"),
            (dict(nk=2049), INVALID, "nk = 2049 exceeds max_pages * page_size = 2048"),
            (dict(ws=WS, ws_bytes=need - 1), INVALID, f"is too small: fa_kvw_paged_workspace_bytes() = {need}"),
            (dict(o=POOL_K + 40 * page_bytes), INVALID, "o overlaps q, a pool"),
            (dict(o=TABLE), INVALID, "o overlaps q, a pool"),
            (dict(lse=LENS_P + 4), INVALID, "lse overlaps q, a pool, the block table, seq_lens or o"),
            (dict(ws=POOL_V, ws_bytes=need), INVALID, "the workspace overlaps a tensor of the call"),
            (dict(k_pool=POOL_K + 8), INVALID, "q, k_pool, v_pool, o must be 16-byte aligned"),
            (dict(block_table=TABLE + 2), INVALID, "block_table and seq_lens must be 4-byte aligned"),
            (dict(row_stride=2 * 128 + 12), INVALID, "must be multiples of 8 elements (16 bytes)"),
            (dict(ws=WS + 128, ws_bytes=need), INVALID, "workspace must be 256-byte aligned")]:
        rc, text = paged(**kw)
        assert rc == code and words in text, (kw, rc, text)
    assert L.fa_kvw_paged_splits_for(2, 2, 4, 1, 2048, 128, 1, BF16, -1) == 0 and L.fa_kvw_paged_workspace_bytes(2, 2, 4, 1, 2048, 128, 1, BF16, -1) == 0


# ---- the plan ----
GRID = [(bh, g, nq, nk) for bh in (1, 2, 8, 64, 300) for g in (1, 4, 8) for nq in (1, 5, 33) for nk in (1, 63, 256, 511, 512, 1000, 4099, 65536)]


def test_a_window_that_hides_nothing_plans_like_the_unwindowed_library():
    L, KV, PG = _cabi_kvw.lib(), _cabi_kv.lib(), _cabi_paged.lib()
    for bh, g, nq, nk in GRID:
        for d in (64, 128):
            for w in (nk - 1, nk, nk + 100, 1 << 24, (1 << 31) - 1):
                assert L.fa_kvw_splits_for(bh, g, nq, nk, d, 1, BF16, w) == KV.fa_kv_splits_for(bh, g, nq, nk, d, 1, BF16), (bh, g, nq, nk, w)
                assert L.fa_kvw_workspace_bytes(bh, g, nq, nk, d, 0, BF16_F32, w) == KV.fa_kv_workspace_bytes(bh, g, nq, nk, d, 0, BF16_F32)
            assert L.fa_kvw_paged_splits_for(bh, 2, g, nq, nk, d, 1, BF16, nk - 1) == PG.fa_paged_splits_for(bh, 2, g, nq, nk, d, 1, BF16)
            assert L.fa_kvw_paged_workspace_bytes(bh, 2, g, nq, nk, d, 1, BF16, nk - 1) == PG.fa_paged_workspace_bytes(bh, 2, g, nq, nk, d, 1, BF16)


def test_the_plan_is_that_of_a_cache_of_span_keys_and_covers_every_tile():
    """share is not exported; the plan is kv_plan over span = min(nk, window_left + nq + 63), so splits and workspace are those of the unwindowed
    library for a cache of span keys, whose shares (multiples of 64 keys, ceil(span / S) rounded up) cover span.  Lengths are no argument of
    either query: the plan cannot depend on them."""
    L, KV = _cabi_kvw.lib(), _cabi_kv.lib()
    for bh, g, nq, nk in GRID:
        for w in (0, 1, 63, 64, 255, 1000, 4095, 30000):
            span = min(nk, w + nq + 63)
            S = L.fa_kvw_splits_for(bh, g, nq, nk, 128, 1, BF16, w)
            assert 1 <= S <= 64 and S == KV.fa_kv_splits_for(bh, g, nq, span, 128, 1, BF16), (bh, g, nq, nk, w)
            share = ((span + S - 1) // S + 63) // 64 * 64
            assert S * share >= span and (S == 1 or (S - 1) * share < span)
            assert L.fa_kvw_workspace_bytes(bh, g, nq, nk, 128, 1, BF16, w) == KV.fa_kv_workspace_bytes(bh, g, nq, span, 128, 1, BF16)
            assert L.fa_kvw_paged_splits_for(bh, 1, g, nq, nk, 128, 1, BF16, w) == S
            if span < 512:
                assert S == 1   # fewer than 512 keys are never split


def test_a_short_window_on_a_long_cache_does_not_split():
    L = _cabi_kvw.lib()
    for bh in (1, 8, 1024):
        assert L.fa_kvw_splits_for(bh, 8, 1, 65536, 128, 1, BF16, 255) == 1
        assert L.fa_kvw_workspace_bytes(bh, 8, 1, 65536, 128, 1, BF16, 255) == 0
    assert _cabi_kv.lib().fa_kv_splits_for(1, 8, 1, 65536, 128, 1, BF16) == 64
    assert L.fa_kvw_splits_for(1, 8, 1, 65536, 128, 1, BF16, 4095) > 1


# ---- the code objects ----
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    out = {}
    for tag, path in (("kvw", _cabi_kvw.LIB_PATH), ("kv", _cabi_kv.LIB_PATH), ("paged", _cabi_paged.LIB_PATH)):
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
                    cur.append(ln.split("//")[0].strip())
        out[tag] = {k.name: (k, dis[k.mangled]) for k in ks.values()}
    return out


COUNTED = ("v_mfma", "global_load", "ds_read", "v_exp", "s_barrier")


def _profile(k, body):
    assert len(body) > 10, k.name
    counts = {p: sum(1 for ins in body if ins.split()[0].startswith(p)) for p in COUNTED}
    vmcnt = sorted(int(n) for ins in body if ins.startswith("s_waitcnt") for n in re.findall(r"vmcnt\((\d+)\)", ins))
    return dict(lds=k.lds, vmcnt=vmcnt, **counts)


def _occupancy(regs):
    """waves per SIMD the 512 registers of a lane allow (allocated in steps of 8)"""
    return 512 // ((regs + 7) // 8 * 8)


def test_every_windowed_kernel_keeps_the_profile_of_its_unwindowed_counterpart(kernels):
    mine = {n: kb for n, kb in kernels["kvw"].items() if "_decode_kernel<" in n}
    assert len(mine) == 16 and len(kernels["kvw"]) == 16 + sum(1 for n in kernels["kvw"] if "combine" in n), sorted(kernels["kvw"])
    bad = []
    for name, (k, body) in sorted(mine.items()):
        m = re.match(r"void fa::fa_kvw_(paged_)?decode_kernel<(\d+), (true|false), (true|false)>\(fa::Kvw(Paged)?Params\)$", name)
        assert m, name
        pg, d, args = bool(m.group(1)), int(m.group(2)), f"<{m.group(2)}, {m.group(3)}, {m.group(4)}>"
        twin_name = f"void fa::fa_paged_decode_kernel{args}(fa::PagedParams)" if pg else f"void fa::fa_kv_decode_kernel{args}(fa::KvParams)"
        tk, tbody = kernels["paged" if pg else "kv"][twin_name]
        assert k.scratch == 0, name
        have, want = _profile(k, body), _profile(tk, tbody)
        print(f"{name}: regs {k.vgprs + k.agprs} (counterpart {tk.vgprs + tk.agprs}), instructions {len(body)} (counterpart {len(tbody)}), {have}")
        bad += [f"{name}\n    {f}: {want[f]} -> {have[f]}" for f in want if have[f] != want[f]]
        assert k.vgprs + k.agprs <= 512, name
        if d == 64:
            assert _occupancy(k.vgprs + k.agprs) >= _occupancy(tk.vgprs + tk.agprs), (name, k.vgprs + k.agprs, tk.vgprs + tk.agprs)
    assert not bad, "\n".join(bad)
