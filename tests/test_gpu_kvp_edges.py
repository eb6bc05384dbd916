"""GPU: the edges of the chunked-prefill kernels (csrc/fa_kvp_prefill_loop.h; fa.prefill_kv / fa.prefill_paged and the _fp8 entries) that
the parity tests of tests/test_gpu_kvp.py and tests/test_gpu_kvp8.py do not reach: the causal tile order with several tiles per head and
several heads per slab, output buffers that hold 0xFF before the call, a guard-band arena around all four entries, softmax inputs on which
single rows decide the rescale branch (tests/kvp_cases.py), pages larger than the 64-key block, shared pages, pools beyond 4 GiB, and lengths
outside [0, nk].

References: tests/kv_reference.py (fp64) on the logical values, tests/paged_reference.py for the gathered cache.  Every bar is imported:
    fp32 output  TOL_PB2 = 2e-4      LSE  TOL_LSE = 1e-4      bf16 output  TOL_BF16 = 2.5e-2
and the one relative bar, 2^-20 on an LSE of 2^19 .. 2^20, is that of tests/test_gpu_kv.py::test_a_key_far_above_the_rest_and_a_constant_v
with its reasoning (the fp32 roundings of m * ln 2 and of the sum, 2^-23 each).  "lib" is bf16 (libflashattn_amd_kvp.so) or fp8
(libflashattn_amd_kvp8.so); the Gaussian data of the fp8 library is that of tests/test_gpu_kvp8.py (k_scale = 0.013, v_scale = 0.011).
Whatever a call must not read holds NaN (bf16) or the NaN code 0xFF (fp8), inside an allocation: a wrong read is a NaN in the result.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import flashattention_c_amd as fa
from flashattention_c_amd import _cabi_kvp, _cabi_kvp8
from tests import arena as ar
from tests import kvp_cases as kc
from tests.kv8_reference import dequant
from tests.kv_reference import attention_kv
from tests.paged_reference import gather
from tests.test_gpu_kvp import TOL_BF16, TOL_LSE, TOL_PB2, cache, dev, err, randn, to_dev
from tests.test_gpu_kvp8 import KS, VS, cache8, codes, to_dev8

pytestmark = pytest.mark.gpu

D = 128
F8 = torch.float8_e4m3fn
NAN = float("nan")
BARS = ((torch.float32, TOL_PB2), (torch.bfloat16, TOL_BF16))
LIBS = ["bf16", "fp8"]
BF16, BF16_F32 = _cabi_kvp.FA_DTYPE_BF16, _cabi_kvp.FA_DTYPE_BF16_OUT_F32
IDS = dict(ids=lambda x: "-".join("full" if y is None else "lens" if isinstance(y, list) else str(y) for y in x) if isinstance(x, tuple) else None)


def poisoned(shape, dtype):
    t = torch.empty(tuple(shape), dtype=dtype, device=dev())
    ar.fill_bytes(t, ar.POISON)
    return t


class Gauss:
    """N(0, 1) data of one library: q, the logical k and v (fp64 arrays the reference takes) and what the cache stores (`kraw`, `vraw`: the bf16
    values, or the e4m3 codes), with the library's calls"""

    def __init__(self, lib, seed, bh_kv, group, nq, nk):
        self.fp8 = lib == "fp8"
        self.q = randn(seed, bh_kv * group, nq, D)
        if self.fp8:
            self.kraw, self.vraw = codes(seed + 1, KS, bh_kv, nk, D), codes(seed + 2, VS, bh_kv, nk, D)
            self.k, self.v = KS * dequant(self.kraw), VS * dequant(self.vraw)
            self.fill, self.scales = 0xFF, dict(k_scale=KS, v_scale=VS)
        else:
            self.k = self.kraw = randn(seed + 1, bh_kv, nk, D)
            self.v = self.vraw = randn(seed + 2, bh_kv, nk, D)
            self.fill, self.scales = NAN, {}

    def raw_to_dev(self, a):
        """stored values -> device tensor of the cache's dtype"""
        return to_dev8(np.ascontiguousarray(a)) if self.fp8 else to_dev(a)   # (to_dev8 alone keeps a transposed array's strides)

    def raw_bytes(self, a):
        """... of the dtype an arena buffer of this cache has (fp8: uint8)"""
        return torch.from_numpy(np.array(a, dtype=np.uint8)).to(dev()) if self.fp8 else to_dev(a)

    def cache(self, a, capacity, lens):
        return cache8(a, capacity, lens) if self.fp8 else cache(a, capacity, lens)

    def prefill(self, *a, **kw):
        return (fa.prefill_kv_fp8 if self.fp8 else fa.prefill_kv)(*a, **self.scales, **kw)

    def prefill_paged(self, *a, **kw):
        return (fa.prefill_paged_fp8 if self.fp8 else fa.prefill_paged)(*a, **self.scales, **kw)


def build_pool(k, v, batch, H, lens, page, fill, seed, spare=5, max_pages=None):
    """Pools (pages, page, H, D) of the dtype of k, v ((batch * H, nk, D)) under a shuffled table: `fill` in every row no sequence owns (unused
    pages, page tails); every table entry at or beyond ceil(len / page) names a spare page, which exists and holds `fill`.  Returns kp, vp,
    the table and the spare pages."""
    nk = k.shape[1]
    used = [-(-n // page) for n in lens]
    max_pages = max_pages or -(-nk // page) + 2
    pages = sum(used) + spare
    order = [int(x) for x in np.random.default_rng(seed).permutation(pages)]
    free = order[sum(used):]
    table = np.empty((batch, max_pages), dtype=np.int32)
    kp, vp = np.full((pages, page, H, D), fill, dtype=k.dtype), np.full((pages, page, H, D), fill, dtype=v.dtype)
    at = 0
    for b, n in enumerate(lens):
        table[b] = [free[(b + i) % len(free)] for i in range(max_pages)]
        for p in range(used[b]):
            phys, rows = order[at], min(page, n - p * page)
            at += 1
            table[b, p] = phys
            for pool, src in ((kp, k), (vp, v)):
                pool[phys, :rows] = src[b * H:(b + 1) * H, p * page:p * page + rows].transpose(1, 0, 2)
    return kp, vp, table, free


# ---- 1. every tile, once, in any order ----------------------------------------------------------------------------------------------------
# (bh_kv, group, nq, nk)
TILES = [
    (2, 2, 512, 600),    # nq % 256 == 0 with group = 2, per_head = 2: the tile formula is no identity
    (1, 3, 256, 300),    # per_head = 1, group = 3
    (1, 1, 768, 800),    # group = 1, per_head = 3
    (3, 3, 200, 260),    # M = 600: three tiles that straddle heads, the tiles - 1 - u order; bh_kv no power of two
    (2, 1, 512, 200),    # causal: the first tile of every slab sees no key and must store 0 / -inf over the poison
]


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", TILES, **IDS)
def test_every_tile_is_written_once_in_any_order(shape, causal, lib):
    bh_kv, group, nq, nk = shape
    g = Gauss(lib, 201, bh_kv, group, nq, nk)
    qd, kd, vd = to_dev(g.q), g.cache(g.kraw, nk + 70, [nk] * bh_kv), g.cache(g.vraw, nk + 70, [nk] * bh_kv)
    ref, lse_ref = attention_kv(g.q, g.k, g.v, None, causal, 1.0)
    for odt, tol in BARS:
        out = poisoned(g.q.shape, odt)
        o, lse = g.prefill(qd, kd, vd, causal, kv_len=nk, out=out, return_lse=True)
        assert o is out and o.dtype == odt
        assert err(o, ref, f"tiles/{lib}/{odt}/o {shape} causal={causal}") < tol
        assert err(lse, lse_ref, f"tiles/{lib}/{odt}/lse {shape} causal={causal}") < TOL_LSE
        if causal and nq > nk:   # rows i < nq - nk see nothing: exactly 0 over the poison, LSE -inf (checked in err())
            assert not ref[:, :nq - nk].any() and not o[:, :nq - nk].any()
        if not g.fp8 and odt == torch.float32:   # the decode kernel: the same arithmetic contract under an independent work split
            od = fa.forward_kv(qd, kd, vd, causal, kv_len=nk, out_dtype=torch.float32)
            e = float((o - od).abs().max())
            print(f"tiles/bf16/prefill_kv vs forward_kv {shape} causal={causal}: {e:.3e}")
            assert e < 2 * TOL_PB2


# ---- 2. bounds: q, K, V (or the pools), o and lse in one guard-band arena at the minimum alignments, through the C ABI ---------------------
def _fill(t, mode, seed, fp8):
    if mode == "nan":
        ar.fill_bytes(t, ar.POISON)
    elif fp8:   # finite codes: never 0x7F / 0xFF
        t.view(-1).copy_(ar.finite_e4m3_bytes(t.numel(), t.device, torch.Generator(device=t.device).manual_seed(seed)))
    else:
        t.copy_(torch.randn(t.shape, device=t.device, generator=torch.Generator(device=t.device).manual_seed(seed)).to(t.dtype))


def _arena(g, bhq, nq, kv_shape, out_f32):
    edt, es = (torch.uint8, 1) if g.fp8 else (torch.bfloat16, 2)
    odt = torch.float32 if out_f32 else torch.bfloat16
    A = ar.Arena([ar.Buf("q", "in", torch.bfloat16, (bhq, nq, D), "tensor", D * 2),
                  ar.Buf("k", "in", edt, kv_shape, "tensor", D * es), ar.Buf("v", "in", edt, kv_shape, "tensor", D * es),
                  ar.Buf("o", "out", odt, (bhq, nq, D), "tensor", D * (4 if out_f32 else 2)), ar.Buf("lse", "out", torch.float32, (bhq, nq), "lse", 4)], dev())
    A.view("q").copy_(to_dev(g.q))
    return A


def _surroundings(A, g, mode, seed):
    A.fill_input_surroundings(mode, seed)
    if g.fp8 and mode == "finite":
        A.fill_input_guards_e4m3(("k", "v"), seed)
    A.fill_output_guards()
    ar.fill_bytes(A.view("o"), ar.POISON)
    ar.fill_bytes(A.view("lse"), ar.POISON)


def _checked(A, g, rc, runs, ref, lse_ref, out_f32, mode):
    mod = _cabi_kvp8 if g.fp8 else _cabi_kvp
    mod.check(rc)
    torch.cuda.synchronize()
    assert A.guards_intact(), str(A.first_damage())
    runs.append((A.view("o").clone(), A.view("lse").clone()))
    assert err(runs[-1][0], ref, f"o, {mode} surroundings") < (TOL_PB2 if out_f32 else TOL_BF16)
    assert err(runs[-1][1], lse_ref, f"lse, {mode} surroundings") < TOL_LSE


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


BOUNDS = [
    # (bh_kv, group, nq, nk, kv_lens)
    (3, 4, 5, 300, [300, 17, 0]),      # M = 20: no multiple of 32; a slab of 17 keys and an empty one
    (3, 4, 70, 321, [321, 17, 0]),     # M = 256 + 24: a second tile with three empty waves
    (2, 4, 70, 321, None),
]


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("out_f32", [True, False])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", BOUNDS, **IDS)
def test_memory_bounds_and_isolation(case, causal, out_f32, lib):
    bh_kv, group, nq, nk, lens = case
    g = Gauss(lib, 91, bh_kv, group, nq, nk)
    L = (_cabi_kvp8 if g.fp8 else _cabi_kvp).lib()
    dt = BF16_F32 if out_f32 else BF16
    cap, bhq = nk + 70, bh_kv * group
    A = _arena(g, bhq, nq, (bh_kv + 1, cap, D), out_f32)   # one K/V slab more than the call covers: the cache of a neighbouring call
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev()) if lens else None
    eff = lens if lens else [nk] * bh_kv
    ref, lse_ref = attention_kv(g.q, g.k, g.v, lens, causal, 1.0)
    runs = []
    for mode, seed in (("nan", 0), ("finite", 7)):
        _surroundings(A, g, mode, seed)
        for name, src in (("k", g.kraw), ("v", g.vraw)):
            t = A.view(name)
            _fill(t, mode, seed + 1, g.fp8)                  # rows [len, capacity) of every slab and the neighbour's slab ...
            for s, n in enumerate(eff):
                t[s, :n] = g.raw_bytes(src[s, :n])           # ... around the rows the call may read
        head = (A.ptr("q"), A.ptr("k"), A.ptr("v"), A.ptr("o"), A.ptr("lse"), bh_kv, group, nq, nk, cap, lens_d.data_ptr() if lens else None, D, 1.0)
        if g.fp8:
            rc = L.fa_kvp8_forward(*head, KS, VS, int(causal), dt, _stream())
        else:
            rc = L.fa_kvp_forward(*head, int(causal), dt, _stream())
        _checked(A, g, rc, runs, ref, lse_ref, out_f32, mode)
    assert ar.bit_equal(runs[0][0], runs[1][0]) and ar.bit_equal(runs[0][1], runs[1][1]), "the result depends on memory the call must not read"


PAGED_BOUNDS = [
    # (batch, heads_kv, group, nq, nk, page, seq_lens)
    (3, 1, 4, 5, 300, 64, [300, 17, 0]),       # M = 20, pages of one key block
    (2, 2, 4, 70, 321, 16, [321, 17]),         # M = 256 + 24, two heads interleaved in every page of 16
    (2, 2, 4, 70, 321, 16, None),
]


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("out_f32", [True, False])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", PAGED_BOUNDS, **IDS)
def test_memory_bounds_and_isolation_paged(case, causal, out_f32, lib):
    batch, H, group, nq, nk, page, lens = case
    bh_kv, bhq = batch * H, batch * H * group
    g = Gauss(lib, 91, bh_kv, group, nq, nk)
    L = (_cabi_kvp8 if g.fp8 else _cabi_kvp).lib()
    dt = BF16_F32 if out_f32 else BF16
    eff = lens if lens else [nk] * batch
    kp, vp, table0, free = build_pool(g.kraw, g.vraw, batch, H, eff, page, g.fill, seed=11, spare=7)   # the assignment, the table, the valid rows
    P = kp.shape[0]
    valid = torch.from_numpy((kp != 0xFF) if g.fp8 else ~np.isnan(kp)).to(dev())                       # the same rows in both pools
    pools = {"k": g.raw_bytes(kp), "v": g.raw_bytes(vp)}
    A = _arena(g, bhq, nq, (P, page, H, D), out_f32)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev()) if lens else None
    ref, lse_ref = attention_kv(g.q, g.k, g.v, [n for n in eff for _ in range(H)], causal, 1.0)
    runs = []
    for mode, seed in (("nan", 0), ("finite", 7)):
        _surroundings(A, g, mode, seed)
        for name in ("k", "v"):
            t = A.view(name)
            _fill(t, mode, seed + 1, g.fp8)                  # unused pages and the tails of last pages ...
            t[valid] = pools[name][valid]                    # ... around the rows the call may read
        table = table0.copy()
        for b, n in enumerate(eff):                          # entries past the length: another page that exists, per mode
            table[b, -(-n // page):] = free[(b + (mode == "finite")) % len(free)]
        table_d = torch.from_numpy(table).to(dev())
        pc = _cabi_kvp.FaPagedCache(A.ptr("k"), A.ptr("v"), P, page, page * H * D, H * D, D, table_d.data_ptr(), table.shape[1],
                                    lens_d.data_ptr() if lens else None)
        head = (A.ptr("q"), ctypes.byref(pc), A.ptr("o"), A.ptr("lse"), batch, H, group, nq, nk, D, 1.0)
        if g.fp8:
            rc = L.fa_kvp8_paged_forward(*head, KS, VS, int(causal), dt, _stream())
        else:
            rc = L.fa_kvp_paged_forward(*head, int(causal), dt, _stream())
        _checked(A, g, rc, runs, ref, lse_ref, out_f32, mode)
    assert ar.bit_equal(runs[0][0], runs[1][0]) and ar.bit_equal(runs[0][1], runs[1][1]), "the result depends on memory the call must not read"


# ---- 3. structured softmax: single rows decide the rescale branch (tests/kvp_cases.py) -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def struct_case(family, nk):
    return kc.make(family, nk)


def lse_ok(lse, lse_ref, what, large):
    """the absolute bar; where the reference is 2^18 or more (the large spike at scale 1 and 1/2) the relative bar 2^-20"""
    got = lse.detach().cpu().numpy().astype(np.float64)
    big = np.isfinite(lse_ref) & (lse_ref >= 2.0 ** 18)
    assert large or not big.any()
    if big.any():
        rel = float(np.abs(got[big] / lse_ref[big] - 1.0).max())
        print(f"{what}: max rel err {rel:.3e} on {int(big.sum())} rows")
        assert rel < 2.0 ** -20, what
    e = err(torch.from_numpy(np.where(big, 0.0, got)), np.where(big, 0.0, lse_ref), what)
    assert e < TOL_LSE, what


def both_libraries(case, q, kcodes, vcodes, capacity, lens, nk, causal, scales=(1.0, 0.5), what=""):
    """The bf16 library on the dequantised cache (the codes' values as bf16, k_scale folded into `scale`, v_scale applied to the result: exact,
    the scales are powers of two) and the fp8 library on the codes: poisoned outputs, both output dtypes, O and LSE against fp64 on the
    logical values at the bars, and the two libraries bit for bit."""
    large = case.name == "lone_mover_large"
    qd = to_dev(q)
    eff = lens if lens is not None else [nk] * len(kcodes)
    k8, v8 = cache8(kcodes, capacity, eff), cache8(vcodes, capacity, eff)
    kb, vb = (t.view(torch.uint8).cpu().view(F8).to(torch.bfloat16).to(dev()) for t in (k8, v8))   # exact; a NaN code becomes a bf16 NaN
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev())
    k, v = case.k_scale * dequant(kcodes), case.v_scale * dequant(vcodes)
    for scale in scales:
        ref, lse_ref = attention_kv(q, k, v, lens, causal, scale)
        for odt, tol in BARS:
            ob, lseb = fa.prefill_kv(qd, kb, vb, causal, kv_len=nk, kv_lens=lens_d, scale=float(np.float32(scale) * np.float32(case.k_scale)),
                                     out=poisoned(q.shape, odt), return_lse=True)
            ob = (case.v_scale * ob.float()).to(odt)
            o8, lse8 = fa.prefill_kv_fp8(qd, k8, v8, causal, k_scale=case.k_scale, v_scale=case.v_scale, kv_len=nk, kv_lens=lens_d, scale=scale,
                                         out=poisoned(q.shape, odt), return_lse=True)
            for lib, o, lse in (("bf16", ob, lseb), ("fp8", o8, lse8)):
                tag = f"struct/{case.name}/{lib}/{odt}"
                assert err(o, ref, f"{tag}/o {what} causal={causal} scale={scale}") < tol, tag
                lse_ok(lse, lse_ref, f"{tag}/lse {what} causal={causal} scale={scale}", large)
            assert ar.bit_equal(o8, ob) and ar.bit_equal(lse8, lseb), f"fp8 on the codes and bf16 on the dequantised cache differ ({case.name}, {odt}, {scale})"


# (group, nq, nk): bh_kv = 1
STRUCT = [
    (4, 70, 321),      # a ragged last block; M = 280: a partial second tile; with shift = 32 the four heads use all 128 profiles
    (1, 256, 256),     # the diagonal through every wave
]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", STRUCT, **IDS)
@pytest.mark.parametrize("family", kc.FAMILIES)
def test_structured_softmax(family, shape, causal):
    group, nq, nk = shape
    case = struct_case(family, nk)
    q = case.q(group, nq, shift=32)
    both_libraries(case, q, case.k_codes[None], case.v_codes[None], nk + 70, None, nk, causal, what=str(shape))
    if family == "lone_mover_large":   # a constant V on the grid comes out exactly, for both output dtypes, whichever rows rescale
        # 0x40: 2.0.  A power of two: c * (a + b) rounds like c * a + c * b only then, so only then do O's sums stay c x the row sum's
        # (with 1.5 the rows whose spike the causal mask hides differ from 1.5 in the last bit, in the decode kernel as well)
        qd, const = to_dev(q), np.full((1, nk, D), 0x40, dtype=np.uint8)
        k8, v8 = cache8(case.k_codes[None], nk + 70, [nk]), cache8(const, nk + 70, [nk])
        kb, vb = (t.view(torch.uint8).cpu().view(F8).to(torch.bfloat16).to(dev()) for t in (k8, v8))
        for odt in (torch.float32, torch.bfloat16):   # nq <= nk: every row sees a key
            o8 = fa.prefill_kv_fp8(qd, k8, v8, causal, k_scale=case.k_scale, v_scale=case.v_scale, kv_len=nk, out=poisoned(q.shape, odt))
            assert torch.equal(o8, torch.full_like(o8, 2.0 * float(np.float32(case.v_scale)))), (causal, odt)
            ob = fa.prefill_kv(qd, kb, vb, causal, kv_len=nk, scale=case.k_scale, out=poisoned(q.shape, odt))
            assert torch.equal(ob, torch.full_like(ob, 2.0)), (causal, odt)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", ["staircase_up", "lone_mover"])
def test_late_start_with_lengths_from_device_memory(family, causal):
    p = kc.late_start()
    nq, nk, group, lens = p["nq"], p["nk"], p["group"], p["kv_lens"]
    case = struct_case(family, nk)
    kcodes, vcodes = (np.repeat(x[None], len(lens), axis=0) for x in (case.k_codes, case.v_codes))
    both_libraries(case, case.q(len(lens) * group, nq, shift=32), kcodes, vcodes, nk, lens, nk, causal, scales=(1.0,), what="late start")


# ---- 4. paged beyond the small pages -----------------------------------------------------------------------------------------------------
def paged_equals_contiguous(g, batch, H, lens, nk, kp, vp, table, permuted=False, causals=(False, True)):
    """fa.prefill_paged* on the pools against fp64 at the bars and, bit for bit, against fa.prefill_kv* on the gathered cache"""
    qd, table_d = to_dev(g.q), torch.from_numpy(table).to(dev())
    if permuted:
        kpd, vpd = (g.raw_to_dev(x.transpose(0, 2, 1, 3)).permute(0, 2, 1, 3) for x in (kp, vp))
        assert not kpd.is_contiguous() or H == 1
    else:
        kpd, vpd = g.raw_to_dev(kp), g.raw_to_dev(vp)
    slab_lens = [n for n in lens for _ in range(H)]
    gk, gv = gather(kp, table, lens, nk), gather(vp, table, lens, nk)
    for s, n in enumerate(slab_lens):   # what the gather leaves past a length
        gk[s, n:], gv[s, n:] = g.fill, g.fill
    kd, vd = g.raw_to_dev(gk), g.raw_to_dev(gv)
    lens_d, slab_lens_d = (torch.tensor(x, dtype=torch.int32, device=dev()) for x in (lens, slab_lens))
    for causal in causals:
        ref, lse_ref = attention_kv(g.q, g.k, g.v, slab_lens, causal, 1.0)
        for odt, tol in BARS:
            o, lse = g.prefill_paged(qd, kpd, vpd, table_d, causal, kv_len=nk, seq_lens=lens_d, out=poisoned(g.q.shape, odt), return_lse=True)
            oc, lsec = g.prefill(qd, kd, vd, causal, kv_len=nk, kv_lens=slab_lens_d, out=poisoned(g.q.shape, odt), return_lse=True)
            assert err(o, ref, f"paged/{'fp8' if g.fp8 else 'bf16'}/{odt}/o page {kp.shape[1]} causal={causal}") < tol
            assert err(lse, lse_ref, f"paged/{'fp8' if g.fp8 else 'bf16'}/{odt}/lse page {kp.shape[1]} causal={causal}") < TOL_LSE
            assert ar.bit_equal(o, oc) and ar.bit_equal(lse, lsec), (odt, causal)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("permuted", [False, True], ids=["pages-page-H-d", "pages-H-page-d-view"])
@pytest.mark.parametrize("page", [128, 256, 2048])
def test_pages_larger_than_the_key_block(page, permuted, lib):
    """several 64-key blocks share one table entry; 2048: one page is larger than nk"""
    batch, H, group, nq, nk, lens = 2, 2, 2, 70, 1000, [1000, 613]
    g = Gauss(lib, 301, batch * H, group, nq, nk)
    kp, vp, table, _ = build_pool(g.kraw, g.vraw, batch, H, lens, page, g.fill, seed=page)
    paged_equals_contiguous(g, batch, H, lens, nk, kp, vp, table, permuted)


@pytest.mark.parametrize("lib", LIBS)
def test_several_causal_tiles_over_pages_of_16_under_a_shuffled_table(lib):
    batch, H, group, nq, nk, lens = 2, 1, 2, 512, 600, [600, 437]     # M = 1024: group = 2, per_head = 2; sequence 1: nq > len
    g = Gauss(lib, 311, batch * H, group, nq, nk)
    kp, vp, table, _ = build_pool(g.kraw, g.vraw, batch, H, lens, 16, g.fill, seed=5)
    paged_equals_contiguous(g, batch, H, lens, nk, kp, vp, table)


@pytest.mark.parametrize("lib", LIBS)
def test_prefix_sharing(lib):
    """Two sequences whose first 512 keys are the same physical pages, with different tails; sequence 1's own copies hold NaN."""
    batch, H, group, nq, nk, page, shared, lens = 2, 1, 4, 70, 1024, 64, 512, [700, 900]
    g = Gauss(lib, 321, batch, group, nq, nk)
    for name in ("kraw", "vraw", "k", "v"):
        a = np.array(getattr(g, name))           # a writable copy: the codes are shared between tests
        a[1, :shared] = a[0, :shared]
        setattr(g, name, a)
    kp, vp, table, _ = build_pool(g.kraw, g.vraw, batch, H, lens, page, g.fill, seed=3)
    own = table[1, :shared // page].copy()
    table[1, :shared // page] = table[0, :shared // page]
    kp[own], vp[own] = g.fill, g.fill              # pages nobody names
    paged_equals_contiguous(g, batch, H, lens, nk, kp, vp, table)


# ---- 5. a pool beyond 4 GiB --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_a_pool_beyond_four_gigabytes(lib):
    """The page base must be formed in 64 bits (the in-page offset is 32-bit: bytes for fp8, elements for bf16).  The pools are allocated and
    not filled; the four used pages lie on both sides of the 2^32-byte line."""
    page, group, nq, nk = 256, 4, 64, 1024
    g = Gauss(lib, 141, 1, group, nq, nk)
    es = 1 if g.fp8 else 2
    line = (1 << 32) // (page * D * es)            # the first page that starts at or beyond 2^32 bytes
    pages = line + 64
    assert pages * page * D * es > 1 << 32 and (line - 1) * page * D * es < 1 << 32 <= line * page * D * es
    kp = torch.empty((pages, page, D), dtype=F8 if g.fp8 else torch.bfloat16, device=dev())
    vp = torch.empty_like(kp)
    where = [line + 1, line - 1, pages - 1, line]
    for p, phys in enumerate(where):
        for pool, src in ((kp, g.kraw), (vp, g.vraw)):
            pool.view(torch.uint8 if g.fp8 else torch.bfloat16)[phys] = g.raw_bytes(src[0, p * page:(p + 1) * page])
    table = torch.tensor([where], dtype=torch.int32, device=dev())
    ref, lse_ref = attention_kv(g.q, g.k, g.v, None, False, 1.0)
    o, lse = g.prefill_paged(to_dev(g.q), kp, vp, table, out=poisoned(g.q.shape, torch.float32), return_lse=True)
    assert err(o, ref, f"pool beyond 2^32 bytes ({lib})") < TOL_PB2 and err(lse, lse_ref, f"pool beyond 2^32 bytes ({lib}), lse") < TOL_LSE
    del kp, vp
    torch.cuda.empty_cache()


# ---- 6. lengths outside [0, nk] ----------------------------------------------------------------------------------------------------------
CLAMP = [-5, 0, None, 1000]     # None: nk; 1000: nk + 1000


def _clamp_checks(g, o, lse, ref, lse_ref, group, tol, what):
    assert err(o, ref, f"{what} o") < tol and err(lse, lse_ref, f"{what} lse") < TOL_LSE
    assert not o[:2 * group].any() and bool((lse[:2 * group] == float("-inf")).all()), "a length of -5 or 0: exactly 0 / -inf"


@pytest.mark.parametrize("lib", LIBS)
def test_kv_lens_are_clamped_to_zero_and_nk(lib):
    """kv_lens = [-5, 0, nk, nk + 1000] from device memory: slabs 0 and 1 see nothing, slabs 2 and 3 are the reference at nk.  The capacity
    reaches beyond nk + 1000 and holds NaN from row nk on (slabs 0, 1: everywhere): a length taken as it stands reads NaN, inside the cache."""
    bh_kv, group, nq, nk = 4, 2, 40, 200
    lens = [nk if n is None else nk + n if n > 0 else n for n in CLAMP]
    eff = [0, 0, nk, nk]
    g = Gauss(lib, 331, bh_kv, group, nq, nk)
    qd, kd, vd = to_dev(g.q), g.cache(g.kraw, nk + 1024, eff), g.cache(g.vraw, nk + 1024, eff)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    for causal in (False, True):
        ref, lse_ref = attention_kv(g.q, g.k, g.v, eff, causal, 1.0)
        for odt, tol in BARS:
            o, lse = g.prefill(qd, kd, vd, causal, kv_len=nk, kv_lens=lens_d, out=poisoned(g.q.shape, odt), return_lse=True)
            _clamp_checks(g, o, lse, ref, lse_ref, group, tol, f"clamp/{lib}/{odt} causal={causal}")


@pytest.mark.parametrize("lib", LIBS)
def test_seq_lens_are_clamped_to_zero_and_nk(lib):
    """The same through seq_lens: the table is long enough for nk + 1000 keys, and its entries at or beyond ceil(nk / page) name a page of NaN."""
    batch, H, group, nq, nk, page = 4, 1, 2, 40, 200, 16
    lens = [nk if n is None else nk + n if n > 0 else n for n in CLAMP]
    eff = [0, 0, nk, nk]
    g = Gauss(lib, 341, batch, group, nq, nk)
    kp, vp, table, _ = build_pool(g.kraw, g.vraw, batch, H, eff, page, g.fill, seed=9, max_pages=-(-(nk + 1000) // page) + 2)
    qd, kpd, vpd, table_d = to_dev(g.q), g.raw_to_dev(kp), g.raw_to_dev(vp), torch.from_numpy(table).to(dev())
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    for causal in (False, True):
        ref, lse_ref = attention_kv(g.q, g.k, g.v, eff, causal, 1.0)
        for odt, tol in BARS:
            o, lse = g.prefill_paged(qd, kpd, vpd, table_d, causal, kv_len=nk, seq_lens=lens_d, out=poisoned(g.q.shape, odt), return_lse=True)
            _clamp_checks(g, o, lse, ref, lse_ref, group, tol, f"clamp paged/{lib}/{odt} causal={causal}")
