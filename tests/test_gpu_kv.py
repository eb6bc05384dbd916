"""GPU: the KV-cache attention extension (include/flashattn_amd_kv.h, fa.forward_kv) against the fp64 reference tests/kv_reference.py.

Tolerances are those of tests/test_gpu_parity.py::test_pb2_kernel_vs_oracle, on its data family (seeded N(0, 1) rounded to bf16, scale 1.0
and 0.125): the arithmetic is the same (one bf16 product for Q.K^T, P as bf16 hi + bf16 lo, fp32 accumulators):
    fp32 output  TOL_PB2 = 2e-4      LSE  1e-4      bf16 output  2.5e-2 (its own rounding of values up to ~4 on this data)
"""
import ctypes

import numpy as np
import pytest
import torch

import flashattention_c_amd as fa
from flashattention_c_amd import _cabi_kv
from oracle import oracle as orc
from tests import arena as ar
from tests.kv_reference import attention_kv

pytestmark = pytest.mark.gpu

TOL_PB2, TOL_LSE, TOL_BF16 = 2e-4, 1e-4, 2.5e-2
BF16, BF16_F32 = _cabi_kv.FA_DTYPE_BF16, _cabi_kv.FA_DTYPE_BF16_OUT_F32


def dev():
    return torch.device("cuda", 0)


def randn(seed, *shape):
    return orc.round_to_bf16(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).numpy())


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(dev())


def cache(a, capacity):
    """(bh, nk, d) array -> bf16 device cache (bh, capacity, d) whose rows past nk are NaN: nothing may read them."""
    t = torch.full((a.shape[0], capacity, a.shape[2]), float("nan"), dtype=torch.bfloat16, device=dev())
    t[:, :a.shape[1]] = to_dev(a)
    return t


def err(t, ref, what):
    got = t.detach().float().cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any(), f"NaN in {what}"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), f"{what}: -inf entries differ"
    e = float(np.abs(got[~inf] - ref[~inf]).max()) if (~inf).any() else 0.0
    print(f"{what}: max abs err {e:.3e}")
    return e


def check_all(q, k, v, qd, kd, vd, nk, causal, lens=None, lens_d=None, what=""):
    """both scales, both output dtypes, output and LSE"""
    for scale in (1.0, 0.125):
        ref, lse_ref = attention_kv(q, k, v, lens, causal, scale)
        o, lse = fa.forward_kv(qd, kd, vd, causal, kv_len=nk, kv_lens=lens_d, scale=scale, out_dtype=torch.float32, return_lse=True)
        assert err(o, ref, f"{what} f32 out scale {scale}") < TOL_PB2
        assert err(lse, lse_ref, f"{what} lse scale {scale}") < TOL_LSE
        ob, lseb = fa.forward_kv(qd, kd, vd, causal, kv_len=nk, kv_lens=lens_d, scale=scale, return_lse=True)
        assert ob.dtype == torch.bfloat16
        assert err(ob, ref, f"{what} bf16 out scale {scale}") < TOL_BF16
        assert err(lseb, lse_ref, f"{what} lse (bf16 out) scale {scale}") < TOL_LSE
    return ref


# (bh_kv, group, nq, nk, d), does the plan split?
PARITY = [
    ((2, 1, 1, 1, 64), False), ((3, 4, 1, 31, 64), False), ((2, 8, 1, 257, 128), False),                 # base
    ((2, 4, 5, 1000, 64), True),          # GQA, odd nq: packed rows straddle heads
    ((1, 8, 16, 4099, 128), True),        # GQA, S > 1 with a ragged last share
    ((1, 4, 33, 700, 64), True),          # M = 132: several row tiles
    ((2, 1, 40, 24, 128), False),         # causal with nq > nk: rows without keys
    ((5, 2, 2, 64, 64), False), ((130, 1, 1, 300, 128), False),                                        # many slabs, unsplit
]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape,splits", PARITY, ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else None)
def test_parity_against_the_fp64_reference(shape, splits, causal):
    bh_kv, group, nq, nk, d = shape
    S = _cabi_kv.lib().fa_kv_splits_for(bh_kv, group, nq, nk, d, int(causal), BF16)
    assert (S > 1) == splits and 1 <= S <= 64, S
    q, k, v = randn(61, bh_kv * group, nq, d), randn(62, bh_kv, nk, d), randn(63, bh_kv, nk, d)
    ref = check_all(q, k, v, to_dev(q), cache(k, nk + 70), cache(v, nk + 70), nk, causal, what=str(shape))
    if causal and nq > nk:   # rows i < nq - nk see nothing: exactly 0 (checked bit for bit), LSE -inf (checked in err())
        assert not ref[:, :nq - nk].any()
        o = fa.forward_kv(to_dev(q), cache(k, nk + 70), cache(v, nk + 70), True, kv_len=nk, out_dtype=torch.float32)
        assert not o[:, :nq - nk].any()


@pytest.mark.parametrize("causal", [False, True])
def test_ragged_lengths_from_device_memory(causal):
    bh_kv, group, nq, nk, d = 4, 4, 2, 2048, 128
    lens = [0, 1, 777, 2048]
    assert _cabi_kv.lib().fa_kv_splits_for(bh_kv, group, nq, nk, d, int(causal), BF16) > 1
    q, k, v = randn(71, bh_kv * group, nq, d), randn(72, bh_kv, nk, d), randn(73, bh_kv, nk, d)
    qd, kd, vd = to_dev(q), to_dev(k), to_dev(v)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    check_all(q, k, v, qd, kd, vd, nk, causal, lens, lens_d, "ragged")
    # each slab equals the reference at its own length, computed on its own
    o, lse = fa.forward_kv(qd, kd, vd, causal, kv_lens=lens_d, out_dtype=torch.float32, return_lse=True)
    for s, n in enumerate(lens):
        sl = slice(s * group, (s + 1) * group)
        if n == 0:
            assert not o[sl].any() and bool((lse[sl] == float("-inf")).all())
            continue
        ref, lse_ref = attention_kv(q[sl], k[s:s + 1, :n], v[s:s + 1, :n], None, causal, 1.0)
        assert err(o[sl], ref, f"slab {s} alone") < TOL_PB2 and err(lse[sl], lse_ref, f"slab {s} lse alone") < TOL_LSE


@pytest.mark.parametrize("causal", [True, False])
def test_agreement_with_the_square_product_kernel(causal):
    """The only route before this extension: pad Q to nk rows, run the square kernel, keep the last nq rows."""
    bh, nq, nk, d = 2, 8, 1536, 64
    q, k, v = randn(81, bh, nq, d), randn(82, bh, nk, d), randn(83, bh, nk, d)
    qd, kd, vd = to_dev(q), to_dev(k), to_dev(v)
    qp = torch.zeros(bh, nk, d, dtype=torch.bfloat16, device=dev())
    qp[:, -nq:] = qd
    sq = fa.forward(qp, kd, vd, causal, out_dtype=torch.float32)[:, -nq:]
    o = fa.forward_kv(qd, kd, vd, causal, out_dtype=torch.float32)
    e = float((o - sq).abs().max())
    print(f"forward_kv vs padded square forward, causal={causal}: {e:.3e}")
    assert e < 2 * TOL_PB2


# ---- bounds: everything in one guard-band arena at the minimum alignments ------------------------------------------------------------
def _fill(t, mode, seed):
    if mode == "nan":
        ar.fill_bytes(t, ar.POISON)
    else:
        t.copy_(torch.randn(t.shape, device=t.device, generator=torch.Generator(device=t.device).manual_seed(seed)).to(t.dtype))


BOUNDS = [
    # (bh_kv, group, nq, nk, d, kv_lens): S = 1, M = 20 (not a multiple of the 32-row tile)
    (3, 4, 5, 300, 64, [300, 17, 0]),
    # S = 4, M = 45: two row tiles, the second ragged; slab 1 leaves whole shares empty (their partial O is never written)
    (2, 5, 9, 1100, 128, [1100, 333]),
    (2, 5, 9, 1100, 128, None),
]


@pytest.mark.parametrize("out_f32", [True, False])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", BOUNDS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}-{'lens' if c[5] else 'full'}")
def test_memory_bounds_and_isolation(case, causal, out_f32):
    bh_kv, group, nq, nk, d, lens = case
    L = _cabi_kv.lib()
    dt = BF16_F32 if out_f32 else BF16
    cap, bhq = nk + 70, bh_kv * group
    S = L.fa_kv_splits_for(bh_kv, group, nq, nk, d, int(causal), dt)
    assert (S > 1) == (nk >= 512)
    ws = int(L.fa_kv_workspace_bytes(bh_kv, group, nq, nk, d, int(causal), dt))
    odt = torch.float32 if out_f32 else torch.bfloat16
    bufs = [ar.Buf("q", "in", torch.bfloat16, (bhq, nq, d), "tensor", d * 2),
            # one K/V slab more than the call covers: the cache of a neighbouring call
            ar.Buf("k", "in", torch.bfloat16, (bh_kv + 1, cap, d), "tensor", d * 2), ar.Buf("v", "in", torch.bfloat16, (bh_kv + 1, cap, d), "tensor", d * 2),
            ar.Buf("o", "out", odt, (bhq, nq, d), "tensor", d * (4 if out_f32 else 2)), ar.Buf("lse", "out", torch.float32, (bhq, nq), "lse", 4)]
    if ws:
        bufs.append(ar.Buf("workspace", "out", torch.uint8, (ws,), "workspace", d * 4))
    A = ar.Arena(bufs, dev())
    q, k, v = randn(91, bhq, nq, d), randn(92, bh_kv, nk, d), randn(93, bh_kv, nk, d)
    A.view("q").copy_(to_dev(q))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev()) if lens else None
    eff = lens if lens else [nk] * bh_kv
    ref, lse_ref = attention_kv(q, k, v, lens, causal, 1.0)
    runs = []
    for mode, seed in (("nan", 0), ("finite", 7)):
        A.fill_input_surroundings(mode, seed)
        for name, src in (("k", k), ("v", v)):
            t = A.view(name)
            _fill(t, mode, seed + 1)             # rows [len, capacity) of every slab and the neighbour's slab ...
            for s, n in enumerate(eff):
                t[s, :n] = to_dev(src[s, :n])    # ... around the rows the call may read
        A.fill_output_guards()
        ar.fill_bytes(A.view("o"), ar.POISON)
        ar.fill_bytes(A.view("lse"), ar.POISON)
        if ws:
            ar.fill_bytes(A.view("workspace"), ar.POISON)   # the kernels must read nothing of it they did not write
        rc = L.fa_kv_forward(A.ptr("q"), A.ptr("k"), A.ptr("v"), A.ptr("o"), A.ptr("lse"), bh_kv, group, nq, nk, cap,
                             lens_d.data_ptr() if lens else None, d, 1.0, int(causal), dt, A.ptr("workspace") if ws else None, ws,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.fa_kv_last_error()
        torch.cuda.synchronize()
        assert A.guards_intact(), str(A.first_damage())
        runs.append((A.view("o").clone(), A.view("lse").clone()))
        assert err(runs[-1][0], ref, f"o, {mode} surroundings") < (TOL_PB2 if out_f32 else TOL_BF16)
        assert err(runs[-1][1], lse_ref, f"lse, {mode} surroundings") < TOL_LSE
    assert ar.bit_equal(runs[0][0], runs[1][0]) and ar.bit_equal(runs[0][1], runs[1][1]), "the result depends on memory the call must not read"


def test_one_captured_graph_follows_a_growing_cache():
    bh_kv, group, nq, cap, d = 2, 4, 1, 1024, 128
    assert _cabi_kv.lib().fa_kv_splits_for(bh_kv, group, nq, cap, d, 1, BF16_F32) > 1
    q, k, v = randn(101, bh_kv * group, nq, d), randn(102, bh_kv, cap, d), randn(103, bh_kv, cap, d)
    qd = to_dev(q)
    kd = torch.full((bh_kv, cap, d), float("nan"), dtype=torch.bfloat16, device=dev())
    vd = torch.full_like(kd, float("nan"))
    lens_d = torch.zeros(bh_kv, dtype=torch.int32, device=dev())
    out = torch.empty(bh_kv * group, nq, d, dtype=torch.float32, device=dev())
    ws = torch.empty(fa.workspace_bytes_kv(bh_kv, group, nq, cap, d, True, out_dtype=torch.float32), dtype=torch.uint8, device=dev())
    assert ws.numel() > 0
    fa.forward_kv(qd, kd, vd, True, kv_lens=lens_d, out=out, workspace=ws)   # library loaded, allocator warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, lse = fa.forward_kv(qd, kd, vd, True, kv_lens=lens_d, out=out, workspace=ws, return_lse=True)
    have = [0, 0]
    for lens in ([100, 300], [101, 640], [1024, 641]):
        for s, n in enumerate(lens):   # the new rows enter the cache, the lengths follow
            kd[s, have[s]:n] = to_dev(k[s, have[s]:n])
            vd[s, have[s]:n] = to_dev(v[s, have[s]:n])
        have = lens
        lens_d.copy_(torch.tensor(lens, dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        ref, lse_ref = attention_kv(q, k, v, lens, True, 1.0)
        assert err(out, ref, f"replay at lengths {lens}") < TOL_PB2 and err(lse, lse_ref, f"replay lse at lengths {lens}") < TOL_LSE


@pytest.mark.parametrize("where", ["first share", "last share"])
def test_a_key_far_above_the_rest_and_a_constant_v(where):
    """One score 2^20 above the others (in the first / the last key share): its weight is 1 to fp64 precision, every other share's partial is
    scaled by exp(-2^20) = 0 in the combine.  O: the usual bar.  LSE is ~2^20 there, so its bar is relative: 2^-20 covers the fp32 roundings of the
    log-sum-exp (m * ln 2 and the sum, 2^-23 each) with margin.  V = 1 everywhere gives O = 1 exactly, for both output dtypes."""
    bh_kv, group, nq, nk, d = 1, 8, 1, 8192, 128
    assert _cabi_kv.lib().fa_kv_splits_for(bh_kv, group, nq, nk, d, 0, BF16) >= 16
    q, k, v = randn(111, group, nq, d), randn(112, bh_kv, nk, d), randn(113, bh_kv, nk, d)
    q[:] = 0.0
    q[:, :, 0] = 1024.0
    j = 100 if where == "first share" else nk - 3
    k[0, :, 0] = 0.0
    k[0, j, 0] = 1024.0          # score 2^20 for key j, |score| <= 0 + noise of the other columns (q is zero there) for the rest
    qd, kd, vd = to_dev(q), to_dev(k), to_dev(v)
    ref, lse_ref = attention_kv(q, k, v, None, False, 1.0)
    o, lse = fa.forward_kv(qd, kd, vd, out_dtype=torch.float32, return_lse=True)
    assert err(o, ref, f"spike in the {where}") < TOL_PB2
    rel = float(np.abs(lse.cpu().numpy().astype(np.float64) / lse_ref - 1.0).max())
    print(f"spike in the {where}: lse rel err {rel:.3e}")
    assert rel < 2.0 ** -20
    ones = torch.ones_like(vd)
    for odt in (torch.float32, torch.bfloat16):
        for qq in (qd, to_dev(randn(114, group, nq, d))):
            o1 = fa.forward_kv(qq, kd, ones, out_dtype=odt)
            assert bool((o1 == 1.0).all()), f"V = 1 must give O = 1 exactly ({odt})"
