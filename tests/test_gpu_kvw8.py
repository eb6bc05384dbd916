"""GPU: sliding-window KV-cache attention over an fp8 (e4m3fn) cache (include/flashattn_amd_kvw8.h; fa.forward_kv_fp8 / fa.forward_paged_fp8 with
window_left).

Three kinds of claim, those of tests/test_gpu_kv8.py under the window of tests/test_gpu_kvw.py:
  bit identity   with v_scale a power of two the result IS v_scale x fa.forward_kv(..., window_left=w) on the cache dequantised to bf16 at
                 scale' = fp32(scale * k_scale), and the LSE for any v_scale; a window that hides nothing gives the bits of the unwindowed fp8
                 entries; an aligned window those of the sliced cache; the paged entry those of the contiguous one on the gathered bytes
  accuracy       against the fp64 reference tests/kvw_reference.attention_kvw on k_scale * deq(k8), v_scale * deq(v8), at the bars of
                 tests/test_gpu_kv.py (imported: 2e-4 fp32 output, 1e-4 LSE, 2.5e-2 bf16 output)
  bounds         the guard-band arena of tests/arena.py

Data are those of tests/test_gpu_kv8.py: N(0, 1) quantised at k_scale = 0.013, v_scale = 0.011, built on the CPU, crossing to the device as bytes,
with no NaN code among them.  Every cache byte the read contract excludes -- rows at or beyond len AND rows below lo_slab = max(0, len - nq -
window_left) -- is a NaN code, and every paged table entry outside [lo_slab // page, ceil(len / page)) names one page of NaN codes: a slid-out row
that reached the V image would meet a zero weight there and come out as NaN.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import flashattention_c_amd as fa
from flashattention_c_amd import _cabi_kv8, _cabi_kvw8
from tests import arena as ar
from tests.kv8_reference import dequant
from tests.kvw_reference import attention_kvw, lo_slab
from tests.paged_reference import gather
from tests.test_gpu_kv import TOL_BF16, TOL_LSE, TOL_PB2, dev, randn, to_dev
from tests.test_gpu_kv8 import F8, KS, VS, _arena, _poison_outputs, _surround, as_bf16, codes, folded, to_dev8, u8
from tests.test_gpu_kvw import BOUNDS, PARITY, err

pytestmark = pytest.mark.gpu

BF16, BF16_F32 = _cabi_kvw8.FA_DTYPE_BF16, _cabi_kvw8.FA_DTYPE_BF16_OUT_F32
NAN_CODE = 0xFF
IDS = dict(ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else None)


def window_cache8(a, capacity, lens, nq, w):
    """(bh, nk, d) codes -> fp8 device cache (bh, capacity, d) that holds rows [lo_slab, len) of every slab and a NaN code everywhere else"""
    t = np.full((a.shape[0], capacity, a.shape[2]), NAN_CODE, dtype=np.uint8)
    for s, n in enumerate(lens):
        lo = lo_slab(n, nq, w)
        t[s, lo:n] = a[s, lo:n]
    return to_dev8(t)


def fp8(qd, k8, v8, causal, vs=VS, **kw):
    return fa.forward_kv_fp8(qd, k8, v8, causal, k_scale=KS, v_scale=vs, **kw)


# ---- 1. bit identity with the 16-bit windowed kernel ----
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape,splits", PARITY, **IDS)
def test_bit_identity_with_the_windowed_bf16_kernel_on_the_dequantised_cache(shape, splits, causal):
    bh_kv, group, nq, nk, d, w = shape
    assert (_cabi_kvw8.lib().fa_kvw8_splits_for(bh_kv, group, nq, nk, d, int(causal), BF16, w) > 1) == splits
    qd = to_dev(randn(61, bh_kv * group, nq, d))
    lens = [nk] * bh_kv
    k8, v8 = window_cache8(codes(62, KS, bh_kv, nk, d), nk + 70, lens, nq, w), window_cache8(codes(63, VS, bh_kv, nk, d), nk + 70, lens, nq, w)
    kb, vb = as_bf16(k8), as_bf16(v8)   # converted on the CPU: the NaN rows stay NaN
    lo = lo_slab(nk, nq, w)
    assert bool(torch.isnan(kb[:, nk:].float()).all()) and bool(torch.isnan(vb[:, :lo].float()).all()) and not bool(torch.isnan(vb[:, lo:nk].float()).any())
    for scale in (1.0, 0.125):
        for odt in (torch.float32, torch.bfloat16):
            ref, lse_ref = fa.forward_kv(qd, kb, vb, causal, kv_len=nk, scale=folded(scale, KS), out_dtype=odt, return_lse=True, window_left=w)
            for vs in (1.0, 0.5, VS):
                o, lse = fp8(qd, k8, v8, causal, vs, kv_len=nk, scale=scale, out_dtype=odt, return_lse=True, window_left=w)
                assert o.dtype == odt
                assert ar.bit_equal(lse, lse_ref), f"LSE differs from the windowed bf16 kernel's (scale {scale}, {odt}, v_scale {vs})"
                if vs != VS:   # a power of two: the product is exact in fp32 and in bf16
                    diff = float((o.float() - vs * ref.float()).abs().max())
                    assert ar.bit_equal(o, (vs * ref).to(odt)), f"O differs from v_scale x the windowed bf16 kernel's (scale {scale}, {odt}, v_scale {vs}): {diff:.3e}"


# ---- 2. accuracy against the fp64 reference ----
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape,splits", PARITY, **IDS)
def test_general_scales_against_the_fp64_reference(shape, splits, causal):
    bh_kv, group, nq, nk, d, w = shape
    q, kc, vc = randn(61, bh_kv * group, nq, d), codes(62, KS, bh_kv, nk, d), codes(63, VS, bh_kv, nk, d)
    lens = [nk] * bh_kv
    qd, k8, v8 = to_dev(q), window_cache8(kc, nk + 70, lens, nq, w), window_cache8(vc, nk + 70, lens, nq, w)
    k, v = KS * dequant(kc), VS * dequant(vc)
    for scale in (1.0, 0.125):
        ref, lse_ref = attention_kvw(q, k, v, None, causal, scale, w)
        o, lse = fp8(qd, k8, v8, causal, kv_len=nk, scale=scale, out_dtype=torch.float32, return_lse=True, window_left=w)
        assert err(o, ref, f"{shape} f32 out scale {scale}") < TOL_PB2
        assert err(lse, lse_ref, f"{shape} lse scale {scale}") < TOL_LSE
        ob, lseb = fp8(qd, k8, v8, causal, kv_len=nk, scale=scale, return_lse=True, window_left=w)
        assert ob.dtype == torch.bfloat16
        assert err(ob, ref, f"{shape} bf16 out scale {scale}") < TOL_BF16
        assert err(lseb, lse_ref, f"{shape} lse (bf16 out) scale {scale}") < TOL_LSE
    if causal and nq > nk:   # rows i < nq - nk see nothing: exactly 0, LSE -inf (err() compares the infinite entries exactly)
        assert not ref[:, :nq - nk].any() and not o[:, :nq - nk].any() and not ob[:, :nq - nk].any()
        assert bool((lse[:, :nq - nk] == float("-inf")).all()) and bool((lseb[:, :nq - nk] == float("-inf")).all())


# ---- 3. ragged lengths ----
@pytest.mark.parametrize("causal", [False, True])
def test_ragged_lengths_from_device_memory(causal):
    bh_kv, group, nq, nk, d, w = 7, 4, 2, 2048, 128, 1000
    lens = [0, 1, 63, 64, 65, 777, 2048]
    assert _cabi_kvw8.lib().fa_kvw8_splits_for(bh_kv, group, nq, nk, d, int(causal), BF16, w) > 1
    q, kc, vc = randn(71, bh_kv * group, nq, d), codes(72, KS, bh_kv, nk, d), codes(73, VS, bh_kv, nk, d)
    k, v = KS * dequant(kc), VS * dequant(vc)
    qd, k8, v8 = to_dev(q), window_cache8(kc, nk, lens, nq, w), window_cache8(vc, nk, lens, nq, w)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    o, lse = fp8(qd, k8, v8, causal, kv_lens=lens_d, out_dtype=torch.float32, return_lse=True, window_left=w)
    ref, lse_ref = attention_kvw(q, k, v, lens, causal, 1.0, w)
    assert err(o, ref, "ragged f32 out") < TOL_PB2 and err(lse, lse_ref, "ragged lse") < TOL_LSE
    ob = fp8(qd, k8, v8, causal, kv_lens=lens_d, window_left=w)
    assert err(ob, ref, "ragged bf16 out") < TOL_BF16
    for s, n in enumerate(lens):   # each slab equals the reference at its own length, computed on its own
        sl = slice(s * group, (s + 1) * group)
        if n == 0:
            assert not o[sl].any() and bool((lse[sl] == float("-inf")).all())
            continue
        ref_s, lse_s = attention_kvw(q[sl], k[s:s + 1, :n], v[s:s + 1, :n], None, causal, 1.0, w)
        assert err(o[sl], ref_s, f"slab {s} alone") < TOL_PB2 and err(lse[sl], lse_s, f"slab {s} lse alone") < TOL_LSE


# ---- a paged fp8 cache under a window ----
def paged_window_cache8(kc, vc, batch, H, lens, page, nq, w, seed=0, spare=4):
    """kc, vc (batch * H, nk, d) codes -> the (pages, page, H, d) pools as bytes (numpy) and a shuffled block table.  A pool holds rows
    [lo_slab, len) of every sequence; every other byte is a NaN code, and every table entry outside [lo_slab // page, ceil(len / page)) names one
    valid page that is all NaN codes.  valid: the (page, row) pairs a call may read; free: pages no entry names."""
    nk, d = kc.shape[1], kc.shape[2]
    max_pages = -(-nk // page) + 2
    ranges = [(lo_slab(n, nq, w) // page, -(-n // page)) for n in lens]
    pages = sum(hi - lo for lo, hi in ranges) + spare
    order = [int(x) for x in np.random.default_rng(seed).permutation(pages)]
    nan_page = order.pop()
    table = np.full((batch, max_pages), nan_page, dtype=np.int32)
    kp, vp = (np.full((pages, page, H, d), NAN_CODE, dtype=np.uint8) for _ in range(2))
    valid = np.zeros((pages, page), dtype=bool)
    for b, (n, (plo, phi)) in enumerate(zip(lens, ranges)):
        lo = lo_slab(n, nq, w)
        for p in range(plo, phi):
            phys = order.pop()
            table[b, p] = phys
            r0, r1 = max(p * page, lo), min((p + 1) * page, n)
            valid[phys, r0 - p * page:r1 - p * page] = True
            for pool, src in ((kp, kc), (vp, vc)):
                pool[phys, r0 - p * page:r1 - p * page] = src[b * H:(b + 1) * H, r0:r1].transpose(1, 0, 2)
    return SimpleNamespace(canon=(kp, vp), table=table, valid=valid, nan_page=nan_page, free=order, pages=pages, max_pages=max_pages)


def upload(canon, layout):
    kd, vd = (u8(t) for t in canon)
    if layout == "hpd":
        kd, vd = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (kd, vd))
        assert not kd.is_contiguous()
    return kd.view(F8), vd.view(F8)


# ---- 4. no window, same bits ----
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", [(2, 4, 3, 300, 64), (2, 4, 3, 2048, 128)], ids=lambda s: "-".join(map(str, s)))
def test_a_window_that_hides_nothing_gives_the_bits_of_the_unwindowed_fp8_library(shape, causal):
    bh_kv, group, nq, nk, d = shape
    S = _cabi_kv8.lib().fa_kv8_splits_for(bh_kv, group, nq, nk, d, int(causal), BF16)
    assert (S > 1) == (nk >= 512)
    lens = [nk - 37, nk // 3]
    qd, kc, vc = to_dev(randn(131, bh_kv * group, nq, d)), codes(132, KS, bh_kv, nk, d), codes(133, VS, bh_kv, nk, d)
    k8, v8 = window_cache8(kc, nk, lens, nq, nk), window_cache8(vc, nk, lens, nq, nk)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    pc = paged_window_cache8(kc, vc, bh_kv, 1, lens, 16, nq, nk, seed=3)
    kp, vp = upload(pc.canon, "phd")
    table_d = torch.from_numpy(pc.table).to(dev())
    for odt in (torch.float32, torch.bfloat16):
        want = fp8(qd, k8, v8, causal, kv_lens=lens_d, out_dtype=odt, return_lse=True)
        wantp = fa.forward_paged_fp8(qd, kp, vp, table_d, causal, k_scale=KS, v_scale=VS, kv_len=nk, seq_lens=lens_d, out_dtype=odt, return_lse=True)
        assert ar.bit_equal(want[0], wantp[0]) and ar.bit_equal(want[1], wantp[1])
        assert not bool(torch.isnan(want[0].float()).any())
        for w in (nk - 1, 1 << 24):
            assert _cabi_kvw8.lib().fa_kvw8_splits_for(bh_kv, group, nq, nk, d, int(causal), BF16, w) == S
            got = fp8(qd, k8, v8, causal, kv_lens=lens_d, out_dtype=odt, return_lse=True, window_left=w)
            assert ar.bit_equal(got[0], want[0]) and ar.bit_equal(got[1], want[1]), (odt, w)
            gotp = fa.forward_paged_fp8(qd, kp, vp, table_d, causal, k_scale=KS, v_scale=VS, kv_len=nk, seq_lens=lens_d, out_dtype=odt, return_lse=True,
                                        window_left=w)
            assert ar.bit_equal(gotp[0], want[0]) and ar.bit_equal(gotp[1], want[1]), (odt, w, "paged")


# ---- 5. an aligned window, the bits of the slice ----
@pytest.mark.parametrize("d", [64, 128])
def test_an_aligned_window_gives_the_bits_of_the_sliced_cache(d):
    """Blocks start at lo & ~63: with lo a multiple of 64 the windowed call walks the blocks a call on rows [lo, len) walks."""
    bh_kv, group, nq, nk, w = 2, 4, 1, 1024, 255
    lens = [448, 960]
    assert all(lo_slab(n, nq, w) % 64 == 0 and lo_slab(n, nq, w) == n - 256 for n in lens)
    assert _cabi_kvw8.lib().fa_kvw8_splits_for(bh_kv, group, nq, nk, d, 1, BF16_F32, w) == 1
    assert _cabi_kv8.lib().fa_kv8_splits_for(1, group, nq, 256, d, 1, BF16_F32) == 1
    qd, kc, vc = to_dev(randn(141, bh_kv * group, nq, d)), codes(142, KS, bh_kv, nk, d), codes(143, VS, bh_kv, nk, d)
    k8, v8 = window_cache8(kc, nk, lens, nq, w), window_cache8(vc, nk, lens, nq, w)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    for causal in (True, False):
        o, lse = fp8(qd, k8, v8, causal, kv_lens=lens_d, out_dtype=torch.float32, return_lse=True, window_left=w)
        for s, n in enumerate(lens):
            sl = slice(s * group, (s + 1) * group)
            ks, vs = to_dev8(kc[s:s + 1, n - 256:n]), to_dev8(vc[s:s + 1, n - 256:n])
            os_, lses = fp8(qd[sl], ks, vs, causal, kv_len=256, out_dtype=torch.float32, return_lse=True)
            assert ar.bit_equal(o[sl], os_) and ar.bit_equal(lse[sl], lses), (causal, s)


# ---- 6. paged equals contiguous on the gathered bytes ----
@pytest.mark.parametrize("layout", ["phd", "hpd"])
@pytest.mark.parametrize("page", [16, 64, 256])
@pytest.mark.parametrize("shape", [(2, 2, 2, 3, 1000, 64, 100, [1000, 613]), (1, 2, 4, 2, 2048, 128, 1000, [1999])], ids=lambda s: "-".join(map(str, s[:7])))
def test_paged_equals_contiguous_on_the_gathered_bytes(shape, page, layout):
    batch, H, group, nq, nk, d, w, lens = shape
    L = _cabi_kvw8.lib()
    S = L.fa_kvw8_paged_splits_for(batch, H, group, nq, nk, d, 1, BF16, w)
    assert S == L.fa_kvw8_splits_for(batch * H, group, nq, nk, d, 1, BF16, w) and (S > 1) == (w >= 512)
    bh_kv = batch * H
    slab_lens = [n for n in lens for _ in range(H)]
    q, kc, vc = randn(151, bh_kv * group, nq, d), codes(152, KS, bh_kv, nk, d), codes(153, VS, bh_kv, nk, d)
    k, v = KS * dequant(kc), VS * dequant(vc)
    qd = to_dev(q)
    pc = paged_window_cache8(kc, vc, batch, H, lens, page, nq, w, seed=page)
    kp, vp = upload(pc.canon, layout)
    for b, n in enumerate(lens):   # what the contract lets the call read, and nothing else, is a page of data
        plo, phi = lo_slab(n, nq, w) // page, -(-n // page)
        assert (pc.table[b, :plo] == pc.nan_page).all() and (pc.table[b, phi:] == pc.nan_page).all() and (pc.table[b, plo:phi] != pc.nan_page).all()
    assert (pc.canon[0][pc.nan_page] == NAN_CODE).all() and (pc.canon[1][pc.nan_page] == NAN_CODE).all()
    gk, gv = gather(pc.canon[0], pc.table, lens, nk).copy(), gather(pc.canon[1], pc.table, lens, nk).copy()   # NaN codes below lo_slab (of data pages too)
    for s, n in enumerate(slab_lens):
        lo = lo_slab(n, nq, w)
        assert (gk[s, :lo] == NAN_CODE).all() and np.array_equal(gk[s, lo:n], kc[s, lo:n]) and np.array_equal(gv[s, lo:n], vc[s, lo:n])
        gk[s, n:], gv[s, n:] = NAN_CODE, NAN_CODE
    kd, vd = to_dev8(gk), to_dev8(gv)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    slab_lens_d = torch.tensor(slab_lens, dtype=torch.int32, device=dev())
    table_d = torch.from_numpy(pc.table).to(dev())
    for causal in (False, True):
        ref, lse_ref = attention_kvw(q, k, v, slab_lens, causal, 1.0, w)
        for odt in (torch.float32, torch.bfloat16):
            o, lse = fa.forward_paged_fp8(qd, kp, vp, table_d, causal, k_scale=KS, v_scale=VS, kv_len=nk, seq_lens=lens_d, out_dtype=odt, return_lse=True,
                                          window_left=w)
            oc, lsec = fp8(qd, kd, vd, causal, kv_len=nk, kv_lens=slab_lens_d, out_dtype=odt, return_lse=True, window_left=w)
            assert err(o, ref, f"paged {odt} causal={causal}") < (TOL_PB2 if odt == torch.float32 else TOL_BF16) and err(lse, lse_ref, "paged lse") < TOL_LSE
            assert ar.bit_equal(o, oc) and ar.bit_equal(lse, lsec), f"paged and contiguous differ ({odt}, causal={causal}): " \
                f"{float((o.float() - oc.float()).abs().max()):.3e}"


# ---- 7. one captured graph, a window that slides ----
def test_one_captured_graph_follows_a_sliding_window():
    batch, group, nq, cap, d, page, w = 2, 4, 1, 512, 128, 16, 199
    q, kc, vc = randn(161, batch * group, nq, d), codes(162, KS, batch, cap, d), codes(163, VS, batch, cap, d)
    k, v = KS * dequant(kc), VS * dequant(vc)
    qd = to_dev(q)
    max_pages = cap // page
    pages = batch * max_pages + 1
    order = [int(x) for x in np.random.default_rng(9).permutation(pages)]
    nan_page = order.pop()
    table_h = np.array(order, dtype=np.int32).reshape(batch, max_pages)
    kp = torch.full((pages, page, d), NAN_CODE, dtype=torch.uint8, device=dev())   # the pools as bytes; the entry sees them as fp8
    vp = torch.full_like(kp, NAN_CODE)
    kdev, vdev = u8(kc), u8(vc)
    for b in range(batch):
        for p in range(max_pages):
            kp[int(table_h[b, p])], vp[int(table_h[b, p])] = kdev[b, p * page:(p + 1) * page], vdev[b, p * page:(p + 1) * page]
    table = torch.from_numpy(table_h).to(dev())
    lens_d = torch.zeros(batch, dtype=torch.int32, device=dev())
    out = torch.empty(batch * group, nq, d, dtype=torch.float32, device=dev())
    eager = torch.empty_like(out)
    assert fa.workspace_bytes_paged(batch, 1, group, nq, cap, d, True, out_dtype=torch.float32, window_left=w) == 0   # 263 keys: never split
    kw = dict(k_scale=KS, v_scale=VS, seq_lens=lens_d, window_left=w)
    fa.forward_paged_fp8(qd, kp.view(F8), vp.view(F8), table, True, out=out, **kw)   # library loaded, allocator warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, lse = fa.forward_paged_fp8(qd, kp.view(F8), vp.view(F8), table, True, out=out, return_lse=True, **kw)
    crossed_blocks, crossed_pages = set(), set()
    for n in range(250, 331):
        lens = [n, n - 13]
        for b, m in enumerate(lens):   # what has slid out of the window is gone: rows below the edge are NaN codes, entries below its page name the NaN page
            lo = lo_slab(m, nq, w)
            for p in range(lo // page):
                table[b, p] = nan_page
            p = lo // page
            kp[int(table_h[b, p]), :lo - p * page] = NAN_CODE
            vp[int(table_h[b, p]), :lo - p * page] = NAN_CODE
            if p:
                kp[[int(x) for x in table_h[b, :p]]] = NAN_CODE
                vp[[int(x) for x in table_h[b, :p]]] = NAN_CODE
            crossed_blocks.add((b, lo // 64))
            crossed_pages.add((b, lo // page))
        lens_d.copy_(torch.tensor(lens, dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        _, lse_e = fa.forward_paged_fp8(qd, kp.view(F8), vp.view(F8), table, True, out=eager, return_lse=True, **kw)
        assert ar.bit_equal(out, eager) and ar.bit_equal(lse, lse_e), f"replay and eager call differ at lengths {lens}"
        if n % 16 == 10 or n == 330:
            ref, lse_ref = attention_kvw(q, k, v, lens, True, 1.0, w)
            assert err(out, ref, f"replay at lengths {lens}") < TOL_PB2 and err(lse, lse_ref, f"replay lse at lengths {lens}") < TOL_LSE
    assert len({c for b, c in crossed_blocks if b == 0}) >= 2 and len({c for b, c in crossed_pages if b == 0}) >= 4


# ---- 8. bounds: everything in one guard-band arena at the minimum alignments ----
RUNS = (("zero", 0), ("nan", 0), ("finite", 7))


def _fill8(t, mode, seed):
    """every byte of an fp8 view: zeros, NaN codes, or finite codes from a seed"""
    if mode == "zero":
        t.view(torch.uint8).zero_()
    else:
        _surround(t, mode, seed)


def _check_run(A, runs, ref, lse_ref, out_f32, mode):
    torch.cuda.synchronize()
    assert A.guards_intact(), str(A.first_damage())   # stores only to o, lse and the workspace
    runs.append((A.view("o").clone(), A.view("lse").clone()))
    assert err(runs[-1][0], ref, f"o, {mode} surroundings") < (TOL_PB2 if out_f32 else TOL_BF16)
    assert err(runs[-1][1], lse_ref, f"lse, {mode} surroundings") < TOL_LSE


@pytest.mark.parametrize("out_f32", [True, False])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", BOUNDS, ids=lambda c: "-".join(map(str, c[:6])))
def test_memory_bounds_and_isolation(case, causal, out_f32):
    bh_kv, group, nq, nk, d, w, lens = case
    L = _cabi_kvw8.lib()
    dt = BF16_F32 if out_f32 else BF16
    cap, bhq = nk + 70, bh_kv * group
    S = L.fa_kvw8_splits_for(bh_kv, group, nq, nk, d, int(causal), dt, w)
    assert (S > 1) == (w >= 512)
    ws = int(L.fa_kvw8_workspace_bytes(bh_kv, group, nq, nk, d, int(causal), dt, w))
    assert (ws > 0) == (S > 1)
    A = _arena(bhq, nq, d, (bh_kv + 1, cap, d), out_f32, ws)   # one K/V slab more than the call covers: the cache of a neighbouring call
    q, kc, vc = randn(91, bhq, nq, d), codes(92, KS, bh_kv, nk, d), codes(93, VS, bh_kv, nk, d)
    A.view("q").copy_(to_dev(q))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    ref, lse_ref = attention_kvw(q, KS * dequant(kc), VS * dequant(vc), lens, causal, 1.0, w)
    assert np.isfinite(lse_ref).all()   # every row sees a key: the three runs below must be finite
    runs = []
    for mode, seed in RUNS:
        A.fill_input_surroundings("nan" if mode == "zero" else mode, seed)
        for name, src in (("k", kc), ("v", vc)):
            t = A.view(name)
            _fill8(t, mode, seed + 1)                 # rows below lo_slab, rows [len, capacity) of every slab and the neighbour's slab ...
            for s, n in enumerate(lens):
                lo = lo_slab(n, nq, w)
                t.view(torch.uint8)[s, lo:n] = u8(src[s, lo:n])   # ... around the rows the call may read
        _poison_outputs(A, ws)
        rc = L.fa_kvw8_forward(A.ptr("q"), A.ptr("k"), A.ptr("v"), A.ptr("o"), A.ptr("lse"), bh_kv, group, nq, nk, cap, lens_d.data_ptr(), d, 1.0, KS, VS,
                               int(causal), dt, w, A.ptr("workspace") if ws else None, ws, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.fa_kvw8_last_error()
        _check_run(A, runs, ref, lse_ref, out_f32, mode)
    bad = ar.isolation_failures(*runs)
    assert not bad, "the result depends on memory the call must not read: " + "; ".join(bad)


# (batch, H, group, nq, nk, d, page, window_left, seq_lens): S = 2, M = 6; sequence 1 leaves whole shares empty, and its window starts inside a page
PAGED_BOUNDS = [(2, 2, 2, 3, 1500, 128, 16, 600, [1500, 333])]


@pytest.mark.parametrize("causal,out_f32", [(False, True), (True, False)])
@pytest.mark.parametrize("case", PAGED_BOUNDS, ids=lambda c: "-".join(map(str, c[:8])))
def test_memory_bounds_and_isolation_paged(case, causal, out_f32):
    batch, H, group, nq, nk, d, page, w, lens = case
    L = _cabi_kvw8.lib()
    dt = BF16_F32 if out_f32 else BF16
    bh_kv, bhq = batch * H, batch * H * group
    S = L.fa_kvw8_paged_splits_for(batch, H, group, nq, nk, d, int(causal), dt, w)
    ws = int(L.fa_kvw8_paged_workspace_bytes(batch, H, group, nq, nk, d, int(causal), dt, w))
    assert S > 1 and ws > 0 and any(lo_slab(n, nq, w) % page for n in lens)
    q, kc, vc = randn(91, bhq, nq, d), codes(92, KS, bh_kv, nk, d), codes(93, VS, bh_kv, nk, d)
    pc = paged_window_cache8(kc, vc, batch, H, lens, page, nq, w, seed=11, spare=7)
    P = pc.pages
    A = _arena(bhq, nq, d, (P, page, H, d), out_f32, ws)
    A.view("q").copy_(to_dev(q))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    ref, lse_ref = attention_kvw(q, KS * dequant(kc), VS * dequant(vc), [n for n in lens for _ in range(H)], causal, 1.0, w)
    assert np.isfinite(lse_ref).all()
    valid = torch.from_numpy(pc.valid).to(dev())                         # what the call may read: the same rows in both pools
    data = [u8(t) for t in pc.canon]
    runs = []
    for i, (mode, seed) in enumerate(RUNS):
        A.fill_input_surroundings("nan" if mode == "zero" else mode, seed)
        for name, pool in (("k", data[0]), ("v", data[1])):
            t = A.view(name)
            _fill8(t, mode, seed + 1)                                    # unused pages, slid-out rows and the tails of last pages ...
            t.view(torch.uint8)[valid] = pool[valid]                     # ... around the rows the call may read
        table = pc.table.copy()
        for b, n in enumerate(lens):                                     # entries outside the readable range: another page that exists, per run
            other = pc.free[(b + i) % len(pc.free)]
            table[b, :lo_slab(n, nq, w) // page] = other
            table[b, -(-n // page):] = other
        table_d = torch.from_numpy(table).to(dev())
        _poison_outputs(A, ws)
        cache = _cabi_kvw8.FaPagedCache(A.ptr("k"), A.ptr("v"), P, page, page * H * d, H * d, d, table_d.data_ptr(), table.shape[1], lens_d.data_ptr())
        rc = L.fa_kvw8_paged_forward(A.ptr("q"), ctypes.byref(cache), A.ptr("o"), A.ptr("lse"), batch, H, group, nq, nk, d, 1.0, KS, VS, int(causal), dt, w,
                                     A.ptr("workspace"), ws, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.fa_kvw8_last_error()
        _check_run(A, runs, ref, lse_ref, out_f32, mode)
    bad = ar.isolation_failures(*runs)
    assert not bad, "the result depends on memory the call must not read: " + "; ".join(bad)


# ---- 9. the Python keyword ----
def test_a_negative_window_is_rejected_before_anything_runs():
    q = torch.zeros(1, 1, 64, dtype=torch.bfloat16, device=dev())
    k8 = torch.zeros(1, 16, 64, dtype=torch.uint8, device=dev()).view(F8)
    table = torch.zeros(1, 1, dtype=torch.int32, device=dev())
    with pytest.raises(ValueError, match="window_left = -1"):
        fa.forward_kv_fp8(q, k8, k8, True, window_left=-1)
    with pytest.raises(ValueError, match="window_left = -1"):
        fa.forward_paged_fp8(q, k8, k8, table, True, window_left=-1)
    for bad in (True, 1.0, "3"):
        with pytest.raises(TypeError, match="window_left"):
            fa.forward_kv_fp8(q, k8, k8, True, window_left=bad)
        with pytest.raises(TypeError, match="window_left"):
            fa.forward_paged_fp8(q, k8, k8, table, True, window_left=bad)
    # None is the unwindowed library, an int the windowed one: both run, and a window wider than the cache changes no bit
    o = fa.forward_kv_fp8(q, k8, k8, True)
    assert ar.bit_equal(o, fa.forward_kv_fp8(q, k8, k8, True, window_left=1 << 30)) and not o.any()
