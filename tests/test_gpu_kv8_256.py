"""GPU: KV-cache attention at head dim 256 over an fp8 (e4m3fn) cache (include/flashattn_amd_kv8_256.h; fa.forward_kv_fp8 / fa.forward_paged_fp8
with d = 256).  Two kinds of claim, as in tests/test_gpu_kv8.py:
  bit identity   with v_scale a power of two the result IS v_scale x fa.forward_kv (d = 256) on the dequantised cache at scale' = fp32(scale * k_scale)
                 with the same window_left; the LSE for any v_scale; the paged entry IS the contiguous one on the gathered bytes
  accuracy       against the fp64 references on the logical values k_scale * deq(k8), v_scale * deq(v8), at the bars of tests/test_gpu_kv256.py
                 (2e-4 fp32 output, 1e-4 LSE, 2.5e-2 bf16 output): the arithmetic is that kernel's and the logical values are N(0, 1)-sized
Data as in tests/test_gpu_kv8.py (k_scale = 0.013, v_scale = 0.011, bytes built on the CPU).  Every row the read contract excludes -- at or
beyond len, below lo_slab = max(0, len - nq - window_left) -- holds the NaN code 0xFF.
"""
import pytest
import torch

import flashattention_c_amd as fa
from flashattention_c_amd import _cabi_kv8_256
from tests import arena as ar
from tests.kv8_reference import dequant
from tests.kvw_reference import attention_kvw, lo_slab
from tests.test_gpu_kv8 import F8, KS, VS, Cache8, as_bf16, codes, folded, u8
from tests.test_gpu_kv256 import D, PARITY, TOL_BF16, TOL_LSE, TOL_PB2, dev, err, randn, to_dev

pytestmark = pytest.mark.gpu

BF16 = _cabi_kv8_256.FA_DTYPE_BF16
NO_WINDOW = 1 << 24   # for the reference: a window that hides nothing
IDS = dict(ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else None)


def cache8(a, capacity, lens, nq=0, w=None):
    """(bh, nk, d) codes -> fp8 device cache (bh, capacity, d): rows [lo_slab, len) of every slab, the NaN code everywhere else"""
    t = torch.full((a.shape[0], capacity, a.shape[2]), 0xFF, dtype=torch.uint8, device=dev())
    for s, n in enumerate(lens):
        lo = 0 if w is None else lo_slab(n, nq, w)
        t[s, lo:n] = u8(a[s, lo:n])
    return t.view(F8)


def same_bits_as_bf16(qd, k8, v8, causal, nk, lens_d=None, w=None):
    """scales 1 and 0.125, both output dtypes: O for v_scale 1 and 0.5, the LSE also at 0.011.  Returns the last fp8 result."""
    kb, vb = as_bf16(k8), as_bf16(v8)
    for scale in (1.0, 0.125):
        for odt in (torch.float32, torch.bfloat16):
            ref, lse_ref = fa.forward_kv(qd, kb, vb, causal, kv_len=nk, kv_lens=lens_d, scale=folded(scale, KS), out_dtype=odt, return_lse=True, window_left=w)
            for vs in (1.0, 0.5, VS):
                o, lse = fa.forward_kv_fp8(qd, k8, v8, causal, k_scale=KS, v_scale=vs, kv_len=nk, kv_lens=lens_d, scale=scale, out_dtype=odt,
                                           return_lse=True, window_left=w)
                assert o.dtype == odt and not bool(torch.isnan(o.float()).any()), "a NaN code was read"
                assert ar.bit_equal(lse, lse_ref), f"LSE differs from the bf16 kernel's (scale {scale}, {odt}, v_scale {vs}, window {w})"
                if vs != VS:   # a power of two: the product is exact in fp32 and in bf16
                    assert ar.bit_equal(o, (vs * ref).to(odt)), f"O differs from v_scale x the bf16 kernel's (scale {scale}, {odt}, v_scale {vs}, window {w}): " \
                        f"{float((o.float() - vs * ref.float()).abs().max()):.3e}"
    return o, lse


def within_bounds(run, ref, lse_ref, what):
    """fp32 output, bf16 output and the LSE of `run(out_dtype)` against an fp64 reference"""
    o, lse = run(torch.float32)
    assert err(o, ref, f"{what} f32 out") < TOL_PB2 and err(lse, lse_ref, f"{what} lse") < TOL_LSE
    ob, lseb = run(torch.bfloat16)
    assert ob.dtype == torch.bfloat16 and err(ob, ref, f"{what} bf16 out") < TOL_BF16 and err(lseb, lse_ref, f"{what} lse (bf16 out)") < TOL_LSE
    return o


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape,splits", PARITY, **IDS)
def test_bit_identity_with_the_bf16_kernel_and_parity_with_fp64(shape, splits, causal):
    bh_kv, group, nq, nk = shape
    assert _cabi_kv8_256.lib().fa_kv8_256_splits_for(bh_kv, group, nq, nk, D, int(causal), BF16, -1) == splits
    q, kc, vc = randn(61, bh_kv * group, nq, D), codes(62, KS, bh_kv, nk, D), codes(63, VS, bh_kv, nk, D)
    qd, k8, v8 = to_dev(q), cache8(kc, nk + 70, [nk] * bh_kv), cache8(vc, nk + 70, [nk] * bh_kv)
    same_bits_as_bf16(qd, k8, v8, causal, nk)
    for scale in (1.0, 0.125):   # general scales against the fp64 reference on the logical values
        ref, lse_ref = attention_kvw(q, KS * dequant(kc), VS * dequant(vc), None, causal, scale, NO_WINDOW)
        o = within_bounds(lambda odt: fa.forward_kv_fp8(qd, k8, v8, causal, k_scale=KS, v_scale=VS, kv_len=nk, scale=scale, out_dtype=odt, return_lse=True),
                          ref, lse_ref, f"{shape} scale {scale}")
    if causal and nq > nk:   # rows i < nq - nk see nothing: exactly 0, LSE -inf (checked in err())
        assert not ref[:, :nq - nk].any() and not o[:, :nq - nk].any()


@pytest.mark.parametrize("causal", [False, True])
def test_ragged_lengths_from_device_memory(causal):
    bh_kv, group, nq, nk, lens = 4, 4, 2, 1024, [0, 1, 777, 1024]
    qd = to_dev(randn(71, bh_kv * group, nq, D))
    k8, v8 = cache8(codes(72, KS, bh_kv, nk, D), nk, lens), cache8(codes(73, VS, bh_kv, nk, D), nk, lens)
    o, lse = same_bits_as_bf16(qd, k8, v8, causal, nk, lens_d=torch.tensor(lens, dtype=torch.int32, device=dev()))
    assert not o[:group].any() and bool((lse[:group] == float("-inf")).all())   # the empty slab: exactly 0 and -inf


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("w", [0, 31, 100])
def test_sliding_window_reads_nothing_below_it(w, causal):
    bh_kv, group, nq, nk = 2, 4, 3, 700
    qd = to_dev(randn(81, bh_kv * group, nq, D))
    kc, vc = codes(82, KS, bh_kv, nk, D), codes(83, VS, bh_kv, nk, D)
    same_bits_as_bf16(qd, cache8(kc, nk + 70, [nk] * bh_kv, nq, w), cache8(vc, nk + 70, [nk] * bh_kv, nq, w), causal, nk, w=w)
    if w == 0:   # a window that hides nothing gives the bits of no window
        k8, v8 = cache8(kc, nk, [nk] * bh_kv), cache8(vc, nk, [nk] * bh_kv)
        for odt in (torch.float32, torch.bfloat16):
            want = fa.forward_kv_fp8(qd, k8, v8, causal, k_scale=KS, v_scale=VS, out_dtype=odt, return_lse=True)
            got = fa.forward_kv_fp8(qd, k8, v8, causal, k_scale=KS, v_scale=VS, out_dtype=odt, return_lse=True, window_left=1 << 24)
            assert ar.bit_equal(got[0], want[0]) and ar.bit_equal(got[1], want[1]), odt


@pytest.mark.parametrize("w", [None, 100])
@pytest.mark.parametrize("page", [16, 64])
def test_paged_is_the_contiguous_entry_on_the_gathered_bytes(page, w):
    batch, H, group, nq, nk, lens = 2, 2, 2, 3, 1000, [1000, 613]
    assert _cabi_kv8_256.lib().fa_kv8_256_paged_splits_for(batch, H, group, nq, nk, D, 1, BF16, -1 if w is None else w) == (3 if w is None else 1)
    q, kc, vc = randn(101, batch * H * group, nq, D), codes(102, KS, batch * H, nk, D), codes(103, VS, batch * H, nk, D)
    cache = Cache8(kc, vc, batch, H, lens, page, seed=page)   # shuffled; unused pages and tails 0xFF; entries past a length out of range
    gk, gv, slab_lens = cache.gathered(nk)
    qd = to_dev(q)
    for causal in (False, True):
        ref, lse_ref = attention_kvw(q, KS * dequant(kc), VS * dequant(vc), [n for n in lens for _ in range(H)], causal, 1.0, NO_WINDOW if w is None else w)
        within_bounds(lambda odt: cache.run(qd, causal, nk, out_dtype=odt, return_lse=True, window_left=w), ref, lse_ref, f"paged {page} causal={causal}")
        for odt in (torch.float32, torch.bfloat16):
            o, lse = cache.run(qd, causal, nk, out_dtype=odt, return_lse=True, window_left=w)
            oc, lsec = fa.forward_kv_fp8(qd, gk, gv, causal, k_scale=KS, v_scale=VS, kv_len=nk, kv_lens=slab_lens, out_dtype=odt, return_lse=True, window_left=w)
            assert ar.bit_equal(o, oc) and ar.bit_equal(lse, lsec), (odt, causal)
