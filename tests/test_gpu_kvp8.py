"""GPU: chunked prefill over the fp8 (e4m3fn) K/V caches (include/flashattn_amd_kvp8.h; fa.prefill_kv_fp8 / fa.prefill_paged_fp8, d = 128): bit
identity with fa.prefill_kv on the dequantised cache and between the paged and the contiguous kernel, and accuracy against the fp64 reference
tests/kv_reference.py on the logical values at the bars of tests/test_gpu_kv.py (fp32 O 2e-4, LSE 1e-4, bf16 O 2.5e-2).  Data as in
tests/test_gpu_kv8.py: K, V ~ N(0, 1) quantised at k_scale = 0.013, v_scale = 0.011; whatever must not be read holds the NaN code 0xFF; fp8
tensors are built on the CPU and cross to the device as bytes."""
import functools

import numpy as np
import pytest
import torch

import flashattention_c_amd as fa
from tests.arena import bit_equal
from tests.kv8_reference import dequant, quantize
from tests.kv_reference import attention_kv
from tests.paged_reference import gather
from tests.test_gpu_kvp import PARITY, TOL_BF16, TOL_LSE, TOL_PB2, dev, err, randn, to_dev

pytestmark = pytest.mark.gpu

D = 128
KS, VS = 0.013, 0.011
F8 = torch.float8_e4m3fn
BARS = ((torch.float32, TOL_PB2), (torch.bfloat16, TOL_BF16))
IDS = dict(ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else None)


@functools.lru_cache(maxsize=None)
def codes(seed, scale, *shape):
    """N(0, 1) quantised at `scale`: the uint8 codes (read-only, shared between tests)"""
    a = quantize(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)), scale).view(torch.uint8).numpy()
    assert not np.isin(a, (0x7F, 0xFF)).any()
    a.setflags(write=False)
    return a


def to_dev8(a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).to(dev()).view(F8)


def cache8(a, capacity, lens):
    """(bh, nk, d) codes -> fp8 device cache (bh, capacity, d): rows [0, len) of every slab, the NaN code everywhere else"""
    t = np.full((a.shape[0], capacity, a.shape[2]), 0xFF, dtype=np.uint8)
    for s, n in enumerate(lens):
        t[s, :n] = a[s, :n]
    return to_dev8(t)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", PARITY, **IDS)
def test_bit_identity_with_the_bf16_prefill_kernel_on_the_dequantised_cache(shape, causal):
    bh_kv, group, nq, nk = shape
    qd = to_dev(randn(61, bh_kv * group, nq, D))
    k8, v8 = cache8(codes(62, KS, bh_kv, nk, D), nk + 70, [nk] * bh_kv), cache8(codes(63, VS, bh_kv, nk, D), nk + 70, [nk] * bh_kv)
    kb, vb = (t.view(torch.uint8).cpu().view(F8).to(torch.bfloat16).to(dev()) for t in (k8, v8))   # exact; a NaN code becomes a bf16 NaN
    assert bool(torch.isnan(kb[:, nk:].float()).all())
    for scale in (1.0, 0.125):
        for odt in (torch.float32, torch.bfloat16):
            ref, lse_ref = fa.prefill_kv(qd, kb, vb, causal, kv_len=nk, scale=float(np.float32(scale) * np.float32(KS)), out_dtype=odt, return_lse=True)
            for vs in (1.0, 0.5, VS):
                o, lse = fa.prefill_kv_fp8(qd, k8, v8, causal, k_scale=KS, v_scale=vs, kv_len=nk, scale=scale, out_dtype=odt, return_lse=True)
                assert o.dtype == odt and bit_equal(lse, lse_ref), f"LSE differs from the bf16 kernel's (scale {scale}, {odt}, v_scale {vs})"
                if vs != VS:   # a power of two: the product is exact in fp32 and in bf16
                    assert bit_equal(o, (vs * ref).to(odt)), f"O differs from v_scale x the bf16 kernel's (scale {scale}, {odt}, v_scale {vs}): " \
                        f"{float((o.float() - vs * ref.float()).abs().max()):.3e}"


def check_all(q, kc, vc, lens, nk, causal, what):
    """general scales, both softmax scales, both output dtypes, output and LSE against the fp64 reference on the logical values"""
    qd, k8, v8 = to_dev(q), cache8(kc, nk + 70, lens or [nk] * len(kc)), cache8(vc, nk + 70, lens or [nk] * len(kc))
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev())
    k, v = KS * dequant(kc), VS * dequant(vc)
    for scale in (1.0, 0.125):
        ref, lse_ref = attention_kv(q, k, v, lens, causal, scale)
        for odt, tol in BARS:
            o, lse = fa.prefill_kv_fp8(qd, k8, v8, causal, k_scale=KS, v_scale=VS, kv_len=nk, kv_lens=lens_d, scale=scale, out_dtype=odt, return_lse=True)
            assert err(o, ref, f"{what} {odt} scale {scale}") < tol
            assert err(lse, lse_ref, f"{what} lse ({odt}) scale {scale}") < TOL_LSE
    return ref, o


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", PARITY, **IDS)
def test_general_scales_against_the_fp64_reference(shape, causal):
    bh_kv, group, nq, nk = shape
    ref, o = check_all(randn(61, bh_kv * group, nq, D), codes(62, KS, bh_kv, nk, D), codes(63, VS, bh_kv, nk, D), None, nk, causal, str(shape))
    if causal and nq > nk:   # rows i < nq - nk see nothing: exactly 0, LSE -inf (checked in err())
        assert not ref[:, :nq - nk].any() and not o[:, :nq - nk].any()


@pytest.mark.parametrize("causal", [False, True])
def test_ragged_lengths_from_device_memory(causal):
    bh_kv, group, nq, nk, lens = 4, 4, 40, 1024, [0, 1, 777, 1024]
    check_all(randn(71, bh_kv * group, nq, D), codes(72, KS, bh_kv, nk, D), codes(73, VS, bh_kv, nk, D), lens, nk, causal, "ragged")


@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("permuted", [False, True], ids=["pages-page-H-d", "pages-H-page-d-view"])
def test_paged_equals_contiguous_on_the_gathered_bytes(page, permuted):
    batch, H, group, nq, nk, lens = 2, 2, 2, 70, 1000, [1000, 613]
    bh_kv = batch * H
    q, kc, vc = randn(101, bh_kv * group, nq, D), codes(102, KS, bh_kv, nk, D), codes(103, VS, bh_kv, nk, D)
    max_pages, used = -(-nk // page) + 2, [-(-n // page) for n in lens]
    pages = sum(used) + 3
    order = [int(x) for x in np.random.default_rng(page).permutation(pages)]   # a shuffled table; the pages left over stay NaN codes
    nan_page = order.pop()
    table = np.full((batch, max_pages), nan_page, dtype=np.int32)              # entries past ceil(len / page): a valid page of NaN codes
    kp, vp = np.full((pages, page, H, D), 0xFF, dtype=np.uint8), np.full((pages, page, H, D), 0xFF, dtype=np.uint8)
    for b, n in enumerate(lens):
        for p in range(used[b]):
            phys = table[b, p] = order.pop()
            rows = min(page, n - p * page)
            kp[phys, :rows] = kc[b * H:(b + 1) * H, p * page:p * page + rows].transpose(1, 0, 2)
            vp[phys, :rows] = vc[b * H:(b + 1) * H, p * page:p * page + rows].transpose(1, 0, 2)
    qd, table_d = to_dev(q), torch.from_numpy(table).to(dev())
    kpd, vpd = ((to_dev8(x.transpose(0, 2, 1, 3)).permute(0, 2, 1, 3) if permuted else to_dev8(x)) for x in (kp, vp))
    slab_lens = [n for n in lens for _ in range(H)]
    gk, gv = gather(kp, table, lens, nk), gather(vp, table, lens, nk)
    for s, n in enumerate(slab_lens):   # what the gather leaves past a length: NaN codes, like the pages' tails
        gk[s, n:], gv[s, n:] = 0xFF, 0xFF
    kd, vd = to_dev8(gk), to_dev8(gv)
    lens_d, slab_lens_d = (torch.tensor(x, dtype=torch.int32, device=dev()) for x in (lens, slab_lens))
    kw = dict(k_scale=KS, v_scale=VS, kv_len=nk, return_lse=True)
    for causal in (False, True):
        ref, lse_ref = attention_kv(q, KS * dequant(kc), VS * dequant(vc), slab_lens, causal, 1.0)
        for odt, tol in BARS:
            o, lse = fa.prefill_paged_fp8(qd, kpd, vpd, table_d, causal, seq_lens=lens_d, out_dtype=odt, **kw)
            oc, lsec = fa.prefill_kv_fp8(qd, kd, vd, causal, kv_lens=slab_lens_d, out_dtype=odt, **kw)
            assert err(o, ref, f"paged {page} {odt} causal={causal}") < tol and err(lse, lse_ref, "paged lse") < TOL_LSE
            assert bit_equal(o, oc) and bit_equal(lse, lsec), (odt, causal)


@pytest.mark.parametrize("causal", [False, True])
def test_a_constant_v_comes_out_as_v_scale_exactly(causal):
    bh_kv, group, nq, nk = 1, 4, 70, 321   # a ragged last block, a partial second tile; nq <= nk: every row sees a key
    qd, k8 = to_dev(randn(81, bh_kv * group, nq, D)), cache8(codes(82, KS, bh_kv, nk, D), nk + 70, [nk])
    v8 = cache8(np.full((bh_kv, nk, D), 0x38, dtype=np.uint8), nk + 70, [nk])   # 0x38: the code of 1.0
    for odt in (torch.float32, torch.bfloat16):
        o = fa.prefill_kv_fp8(qd, k8, v8, causal, k_scale=KS, v_scale=VS, kv_len=nk, out_dtype=odt)
        assert torch.equal(o, torch.full_like(o, float(np.float32(VS)))), (causal, odt)   # full_like rounds fp32(v_scale) to bf16 for the bf16 output
