"""GPU: chunked prefill under a sliding window (include/flashattn_amd_kvpw.h; window_left on fa.prefill_kv / prefill_paged and their _fp8
twins) against the fp64 reference tests/kvw_reference.py, the unwindowed kernels, the decode kernels, and bit for bit between paged and
contiguous and between fp8 and bf16.  Data and bars are those of tests/test_gpu_kvp.py / test_gpu_kvp256.py / test_gpu_kvp8.py
(fp32 O 2e-4, LSE 1e-4, bf16 O 2.5e-2).  Every cache holds NaN (fp8: the NaN code) in all rows below lo_slab(len, nq, window_left) and at
or beyond len; every output buffer is pre-filled with 0xFF bytes."""
import numpy as np
import pytest
import torch

import flashattention_c_amd as fa
from tests.arena import bit_equal
from tests.kv8_reference import dequant
from tests.kvw_reference import attention_kvw, lo_slab
from tests.test_gpu_kvp import TOL_BF16, TOL_LSE, TOL_PB2, dev, err, randn, to_dev
from tests.test_gpu_kvp8 import F8, KS, VS, codes, to_dev8

pytestmark = pytest.mark.gpu

KINDS = {"bf16-128": (128, False), "bf16-256": (256, False), "fp8-128": (128, True)}
WINDOWS = [0, 5, 31, 32, 63, 100, 333]   # inside a 32-key half, on a half and on a block boundary, shorter and longer than a tile
BARS = ((torch.float32, TOL_PB2), (torch.bfloat16, TOL_BF16))
SCALES = {False: {}, True: dict(k_scale=KS, v_scale=VS)}


def shapes(d):
    """(bh_kv, group, nq, nk, lens): one tile whose walk starts beyond block 0 with the lower edge through every wave; tiles straddling heads
    over two slabs of different lengths; a last tile with three empty waves; causal nq > len with rows and waves without a key"""
    return [(1, 1, 2 * d if d == 128 else 128, 700, None), (2, 2, 200, 700, [700, 333]), (1, 4, 70, 321, None), (2, 1, 300, 129, None)]


def tensors(kind, shape, w, seed=401):
    """q, K, V as arrays, and on the device with NaN (the NaN code) in every row outside [lo_slab, len)"""
    (d, fp8), (bh_kv, group, nq, nk, lens) = KINDS[kind], shape
    q = randn(seed, bh_kv * group, nq, d)
    k, v = (codes(seed + 1 + i, s, bh_kv, nk, d) if fp8 else randn(seed + 1 + i, bh_kv, nk, d) for i, s in enumerate((KS, VS)))
    masked = []
    for a in (k, v):
        t = np.full((bh_kv, nk + 70, d), 0xFF if fp8 else np.nan, dtype=a.dtype)
        for s, n in enumerate(lens or [nk] * bh_kv):
            t[s, lo_slab(n, nq, w):n] = a[s, lo_slab(n, nq, w):n]
        masked.append(t)
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev())
    return q, k, v, to_dev(q), masked, lens_d


def put(fp8, a):
    return to_dev8(a) if fp8 else to_dev(a)


def poisoned(qd, odt):
    return torch.full((*qd.shape[:-1], qd.shape[-1] * odt.itemsize), 0xFF, dtype=torch.uint8, device=dev()).view(odt)


def prefill(fp8, qd, kd, vd, causal, odt, **kw):
    return (fa.prefill_kv_fp8 if fp8 else fa.prefill_kv)(qd, kd, vd, causal, out=poisoned(qd, odt), return_lse=True, **kw)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("si", range(4))
@pytest.mark.parametrize("kind", KINDS)
def test_parity_against_the_fp64_reference_and_the_decode_kernel(kind, si, w, causal):
    (_, fp8), shape = KINDS[kind], shapes(KINDS[kind][0])[si]
    nk, lens = shape[3:]
    q, k, v, qd, (km, vm), lens_d = tensors(kind, shape, w)
    kd, vd = put(fp8, km), put(fp8, vm)
    kl, vl = (KS * dequant(k), VS * dequant(v)) if fp8 else (k, v)
    for scale in (1.0, 1.0 / 16):
        ref, lse_ref = attention_kvw(q, kl, vl, lens, causal, scale, w)
        kw = dict(kv_len=nk, kv_lens=lens_d, scale=scale, window_left=w, **SCALES[fp8])
        for odt, tol in reversed(BARS):
            o, lse = prefill(fp8, qd, kd, vd, causal, odt, **kw)
            assert o.dtype == odt and err(o, ref, f"{kind} {shape} w={w} {odt} scale {scale}") < tol
            assert err(lse, lse_ref, f"{kind} {shape} w={w} lse scale {scale}") < TOL_LSE   # err() holds the -inf entries to equality
            assert not o[torch.from_numpy(np.isinf(lse_ref)).to(dev())].any(), "a row without a key must be exactly 0"
        b = (fa.forward_kv_fp8 if fp8 else fa.forward_kv)(qd, kd, vd, causal, out_dtype=torch.float32, **kw)
        assert float((o - b).abs().max()) < 2 * TOL_PB2, "the fp32 output against the decode kernel under the same window"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("si", range(4))
@pytest.mark.parametrize("kind", KINDS)
def test_a_window_that_hides_nothing_gives_the_unwindowed_bits(kind, si, causal):
    (_, fp8), shape = KINDS[kind], shapes(KINDS[kind][0])[si]
    nk = shape[3]
    _, _, _, qd, (km, vm), lens_d = tensors(kind, shape, nk)
    kd, vd = put(fp8, km), put(fp8, vm)
    for odt, _ in BARS:
        kw = dict(kv_len=nk, kv_lens=lens_d, scale=0.25, **SCALES[fp8])
        o0, lse0 = prefill(fp8, qd, kd, vd, causal, odt, **kw)
        for w in (nk, 1 << 30):
            o, lse = prefill(fp8, qd, kd, vd, causal, odt, window_left=w, **kw)
            assert bit_equal(o, o0) and bit_equal(lse, lse0), (odt, w)


@pytest.mark.parametrize("w", WINDOWS + [700])
@pytest.mark.parametrize("permuted", [False, True], ids=["pages-page-H-d", "pages-H-page-d-view"])
@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_paged_equals_contiguous_on_the_gathered_cache(kind, page, permuted, w):
    (d, fp8), (batch, H, group, nq, nk, lens) = KINDS[kind], (2, 2, 2, 200, 700, [700, 333])
    slab_lens = [n for n in lens for _ in range(H)]
    _, _, _, qd, (km, vm), _ = tensors(kind, (batch * H, group, nq, nk, slab_lens), w, seed=431)
    max_pages = -(-nk // page) + 2
    live = [(b, p) for b, n in enumerate(lens) for p in range(lo_slab(n, nq, w) // page, -(-n // page))]   # pages not wholly below lo
    order = [int(x) for x in np.random.default_rng(page).permutation(len(live) + 3)]   # a shuffled table; the pages left over stay NaN
    nan_page = order.pop()
    table = np.full((batch, max_pages), nan_page, dtype=np.int32)   # entries of pages that slid out, and past the length: one page of NaN
    pools = [np.full((len(live) + 3, page, H, d), 0xFF if fp8 else np.nan, dtype=a.dtype) for a in (km, vm)]
    for b, p in live:
        phys = table[b, p] = order.pop()
        for pool, a in zip(pools, (km, vm)):   # whole pages of the masked cache: their rows below lo and at or beyond len are NaN too
            pool[phys] = a[b * H:(b + 1) * H, p * page:(p + 1) * page].transpose(1, 0, 2)
    kpd, vpd = ((put(fp8, x.transpose(0, 2, 1, 3)).permute(0, 2, 1, 3) if permuted else put(fp8, x)) for x in pools)
    kd, vd, table_d = put(fp8, km), put(fp8, vm), torch.from_numpy(table).to(dev())
    lens_d, slab_lens_d = (torch.tensor(x, dtype=torch.int32, device=dev()) for x in (lens, slab_lens))
    for causal in (False, True):
        for odt, _ in BARS:
            kw = dict(kv_len=nk, window_left=w, return_lse=True, **SCALES[fp8])
            o, lse = (fa.prefill_paged_fp8 if fp8 else fa.prefill_paged)(qd, kpd, vpd, table_d, causal, seq_lens=lens_d, out=poisoned(qd, odt), **kw)
            oc, lsec = (fa.prefill_kv_fp8 if fp8 else fa.prefill_kv)(qd, kd, vd, causal, kv_lens=slab_lens_d, out=poisoned(qd, odt), **kw)
            assert not torch.isnan(o.float()).any() and bit_equal(o, oc) and bit_equal(lse, lsec), (odt, causal)
            if w >= nk:   # ... and a window that hides nothing gives the bits of the unwindowed paged kernel
                kw.pop("window_left")
                o0, lse0 = (fa.prefill_paged_fp8 if fp8 else fa.prefill_paged)(qd, kpd, vpd, table_d, causal, seq_lens=lens_d, out=poisoned(qd, odt), **kw)
                assert bit_equal(o, o0) and bit_equal(lse, lse0), (odt, causal)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("si", range(4))
def test_fp8_is_v_scale_times_the_bf16_kernel_on_the_dequantised_cache(si, w, causal):
    shape = shapes(128)[si]
    nk = shape[3]
    _, _, _, qd, (km, vm), lens_d = tensors("fp8-128", shape, w)
    k8, v8 = to_dev8(km), to_dev8(vm)
    kb, vb = (t.view(torch.uint8).cpu().view(F8).to(torch.bfloat16).to(dev()) for t in (k8, v8))   # exact; a NaN code becomes a bf16 NaN
    for odt, _ in BARS:
        kw = dict(kv_len=nk, kv_lens=lens_d, window_left=w)
        ref, lse_ref = prefill(False, qd, kb, vb, causal, odt, scale=float(np.float32(0.125) * np.float32(KS)), **kw)
        for vs in (1.0, 0.5):
            o, lse = prefill(True, qd, k8, v8, causal, odt, scale=0.125, k_scale=KS, v_scale=vs, **kw)
            assert bit_equal(lse, lse_ref) and bit_equal(o, (vs * ref).to(odt)), (odt, vs)
