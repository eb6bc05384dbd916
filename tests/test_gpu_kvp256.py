"""GPU: chunked prefill over the bf16 K/V caches at head dim 256 (include/flashattn_amd_kvp256.h; fa.prefill_kv / fa.prefill_paged with
d = 256) against the fp64 reference tests/kv_reference.py, bit for bit between the paged and the contiguous kernel, and against the decode
kernel of include/flashattn_amd_kv256.h.  The tile built is the 128 rows of the design, so the shapes are the issue's.

Tolerances are those of tests/test_gpu_kv256.py, on its data family (seeded N(0, 1) rounded to bf16): the same arithmetic at the same d
    fp32 output  2e-4      LSE  1e-4      bf16 output  2.5e-2
Every device cache holds NaN in the rows the read contract excludes: at or beyond len.
"""
import numpy as np
import pytest
import torch

import flashattention_c_amd as fa
from oracle import oracle as orc
from tests.kv_reference import attention_kv
from tests.paged_reference import gather

pytestmark = pytest.mark.gpu

D = 256
TOL_PB2, TOL_LSE, TOL_BF16 = 2e-4, 1e-4, 2.5e-2
NAN = float("nan")


def dev():
    return torch.device("cuda", 0)


def randn(seed, *shape):
    return orc.round_to_bf16(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).numpy())


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(dev())


def cache(a, capacity, lens):
    """(bh, nk, d) array -> bf16 device cache (bh, capacity, d): rows [0, len) of every slab, NaN everywhere else"""
    t = torch.full((a.shape[0], capacity, a.shape[2]), NAN, dtype=torch.bfloat16, device=dev())
    for s, n in enumerate(lens):
        t[s, :n] = to_dev(a[s, :n])
    return t


def err(t, ref, what):
    got = t.detach().float().cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any(), f"NaN in {what}"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), f"{what}: -inf entries differ"
    e = float(np.abs(got[~inf] - ref[~inf]).max()) if (~inf).any() else 0.0
    print(f"{what}: max abs err {e:.3e}")
    return e


def check_all(q, k, v, qd, kd, vd, nk, causal, lens=None, what=""):
    """both scales, both output dtypes, output and LSE"""
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev())
    for scale in (1.0, 1.0 / 16):
        ref, lse_ref = attention_kv(q, k, v, lens, causal, scale)
        for odt, tol in ((torch.float32, TOL_PB2), (torch.bfloat16, TOL_BF16)):
            o, lse = fa.prefill_kv(qd, kd, vd, causal, kv_len=nk, kv_lens=lens_d, scale=scale, out_dtype=odt, return_lse=True)
            assert o.dtype == odt
            assert err(o, ref, f"{what} {odt} scale {scale}") < tol
            assert err(lse, lse_ref, f"{what} lse ({odt}) scale {scale}") < TOL_LSE
    return ref


def tensors(shape, seed):
    bh_kv, group, nq, nk = shape
    q, k, v = randn(seed, bh_kv * group, nq, D), randn(seed + 1, bh_kv, nk, D), randn(seed + 2, bh_kv, nk, D)
    return q, k, v, to_dev(q), cache(k, nk + 70, [nk] * bh_kv), cache(v, nk + 70, [nk] * bh_kv)


# (bh_kv, group, nq, nk)
PARITY = [
    (1, 1, 1, 1),        # one row, one key
    (2, 2, 33, 63),      # below one block; a row block straddling heads
    (1, 1, 128, 128),    # one full tile, the diagonal through every wave
    (1, 4, 70, 321),     # M = 280: three tiles, the last with 24 rows and three empty waves; six key blocks: both stages three times
    (2, 1, 300, 129),    # causal with nq > nk: rows, waves and a whole tile without keys
    (1, 8, 64, 1000),    # tiles over several heads; a ragged last block
    (1, 3, 128, 200),    # the nq % 128 == 0 tile order with group > 1
    (3, 3, 100, 160),    # the tiles - 1 - u order with tiles that straddle heads
]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", PARITY, ids=lambda x: "-".join(map(str, x)))
def test_parity_against_the_fp64_reference(shape, causal):
    nq, nk = shape[2:]
    q, k, v, qd, kd, vd = tensors(shape, 261)
    ref = check_all(q, k, v, qd, kd, vd, nk, causal, what=str(shape))
    if causal and nq > nk:   # rows i < nq - nk see nothing: exactly 0, LSE -inf (checked in err())
        o = fa.prefill_kv(qd, kd, vd, True, kv_len=nk, out_dtype=torch.float32)
        assert not ref[:, :nq - nk].any() and not o[:, :nq - nk].any()


@pytest.mark.parametrize("causal", [False, True])
def test_ragged_lengths_from_device_memory(causal):
    bh_kv, group, nq, nk, lens = 4, 4, 40, 1024, [0, 1, 777, 1024]
    q, k, v = randn(271, bh_kv * group, nq, D), randn(272, bh_kv, nk, D), randn(273, bh_kv, nk, D)
    check_all(q, k, v, to_dev(q), cache(k, nk, lens), cache(v, nk, lens), nk, causal, lens=lens, what="ragged")


def test_a_constant_v_comes_out_exactly():
    bh_kv, group, nq, nk = 1, 4, 70, 321   # a ragged last block, a partial last tile
    qd, kd = to_dev(randn(281, bh_kv * group, nq, D)), cache(randn(282, bh_kv, nk, D), nk + 70, [nk])
    vd = torch.full((bh_kv, nk + 70, D), NAN, dtype=torch.bfloat16, device=dev())
    vd[:, :nk] = 0.5
    for causal in (False, True):
        o = fa.prefill_kv(qd, kd, vd, causal, kv_len=nk, out_dtype=torch.float32)
        assert torch.equal(o, torch.full_like(o, 0.5)), causal   # nq <= nk: every row sees a key


@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("permuted", [False, True], ids=["pages-page-H-d", "pages-H-page-d-view"])
def test_paged_equals_contiguous_on_the_gathered_cache(page, permuted):
    batch, H, group, nq, nk, lens = 2, 2, 2, 70, 1000, [1000, 613]
    bh_kv = batch * H
    q, k, v = randn(301, bh_kv * group, nq, D), randn(302, bh_kv, nk, D), randn(303, bh_kv, nk, D)
    max_pages = -(-nk // page) + 2
    used = [-(-n // page) for n in lens]
    pages = sum(used) + 3
    order = [int(x) for x in np.random.default_rng(page).permutation(pages)]   # a shuffled table; the pages left over stay NaN
    nan_page = order.pop()
    table = np.full((batch, max_pages), nan_page, dtype=np.int32)              # entries past ceil(len / page): a valid page of NaN
    kp, vp = np.full((pages, page, H, D), NAN), np.full((pages, page, H, D), NAN)
    for b, n in enumerate(lens):
        for p in range(used[b]):
            phys = table[b, p] = order.pop()
            rows = min(page, n - p * page)
            kp[phys, :rows] = k[b * H:(b + 1) * H, p * page:p * page + rows].transpose(1, 0, 2)
            vp[phys, :rows] = v[b * H:(b + 1) * H, p * page:p * page + rows].transpose(1, 0, 2)
    qd, table_d = to_dev(q), torch.from_numpy(table).to(dev())
    if permuted:
        kpd, vpd = (to_dev(x.transpose(0, 2, 1, 3)).permute(0, 2, 1, 3) for x in (kp, vp))
    else:
        kpd, vpd = to_dev(kp), to_dev(vp)
    kd, vd = to_dev(gather(kp, table, lens, nk)), to_dev(gather(vp, table, lens, nk))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    slab_lens = [n for n in lens for _ in range(H)]
    slab_lens_d = torch.tensor(slab_lens, dtype=torch.int32, device=dev())
    for causal in (False, True):
        ref, lse_ref = attention_kv(q, k, v, slab_lens, causal, 1.0)
        for odt, tol in ((torch.float32, TOL_PB2), (torch.bfloat16, TOL_BF16)):
            o, lse = fa.prefill_paged(qd, kpd, vpd, table_d, causal, kv_len=nk, seq_lens=lens_d, out_dtype=odt, return_lse=True)
            oc, lsec = fa.prefill_kv(qd, kd, vd, causal, kv_len=nk, kv_lens=slab_lens_d, out_dtype=odt, return_lse=True)
            assert err(o, ref, f"paged {page} {odt} causal={causal}") < tol and err(lse, lse_ref, "paged lse") < TOL_LSE
            assert torch.equal(o, oc) and torch.equal(lse, lsec), (odt, causal)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", [PARITY[3], PARITY[5]], ids=lambda x: "-".join(map(str, x)))
def test_agrees_with_the_decode_kernel(shape, causal):
    nk = shape[3]
    q, k, v, qd, kd, vd = tensors(shape, 311)
    ref, _ = attention_kv(q, k, v, None, causal, 1.0)
    a = fa.prefill_kv(qd, kd, vd, causal, kv_len=nk, out_dtype=torch.float32)
    b = fa.forward_kv(qd, kd, vd, causal, kv_len=nk, out_dtype=torch.float32)
    assert err(a, ref, "prefill_kv") < TOL_PB2 and err(b, ref, "forward_kv") < TOL_PB2
    assert float((a - b).abs().max()) < 2 * TOL_PB2
