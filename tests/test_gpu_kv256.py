"""GPU: KV-cache attention at head dim 256 (include/flashattn_amd_kv256.h; fa.forward_kv / fa.forward_paged with d = 256) against the fp64
references tests/kv_reference.py and tests/kvw_reference.py, and bit for bit between its own paths where they must agree.

Tolerances are those of tests/test_gpu_kv.py, on its data family (seeded N(0, 1) rounded to bf16): the arithmetic is the same
    fp32 output  2e-4      LSE  1e-4      bf16 output  2.5e-2
Every device cache holds NaN in the rows the read contract excludes: at or beyond len, and below lo_slab = max(0, len - nq - window_left).
"""
import numpy as np
import pytest
import torch

import flashattention_c_amd as fa
from flashattention_c_amd import _cabi_kv256
from oracle import oracle as orc
from tests.kv_reference import attention_kv
from tests.kvw_reference import attention_kvw, lo_slab
from tests.paged_reference import gather

pytestmark = pytest.mark.gpu

D = 256
TOL_PB2, TOL_LSE, TOL_BF16 = 2e-4, 1e-4, 2.5e-2
BF16 = _cabi_kv256.FA_DTYPE_BF16
NAN = float("nan")


def dev():
    return torch.device("cuda", 0)


def randn(seed, *shape):
    return orc.round_to_bf16(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).numpy())


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(dev())


def cache(a, capacity, lens, nq=0, w=None):
    """(bh, nk, d) array -> bf16 device cache (bh, capacity, d): rows [lo_slab, len) of every slab, NaN everywhere else"""
    t = torch.full((a.shape[0], capacity, a.shape[2]), NAN, dtype=torch.bfloat16, device=dev())
    for s, n in enumerate(lens):
        lo = 0 if w is None else lo_slab(n, nq, w)
        t[s, lo:n] = to_dev(a[s, lo:n])
    return t


def err(t, ref, what):
    got = t.detach().float().cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any(), f"NaN in {what}"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), f"{what}: -inf entries differ"
    e = float(np.abs(got[~inf] - ref[~inf]).max()) if (~inf).any() else 0.0
    print(f"{what}: max abs err {e:.3e}")
    return e


def check_all(q, k, v, qd, kd, vd, nk, causal, w=None, lens=None, what=""):
    """both scales, both output dtypes, output and LSE"""
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev())
    for scale in (1.0, 1.0 / 16):
        ref, lse_ref = attention_kv(q, k, v, lens, causal, scale) if w is None else attention_kvw(q, k, v, lens, causal, scale, w)
        for odt, tol in ((torch.float32, TOL_PB2), (torch.bfloat16, TOL_BF16)):
            o, lse = fa.forward_kv(qd, kd, vd, causal, kv_len=nk, kv_lens=lens_d, scale=scale, out_dtype=odt, return_lse=True, window_left=w)
            assert o.dtype == odt
            assert err(o, ref, f"{what} {odt} scale {scale}") < tol
            assert err(lse, lse_ref, f"{what} lse ({odt}) scale {scale}") < TOL_LSE
    return ref


# (bh_kv, group, nq, nk), key shares S
PARITY = [
    ((2, 1, 1, 1), 1),         # one key
    ((3, 4, 1, 31), 1),        # below one block
    ((2, 8, 1, 33), 1),        # across a 32-key block edge: the second wave
    ((1, 8, 1, 257), 1),       # all four waves, a third round: both V images and both K sets
    ((2, 4, 5, 1000), 3),      # a ragged last share, packed rows straddling heads
    ((1, 4, 33, 700), 2),      # M = 132: five row tiles
    ((2, 1, 40, 24), 1),       # causal with nq > nk: rows without keys
]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape,splits", PARITY, ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else None)
def test_parity_against_the_fp64_reference(shape, splits, causal):
    bh_kv, group, nq, nk = shape
    assert _cabi_kv256.lib().fa_kv256_splits_for(bh_kv, group, nq, nk, D, int(causal), BF16, -1) == splits
    q, k, v = randn(61, bh_kv * group, nq, D), randn(62, bh_kv, nk, D), randn(63, bh_kv, nk, D)
    qd, kd, vd = to_dev(q), cache(k, nk + 70, [nk] * bh_kv), cache(v, nk + 70, [nk] * bh_kv)
    ref = check_all(q, k, v, qd, kd, vd, nk, causal, what=str(shape))
    if causal and nq > nk:   # rows i < nq - nk see nothing: exactly 0, LSE -inf (checked in err())
        o = fa.forward_kv(qd, kd, vd, True, kv_len=nk, out_dtype=torch.float32)
        assert not ref[:, :nq - nk].any() and not o[:, :nq - nk].any()


@pytest.mark.parametrize("causal", [False, True])
def test_ragged_lengths_from_device_memory(causal):
    bh_kv, group, nq, nk, lens = 4, 4, 2, 1024, [0, 1, 777, 1024]
    q, k, v = randn(71, bh_kv * group, nq, D), randn(72, bh_kv, nk, D), randn(73, bh_kv, nk, D)
    check_all(q, k, v, to_dev(q), cache(k, nk, lens), cache(v, nk, lens), nk, causal, lens=lens, what="ragged")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("w", [0, 31, 100])
def test_sliding_window_reads_nothing_below_it(w, causal):
    bh_kv, group, nq, nk = 2, 4, 3, 700
    q, k, v = randn(81, bh_kv * group, nq, D), randn(82, bh_kv, nk, D), randn(83, bh_kv, nk, D)
    lens = [nk] * bh_kv
    check_all(q, k, v, to_dev(q), cache(k, nk + 70, lens, nq, w), cache(v, nk + 70, lens, nq, w), nk, causal, w=w, what=f"window {w}")


@pytest.mark.parametrize("causal", [False, True])
def test_a_window_that_hides_nothing_gives_the_bits_of_no_window(causal):
    bh_kv, group, nq, nk = 2, 4, 3, 700
    qd, kd, vd = to_dev(randn(91, bh_kv * group, nq, D)), to_dev(randn(92, bh_kv, nk, D)), to_dev(randn(93, bh_kv, nk, D))
    for odt in (torch.float32, torch.bfloat16):
        want = fa.forward_kv(qd, kd, vd, causal, out_dtype=odt, return_lse=True, window_left=None)
        got = fa.forward_kv(qd, kd, vd, causal, out_dtype=odt, return_lse=True, window_left=1 << 24)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), odt


@pytest.mark.parametrize("w", [None, 100])
@pytest.mark.parametrize("page", [16, 64])
def test_paged_equals_contiguous_on_the_gathered_cache(page, w):
    batch, H, group, nq, nk, lens = 2, 2, 2, 3, 1000, [1000, 613]
    S = _cabi_kv256.lib().fa_kv256_paged_splits_for(batch, H, group, nq, nk, D, 1, BF16, -1 if w is None else w)
    assert S == (3 if w is None else 1)
    bh_kv = batch * H
    q, k, v = randn(101, bh_kv * group, nq, D), randn(102, bh_kv, nk, D), randn(103, bh_kv, nk, D)
    max_pages = -(-nk // page) + 2
    used = [-(-n // page) for n in lens]
    pages = sum(used) + 3
    order = [int(x) for x in np.random.default_rng(page).permutation(pages)]   # a shuffled table; the pages left over stay NaN
    table = np.full((batch, max_pages), 1 << 30, dtype=np.int32)               # entries past ceil(len / page) point out of range: never read
    kp, vp = np.full((pages, page, H, D), NAN), np.full((pages, page, H, D), NAN)
    for b, n in enumerate(lens):
        for p in range(used[b]):
            phys = table[b, p] = order.pop()
            rows = min(page, n - p * page)
            kp[phys, :rows] = k[b * H:(b + 1) * H, p * page:p * page + rows].transpose(1, 0, 2)
            vp[phys, :rows] = v[b * H:(b + 1) * H, p * page:p * page + rows].transpose(1, 0, 2)
    qd, kpd, vpd, table_d = to_dev(q), to_dev(kp), to_dev(vp), torch.from_numpy(table).to(dev())
    kd, vd = to_dev(gather(kp, table, lens, nk)), to_dev(gather(vp, table, lens, nk))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    slab_lens = [n for n in lens for _ in range(H)]
    slab_lens_d = torch.tensor(slab_lens, dtype=torch.int32, device=dev())
    for causal in (False, True):
        ref, lse_ref = attention_kvw(q, k, v, slab_lens, causal, 1.0, (1 << 24) if w is None else w)
        for odt, tol in ((torch.float32, TOL_PB2), (torch.bfloat16, TOL_BF16)):
            o, lse = fa.forward_paged(qd, kpd, vpd, table_d, causal, kv_len=nk, seq_lens=lens_d, out_dtype=odt, return_lse=True, window_left=w)
            oc, lsec = fa.forward_kv(qd, kd, vd, causal, kv_len=nk, kv_lens=slab_lens_d, out_dtype=odt, return_lse=True, window_left=w)
            assert err(o, ref, f"paged {page} {odt} causal={causal}") < tol and err(lse, lse_ref, "paged lse") < TOL_LSE
            assert torch.equal(o, oc) and torch.equal(lse, lsec), (odt, causal)
