"""GPU: sliding-window KV-cache attention (include/flashattn_amd_kvw.h; fa.forward_kv / fa.forward_paged with window_left) against the fp64
reference tests/kvw_reference.py, and bit for bit against the unwindowed libraries wherever the window changes nothing.

Tolerances are those of tests/test_gpu_kv.py, on its data family (seeded N(0, 1) rounded to bf16, scale 1.0 and 0.125): the arithmetic is the same
    fp32 output  2e-4      LSE  1e-4      bf16 output  2.5e-2
Every cache is built so that the rows the read contract excludes -- at or beyond len AND below lo_slab = max(0, len - nq - window_left) -- are NaN,
and every paged table entry outside [lo_slab // page, ceil(len / page)) names one valid page of NaN rows.
"""
import ctypes

import numpy as np
import pytest
import torch

import flashattention_c_amd as fa
from flashattention_c_amd import _cabi_kv, _cabi_kvw
from oracle import oracle as orc
from tests import arena as ar
from tests.kvw_reference import attention_kvw, lo_slab
from tests.paged_reference import gather

pytestmark = pytest.mark.gpu

TOL_PB2, TOL_LSE, TOL_BF16 = 2e-4, 1e-4, 2.5e-2
BF16, BF16_F32 = _cabi_kvw.FA_DTYPE_BF16, _cabi_kvw.FA_DTYPE_BF16_OUT_F32
NAN = float("nan")


def dev():
    return torch.device("cuda", 0)


def randn(seed, *shape):
    return orc.round_to_bf16(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).numpy())


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(dev())


def window_cache(a, capacity, lens, nq, w):
    """(bh, nk, d) array -> bf16 device cache (bh, capacity, d) that holds rows [lo_slab, len) of every slab and NaN everywhere else"""
    t = torch.full((a.shape[0], capacity, a.shape[2]), NAN, dtype=torch.bfloat16, device=dev())
    for s, n in enumerate(lens):
        lo = lo_slab(n, nq, w)
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


def check_all(q, k, v, qd, kd, vd, nk, causal, w, lens=None, lens_d=None, what=""):
    """both scales, both output dtypes, output and LSE"""
    for scale in (1.0, 0.125):
        ref, lse_ref = attention_kvw(q, k, v, lens, causal, scale, w)
        o, lse = fa.forward_kv(qd, kd, vd, causal, kv_len=nk, kv_lens=lens_d, scale=scale, out_dtype=torch.float32, return_lse=True, window_left=w)
        assert err(o, ref, f"{what} f32 out scale {scale}") < TOL_PB2
        assert err(lse, lse_ref, f"{what} lse scale {scale}") < TOL_LSE
        ob, lseb = fa.forward_kv(qd, kd, vd, causal, kv_len=nk, kv_lens=lens_d, scale=scale, return_lse=True, window_left=w)
        assert ob.dtype == torch.bfloat16
        assert err(ob, ref, f"{what} bf16 out scale {scale}") < TOL_BF16
        assert err(lseb, lse_ref, f"{what} lse (bf16 out) scale {scale}") < TOL_LSE
    return ref


# ---- 1. parity ----
# (bh_kv, group, nq, nk, d, window_left), does the plan split?
PARITY = [
    ((2, 1, 1, 1, 64, 0), False),
    ((3, 4, 1, 300, 64, 0), False),           # one key: P = 1 exactly
    ((2, 8, 1, 257, 128, 63), False),         # the lower edge inside a block
    ((2, 4, 5, 1000, 64, 100), False),        # rows of one tile with different edges, straddling heads
    ((1, 8, 16, 4099, 128, 1500), True),      # S > 1 with a ragged last share
    ((1, 4, 33, 700, 64, 40), False),         # several row tiles
    ((1, 1, 96, 2048, 64, 31), False),        # three row tiles with disjoint key ranges: the base of a tile is the TILE's lowest key
    ((2, 1, 40, 24, 128, 7), False),          # causal with nq > len: rows without keys
    ((130, 1, 1, 300, 128, 17), False),
]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape,splits", PARITY, ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else None)
def test_parity_against_the_fp64_reference(shape, splits, causal):
    bh_kv, group, nq, nk, d, w = shape
    S = _cabi_kvw.lib().fa_kvw_splits_for(bh_kv, group, nq, nk, d, int(causal), BF16, w)
    assert (S > 1) == splits and 1 <= S <= 64, S
    q, k, v = randn(61, bh_kv * group, nq, d), randn(62, bh_kv, nk, d), randn(63, bh_kv, nk, d)
    qd, kd, vd = to_dev(q), window_cache(k, nk + 70, [nk] * bh_kv, nq, w), window_cache(v, nk + 70, [nk] * bh_kv, nq, w)
    ref = check_all(q, k, v, qd, kd, vd, nk, causal, w, what=str(shape))
    if w == 0 and nq == 1:   # the one visible key has weight 1 exactly: V[len - 1], bit for bit
        o = fa.forward_kv(qd, kd, vd, causal, kv_len=nk, out_dtype=torch.float32, window_left=0)
        want = vd[:, nk - 1].float().repeat_interleave(group, dim=0)[:, None, :]
        assert ar.bit_equal(o, want)
    if causal and nq > nk:   # rows i < nq - nk see nothing: exactly 0 (checked bit for bit), LSE -inf (checked in err())
        assert not ref[:, :nq - nk].any()
        o, lse = fa.forward_kv(qd, kd, vd, True, kv_len=nk, out_dtype=torch.float32, return_lse=True, window_left=w)
        assert not o[:, :nq - nk].any() and bool((lse[:, :nq - nk] == float("-inf")).all())


# ---- 2. ragged lengths ----
@pytest.mark.parametrize("causal", [False, True])
def test_ragged_lengths_from_device_memory(causal):
    bh_kv, group, nq, nk, d, w = 7, 4, 2, 2048, 128, 1000
    lens = [0, 1, 63, 64, 65, 777, 2048]
    assert _cabi_kvw.lib().fa_kvw_splits_for(bh_kv, group, nq, nk, d, int(causal), BF16, w) > 1
    q, k, v = randn(71, bh_kv * group, nq, d), randn(72, bh_kv, nk, d), randn(73, bh_kv, nk, d)
    qd, kd, vd = to_dev(q), window_cache(k, nk, lens, nq, w), window_cache(v, nk, lens, nq, w)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    check_all(q, k, v, qd, kd, vd, nk, causal, w, lens, lens_d, "ragged")
    # each slab equals the reference at its own length, computed on its own
    o, lse = fa.forward_kv(qd, kd, vd, causal, kv_lens=lens_d, out_dtype=torch.float32, return_lse=True, window_left=w)
    for s, n in enumerate(lens):
        sl = slice(s * group, (s + 1) * group)
        if n == 0:
            assert not o[sl].any() and bool((lse[sl] == float("-inf")).all())
            continue
        ref, lse_ref = attention_kvw(q[sl], k[s:s + 1, :n], v[s:s + 1, :n], None, causal, 1.0, w)
        assert err(o[sl], ref, f"slab {s} alone") < TOL_PB2 and err(lse[sl], lse_ref, f"slab {s} lse alone") < TOL_LSE


# ---- a paged cache under a window ----
def paged_window_cache(k, v, batch, H, lens, page, nq, w, layout, seed=0, spare=4):
    """k, v (batch * H, nk, d) arrays -> pools (device, "phd": (pages, page, H, d); "hpd": the permuted view of (pages, H, page, d)) and a shuffled
    block table (numpy).  A pool holds rows [lo_slab, len) of every sequence; every other row is NaN, and every table entry outside
    [lo_slab // page, ceil(len / page)) names one valid page that is all NaN."""
    nk, d = k.shape[1], k.shape[2]
    max_pages = -(-nk // page) + 2
    ranges = [(lo_slab(n, nq, w) // page, -(-n // page)) for n in lens]
    pages = sum(hi - lo for lo, hi in ranges) + spare
    order = [int(x) for x in np.random.default_rng(seed).permutation(pages)]
    nan_page = order.pop()
    table = np.full((batch, max_pages), nan_page, dtype=np.int32)
    kp, vp = torch.full((pages, page, H, d), NAN), torch.full((pages, page, H, d), NAN)
    for b, (n, (plo, phi)) in enumerate(zip(lens, ranges)):
        lo = lo_slab(n, nq, w)
        for p in range(plo, phi):
            phys = order.pop()
            table[b, p] = phys
            r0, r1 = max(p * page, lo), min((p + 1) * page, n)
            for pool, src in ((kp, k), (vp, v)):
                pool[phys, r0 - p * page:r1 - p * page] = torch.from_numpy(np.ascontiguousarray(src[b * H:(b + 1) * H, r0:r1])).float().transpose(0, 1)
    kd, vd = kp.to(torch.bfloat16).to(dev()), vp.to(torch.bfloat16).to(dev())
    if layout == "hpd":
        kd, vd = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (kd, vd))
        assert not kd.is_contiguous()
    return kd, vd, table, (kp.numpy().astype(np.float64), vp.numpy().astype(np.float64))


# ---- 3. no window, same bits ----
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", [(2, 4, 3, 300, 64), (2, 4, 3, 2048, 128)], ids=lambda s: "-".join(map(str, s)))
def test_a_window_that_hides_nothing_gives_the_bits_of_the_unwindowed_libraries(shape, causal):
    bh_kv, group, nq, nk, d = shape
    S = _cabi_kv.lib().fa_kv_splits_for(bh_kv, group, nq, nk, d, int(causal), BF16)
    assert (S > 1) == (nk >= 512)
    lens = [nk - 37, nk // 3]
    q, k, v = randn(131, bh_kv * group, nq, d), randn(132, bh_kv, nk, d), randn(133, bh_kv, nk, d)
    qd, kd, vd = to_dev(q), window_cache(k, nk, lens, nq, nk), window_cache(v, nk, lens, nq, nk)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    kp, vp, table, _ = paged_window_cache(k, v, bh_kv, 1, lens, 16, nq, nk, "phd", seed=3)
    table_d = torch.from_numpy(table).to(dev())
    for odt in (torch.float32, torch.bfloat16):
        want = fa.forward_kv(qd, kd, vd, causal, kv_lens=lens_d, out_dtype=odt, return_lse=True)
        wantp = fa.forward_paged(qd, kp, vp, table_d, causal, kv_len=nk, seq_lens=lens_d, out_dtype=odt, return_lse=True)
        assert ar.bit_equal(want[0], wantp[0]) and ar.bit_equal(want[1], wantp[1])
        for w in (nk - 1, 1 << 24):
            assert _cabi_kvw.lib().fa_kvw_splits_for(bh_kv, group, nq, nk, d, int(causal), BF16, w) == S
            got = fa.forward_kv(qd, kd, vd, causal, kv_lens=lens_d, out_dtype=odt, return_lse=True, window_left=w)
            assert ar.bit_equal(got[0], want[0]) and ar.bit_equal(got[1], want[1]), (odt, w)
            gotp = fa.forward_paged(qd, kp, vp, table_d, causal, kv_len=nk, seq_lens=lens_d, out_dtype=odt, return_lse=True, window_left=w)
            assert ar.bit_equal(gotp[0], want[0]) and ar.bit_equal(gotp[1], want[1]), (odt, w, "paged")


# ---- 4. an aligned window, the bits of the slice ----
@pytest.mark.parametrize("d", [64, 128])
def test_an_aligned_window_gives_the_bits_of_the_sliced_cache(d):
    """Blocks start at lo & ~63: with lo a multiple of 64 the windowed call walks the blocks a call on rows [lo, len) walks."""
    bh_kv, group, nq, nk, w = 2, 4, 1, 1024, 255
    lens = [448, 960]
    assert _cabi_kvw.lib().fa_kvw_splits_for(bh_kv, group, nq, nk, d, 1, BF16_F32, w) == 1
    assert _cabi_kv.lib().fa_kv_splits_for(1, group, nq, 256, d, 1, BF16_F32) == 1
    q, k, v = randn(141, bh_kv * group, nq, d), randn(142, bh_kv, nk, d), randn(143, bh_kv, nk, d)
    qd, kd, vd = to_dev(q), window_cache(k, nk, lens, nq, w), window_cache(v, nk, lens, nq, w)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    for causal in (True, False):
        o, lse = fa.forward_kv(qd, kd, vd, causal, kv_lens=lens_d, out_dtype=torch.float32, return_lse=True, window_left=w)
        for s, n in enumerate(lens):
            sl = slice(s * group, (s + 1) * group)
            ks, vs = kd[s:s + 1, n - 256:n].contiguous(), vd[s:s + 1, n - 256:n].contiguous()
            assert not torch.isnan(ks.float()).any()
            os_, lses = fa.forward_kv(qd[sl], ks, vs, causal, kv_len=256, out_dtype=torch.float32, return_lse=True)
            assert ar.bit_equal(o[sl], os_) and ar.bit_equal(lse[sl], lses), (causal, s)


# ---- 5. paged equals contiguous on the gathered cache ----
@pytest.mark.parametrize("layout", ["phd", "hpd"])
@pytest.mark.parametrize("page", [16, 64, 256])
@pytest.mark.parametrize("shape", [(2, 2, 2, 3, 1000, 64, 100, [1000, 613]), (1, 2, 4, 2, 2048, 128, 1000, [1999])], ids=lambda s: "-".join(map(str, s[:7])))
def test_paged_equals_contiguous_on_the_gathered_cache(shape, page, layout):
    batch, H, group, nq, nk, d, w, lens = shape
    L = _cabi_kvw.lib()
    S = L.fa_kvw_paged_splits_for(batch, H, group, nq, nk, d, 1, BF16, w)
    assert S == L.fa_kvw_splits_for(batch * H, group, nq, nk, d, 1, BF16, w) and (S > 1) == (w >= 512)
    bh_kv = batch * H
    slab_lens = [n for n in lens for _ in range(H)]
    q, k, v = randn(151, bh_kv * group, nq, d), randn(152, bh_kv, nk, d), randn(153, bh_kv, nk, d)
    qd = to_dev(q)
    kp, vp, table, canon = paged_window_cache(k, v, batch, H, lens, page, nq, w, layout, seed=page)
    nan_page = int(table[0, -1])
    for b, n in enumerate(lens):   # what the contract lets the call read, and nothing else, is a page of data
        plo, phi = lo_slab(n, nq, w) // page, -(-n // page)
        assert (table[b, :plo] == nan_page).all() and (table[b, phi:] == nan_page).all() and (table[b, plo:phi] != nan_page).all()
    assert np.isnan(canon[0][nan_page]).all()
    gk, gv = gather(canon[0], table, lens, nk), gather(canon[1], table, lens, nk)   # NaN below lo_slab (rounded down to a page: NaN rows of data pages too)
    kd, vd = to_dev(gk), to_dev(gv)
    for s, n in enumerate(slab_lens):
        lo = lo_slab(n, nq, w)
        assert np.isnan(gk[s, :lo]).all() and np.array_equal(gk[s, lo:n], k[s, lo:n])
        kd[s, n:], vd[s, n:] = NAN, NAN
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    slab_lens_d = torch.tensor(slab_lens, dtype=torch.int32, device=dev())
    table_d = torch.from_numpy(table).to(dev())
    for causal in (False, True):
        ref, lse_ref = attention_kvw(q, k, v, slab_lens, causal, 1.0, w)
        for odt in (torch.float32, torch.bfloat16):
            o, lse = fa.forward_paged(qd, kp, vp, table_d, causal, kv_len=nk, seq_lens=lens_d, out_dtype=odt, return_lse=True, window_left=w)
            oc, lsec = fa.forward_kv(qd, kd, vd, causal, kv_len=nk, kv_lens=slab_lens_d, out_dtype=odt, return_lse=True, window_left=w)
            assert err(o, ref, f"paged {odt} causal={causal}") < (TOL_PB2 if odt == torch.float32 else TOL_BF16) and err(lse, lse_ref, "paged lse") < TOL_LSE
            assert ar.bit_equal(o, oc) and ar.bit_equal(lse, lsec), f"paged and contiguous differ ({odt}, causal={causal}): " \
                f"{float((o.float() - oc.float()).abs().max()):.3e}"


# ---- 6. one captured graph, a window that slides ----
def test_one_captured_graph_follows_a_sliding_window():
    batch, group, nq, cap, d, page, w = 2, 4, 1, 512, 128, 16, 199
    q, k, v = randn(161, batch * group, nq, d), randn(162, batch, cap, d), randn(163, batch, cap, d)
    qd = to_dev(q)
    max_pages = cap // page
    pages = batch * max_pages + 1
    order = [int(x) for x in np.random.default_rng(9).permutation(pages)]
    nan_page = order.pop()
    table_h = np.array(order, dtype=np.int32).reshape(batch, max_pages)
    kp = torch.full((pages, page, d), NAN, dtype=torch.bfloat16, device=dev())
    vp = torch.full_like(kp, NAN)
    kdev, vdev = to_dev(k), to_dev(v)
    for b in range(batch):
        for p in range(max_pages):
            kp[int(table_h[b, p])], vp[int(table_h[b, p])] = kdev[b, p * page:(p + 1) * page], vdev[b, p * page:(p + 1) * page]
    table = torch.from_numpy(table_h).to(dev())
    lens_d = torch.zeros(batch, dtype=torch.int32, device=dev())
    out = torch.empty(batch * group, nq, d, dtype=torch.float32, device=dev())
    eager = torch.empty_like(out)
    assert fa.workspace_bytes_paged(batch, 1, group, nq, cap, d, True, out_dtype=torch.float32, window_left=w) == 0   # 263 keys: never split
    fa.forward_paged(qd, kp, vp, table, True, seq_lens=lens_d, out=out, window_left=w)   # library loaded, allocator warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, lse = fa.forward_paged(qd, kp, vp, table, True, seq_lens=lens_d, out=out, return_lse=True, window_left=w)
    crossed_blocks, crossed_pages = set(), set()
    for n in range(250, 331):
        lens = [n, n - 13]
        for b, m in enumerate(lens):   # what has slid out of the window is gone: rows below the edge are NaN, entries below its page name the NaN page
            lo = lo_slab(m, nq, w)
            for p in range(lo // page):
                table[b, p] = nan_page
            p = lo // page
            kp[int(table_h[b, p]), :lo - p * page] = NAN
            vp[int(table_h[b, p]), :lo - p * page] = NAN
            if p:
                kp[[int(x) for x in table_h[b, :p]]] = NAN
                vp[[int(x) for x in table_h[b, :p]]] = NAN
            crossed_blocks.add((b, lo // 64))
            crossed_pages.add((b, lo // page))
        lens_d.copy_(torch.tensor(lens, dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        _, lse_e = fa.forward_paged(qd, kp, vp, table, True, seq_lens=lens_d, out=eager, return_lse=True, window_left=w)
        assert ar.bit_equal(out, eager) and ar.bit_equal(lse, lse_e), f"replay and eager call differ at lengths {lens}"
        if n % 16 == 10 or n == 330:
            ref, lse_ref = attention_kvw(q, k, v, lens, True, 1.0, w)
            assert err(out, ref, f"replay at lengths {lens}") < TOL_PB2 and err(lse, lse_ref, f"replay lse at lengths {lens}") < TOL_LSE
    assert len({c for b, c in crossed_blocks if b == 0}) >= 2 and len({c for b, c in crossed_pages if b == 0}) >= 4


# ---- 7. bounds: everything in one guard-band arena at the minimum alignments ----
def _fill(t, mode, seed):
    if mode == "nan":
        ar.fill_bytes(t, ar.POISON)
    elif mode == "zero":
        t.zero_()
    else:
        t.copy_(torch.randn(t.shape, device=t.device, generator=torch.Generator(device=t.device).manual_seed(seed)).to(t.dtype))


BOUNDS = [
    # (bh_kv, group, nq, nk, d, window_left, kv_lens): S = 1, M = 20 (not a multiple of the 32-row tile)
    (3, 4, 5, 300, 64, 70, [300, 117, 5]),
    # S = 2, M = 45: two row tiles, the second ragged; slab 1 leaves whole shares empty (their partial O is never written)
    (2, 5, 9, 1500, 128, 600, [1500, 333]),
]


@pytest.mark.parametrize("out_f32", [True, False])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", BOUNDS, ids=lambda c: "-".join(map(str, c[:6])))
def test_memory_bounds_and_isolation(case, causal, out_f32):
    bh_kv, group, nq, nk, d, w, lens = case
    L = _cabi_kvw.lib()
    dt = BF16_F32 if out_f32 else BF16
    cap, bhq = nk + 70, bh_kv * group
    S = L.fa_kvw_splits_for(bh_kv, group, nq, nk, d, int(causal), dt, w)
    assert (S > 1) == (w >= 512)
    ws = int(L.fa_kvw_workspace_bytes(bh_kv, group, nq, nk, d, int(causal), dt, w))
    assert (ws > 0) == (S > 1)
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
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    ref, lse_ref = attention_kvw(q, k, v, lens, causal, 1.0, w)
    assert np.isfinite(lse_ref).all()   # every row sees a key: the three runs below must be finite
    runs = []
    for mode, seed in (("zero", 0), ("nan", 0), ("finite", 7)):
        A.fill_input_surroundings("nan" if mode == "zero" else mode, seed)
        for name, src in (("k", k), ("v", v)):
            t = A.view(name)
            _fill(t, mode, seed + 1)                 # rows below lo_slab, rows [len, capacity) of every slab and the neighbour's slab ...
            for s, n in enumerate(lens):
                lo = lo_slab(n, nq, w)
                t[s, lo:n] = to_dev(src[s, lo:n])    # ... around the rows the call may read
        A.fill_output_guards()
        ar.fill_bytes(A.view("o"), ar.POISON)
        ar.fill_bytes(A.view("lse"), ar.POISON)
        if ws:
            ar.fill_bytes(A.view("workspace"), ar.POISON)   # the kernels must read nothing of it they did not write
        rc = L.fa_kvw_forward(A.ptr("q"), A.ptr("k"), A.ptr("v"), A.ptr("o"), A.ptr("lse"), bh_kv, group, nq, nk, cap, lens_d.data_ptr(), d, 1.0,
                              int(causal), dt, w, A.ptr("workspace") if ws else None, ws, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.fa_kvw_last_error()
        torch.cuda.synchronize()
        assert A.guards_intact(), str(A.first_damage())   # stores only to o, lse and the workspace
        runs.append((A.view("o").clone(), A.view("lse").clone()))
        assert err(runs[-1][0], ref, f"o, {mode} surroundings") < (TOL_PB2 if out_f32 else TOL_BF16)
        assert err(runs[-1][1], lse_ref, f"lse, {mode} surroundings") < TOL_LSE
    bad = ar.isolation_failures(*runs)
    assert not bad, "the result depends on memory the call must not read: " + "; ".join(bad)


def test_a_negative_window_is_rejected_before_anything_runs():
    q, k = torch.zeros(1, 1, 64, dtype=torch.bfloat16, device=dev()), torch.zeros(1, 16, 64, dtype=torch.bfloat16, device=dev())
    table = torch.zeros(1, 1, dtype=torch.int32, device=dev())
    with pytest.raises(ValueError):
        fa.forward_kv(q, k, k, True, window_left=-1)
    with pytest.raises(ValueError):
        fa.forward_paged(q, k, k, table, True, window_left=-1)
    with pytest.raises(ValueError):
        fa.workspace_bytes_kv(1, 1, 1, 16, 64, window_left=-1)
    with pytest.raises(ValueError):
        fa.workspace_bytes_paged(1, 1, 1, 1, 16, 64, window_left=-1)
