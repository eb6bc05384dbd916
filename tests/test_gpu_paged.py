"""GPU: paged KV-cache attention (include/flashattn_amd_paged.h, fa.forward_paged) against the fp64 reference tests/kv_reference.py on the
cache tests/paged_reference.gather rebuilds, and bit for bit against fa.forward_kv on that cache.

Tolerances are tests/test_gpu_kv.py's, on its data family (seeded N(0, 1) rounded to bf16, scale 1.0 and 0.125): the arithmetic is the same.
    fp32 output  2e-4      LSE  1e-4      bf16 output  2.5e-2

Every pool is built so that a wrong read shows as a NaN in the result and never as a fault: more pages than are used, a random page
assignment, unused pages NaN, the tail of every last page NaN, every table entry at or beyond ceil(len / page) the index of a NaN page that
exists.  No index is ever out of range.
"""
import ctypes

import numpy as np
import pytest
import torch

import flashattention_c_amd as fa
from flashattention_c_amd import _cabi_paged
from tests import arena as ar
from tests.kv_reference import attention_kv
from tests.paged_reference import gather
from tests.test_gpu_kv import TOL_BF16, TOL_LSE, TOL_PB2, dev, err, randn, to_dev

pytestmark = pytest.mark.gpu

BF16, BF16_F32 = _cabi_paged.FA_DTYPE_BF16, _cabi_paged.FA_DTYPE_BF16_OUT_F32
NAN = float("nan")


class Cache:
    """A paged cache holding k, v ((batch * H, nk, d) arrays; sequence b has lens[b] keys).  layout: "phd" (pages, page, H, d), "hpd" the
    (pages, H, page, d) form seen through permute(0, 2, 1, 3), "slab" (pages, page, d) -- one K/V head per sequence, so the batch * H slabs
    become batch * H sequences with a table row each."""

    def __init__(self, k, v, batch, H, lens, page, layout="phd", shuffle=True, seed=0, spare=5, max_pages=None):
        if layout == "slab":
            batch, lens, H = batch * H, [n for n in lens for _ in range(H)], 1
        self.batch, self.H, self.page, self.lens = batch, H, page, list(lens)
        nk, d = k.shape[1], k.shape[2]
        used = [-(-n // page) for n in lens]
        self.max_pages = max_pages or -(-nk // page) + 2            # two entries no length reaches
        self.pages = sum(used) + spare
        rng = np.random.default_rng(seed)
        order = rng.permutation(self.pages) if shuffle else np.arange(self.pages)
        self.free = [int(x) for x in order[sum(used):]]               # NaN pages that exist
        table = np.empty((batch, self.max_pages), dtype=np.int32)
        kp = torch.full((self.pages, page, H, d), NAN)
        vp = torch.full((self.pages, page, H, d), NAN)
        at = 0
        for b, n in enumerate(lens):
            table[b] = [self.free[(b + i) % len(self.free)] for i in range(self.max_pages)]
            for p in range(used[b]):
                phys, rows = int(order[at]), min(page, n - p * page)
                at += 1
                table[b, p] = phys
                for pool, src in ((kp, k), (vp, v)):
                    pool[phys, :rows] = torch.from_numpy(np.ascontiguousarray(src[b * H:(b + 1) * H, p * page:p * page + rows])).float().transpose(0, 1)
        self.table_host = table
        self.table = torch.from_numpy(table).to(dev())
        self.canon = (kp.numpy().astype(np.float64), vp.numpy().astype(np.float64))
        kd, vd = kp.to(torch.bfloat16).to(dev()), vp.to(torch.bfloat16).to(dev())
        if layout == "hpd":
            kd, vd = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (kd, vd))
            assert not kd.is_contiguous()
        elif layout == "slab":
            kd, vd = kd[:, :, 0].contiguous(), vd[:, :, 0].contiguous()
        self.k, self.v = kd, vd

    def gathered(self, nk):
        return gather(self.canon[0], self.table_host, self.lens, nk), gather(self.canon[1], self.table_host, self.lens, nk)

    def run(self, qd, causal, nk, lens_d=None, **kw):
        return fa.forward_paged(qd, self.k, self.v, self.table, causal, kv_len=nk, seq_lens=lens_d, **kw)


def check_all(q, k, v, qd, cache, nk, causal, lens=None, lens_d=None, what=""):
    """both scales, both output dtypes, output and LSE against the fp64 reference"""
    for scale in (1.0, 0.125):
        ref, lse_ref = attention_kv(q, k, v, lens, causal, scale)
        o, lse = cache.run(qd, causal, nk, lens_d, scale=scale, out_dtype=torch.float32, return_lse=True)
        assert err(o, ref, f"{what} f32 out scale {scale}") < TOL_PB2
        assert err(lse, lse_ref, f"{what} lse scale {scale}") < TOL_LSE
        ob, lseb = cache.run(qd, causal, nk, lens_d, scale=scale, return_lse=True)
        assert ob.dtype == torch.bfloat16
        assert err(ob, ref, f"{what} bf16 out scale {scale}") < TOL_BF16
        assert err(lseb, lse_ref, f"{what} lse (bf16 out) scale {scale}") < TOL_LSE
    return ref


# (batch, heads_kv, group, nq, nk, d, page), does the plan split?
PARITY = [
    ((2, 1, 1, 1, 1, 64, 16), False), ((3, 2, 4, 1, 31, 64, 16), False), ((2, 1, 8, 1, 257, 128, 64), False),
    ((2, 2, 4, 5, 1000, 64, 16), True),          # split, four pages per block
    ((1, 1, 8, 16, 4099, 128, 256), True),       # split, ragged last share
    ((1, 1, 4, 33, 700, 64, 32), True),          # several row tiles
    ((2, 1, 1, 40, 24, 128, 16), False),         # causal rows without keys
]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape,splits", PARITY, ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else None)
def test_parity_and_agreement_with_the_contiguous_cache(shape, splits, causal):
    batch, H, group, nq, nk, d, page = shape
    S = _cabi_paged.lib().fa_paged_splits_for(batch, H, group, nq, nk, d, int(causal), BF16)
    assert (S > 1) == splits and 1 <= S <= 64, S
    bh_kv = batch * H
    q, k, v = randn(61, bh_kv * group, nq, d), randn(62, bh_kv, nk, d), randn(63, bh_kv, nk, d)
    qd = to_dev(q)
    cache = Cache(k, v, batch, H, [nk] * batch, page, "phd" if H > 1 else "slab")
    gk, gv = cache.gathered(nk)
    assert np.array_equal(gk, k) and np.array_equal(gv, v)       # the reference is attention_kv on the gathered cache
    ref = check_all(q, gk, gv, qd, cache, nk, causal, what=str(shape))
    # the same plan and the same operation sequence as the contiguous-cache forward: the same bits
    ident = Cache(k, v, batch, H, [nk] * batch, page, "phd" if H > 1 else "slab", shuffle=False)
    assert np.array_equal(ident.table_host[:, :-(-nk // page)], np.arange(bh_kv // H * -(-nk // page)).reshape(batch, -1))
    kd, vd = to_dev(gk), to_dev(gv)
    for odt in (torch.float32, torch.bfloat16):
        o, lse = cache.run(qd, causal, nk, out_dtype=odt, return_lse=True)
        oi, lsei = ident.run(qd, causal, nk, out_dtype=odt, return_lse=True)
        assert ar.bit_equal(o, oi) and ar.bit_equal(lse, lsei), "an identity table and a shuffled table differ"
        oc, lsec = fa.forward_kv(qd, kd, vd, causal, kv_len=nk, out_dtype=odt, return_lse=True)
        assert ar.bit_equal(o, oc) and ar.bit_equal(lse, lsec), f"forward_paged and forward_kv on the gathered cache differ ({odt}): " \
            f"{float((o.float() - oc.float()).abs().max()):.3e}"
    if causal and nq > nk:   # rows i < nq - nk see nothing: exactly 0 (checked bit for bit), LSE -inf (checked in err())
        assert not ref[:, :nq - nk].any()
        o = cache.run(qd, True, nk, out_dtype=torch.float32)
        assert not o[:, :nq - nk].any()


@pytest.mark.parametrize("shape", [(2, 2, 4, 3, 1000, 64, 16), (2, 2, 4, 3, 200, 128, 32)], ids=lambda s: "-".join(map(str, s)))
def test_three_layouts_give_the_same_bits(shape):
    batch, H, group, nq, nk, d, page = shape
    assert (_cabi_paged.lib().fa_paged_splits_for(batch, H, group, nq, nk, d, 1, BF16) > 1) == (nk >= 512)
    bh_kv = batch * H
    q, k, v = randn(121, bh_kv * group, nq, d), randn(122, bh_kv, nk, d), randn(123, bh_kv, nk, d)
    qd = to_dev(q)
    lens = [nk, nk - 37]
    ref, lse_ref = attention_kv(q, k, v, [n for n in lens for _ in range(H)], True, 1.0)
    got = {}
    for layout in ("phd", "hpd", "slab"):
        cache = Cache(k, v, batch, H, lens, page, layout, seed=len(layout))
        lens_d = torch.tensor(cache.lens, dtype=torch.int32, device=dev())
        assert cache.k.dim() == (3 if layout == "slab" else 4)
        got[layout] = cache.run(qd, True, nk, lens_d, out_dtype=torch.float32, return_lse=True)
        assert err(got[layout][0], ref, f"{layout} o") < TOL_PB2 and err(got[layout][1], lse_ref, f"{layout} lse") < TOL_LSE
    for layout in ("hpd", "slab"):
        assert ar.bit_equal(got["phd"][0], got[layout][0]) and ar.bit_equal(got["phd"][1], got[layout][1]), layout


@pytest.mark.parametrize("page", [16, 256])
@pytest.mark.parametrize("causal", [False, True])
def test_lengths_from_device_memory(causal, page):
    batch, H, group, nq, nk, d = 4, 1, 4, 2, 2048, 128
    lens = [0, 1, 777, 2048]
    assert _cabi_paged.lib().fa_paged_splits_for(batch, H, group, nq, nk, d, int(causal), BF16) > 1
    q, k, v = randn(71, batch * group, nq, d), randn(72, batch, nk, d), randn(73, batch, nk, d)
    qd = to_dev(q)
    cache = Cache(k, v, batch, H, lens, page, "slab", seed=page)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    o, lse = cache.run(qd, causal, nk, lens_d, out_dtype=torch.float32, return_lse=True)
    for s, n in enumerate(lens):   # each sequence equals the reference at its own length, computed on its own
        sl = slice(s * group, (s + 1) * group)
        if n == 0:
            assert not o[sl].any() and bool((lse[sl] == float("-inf")).all())
            continue
        ref, lse_ref = attention_kv(q[sl], k[s:s + 1, :n], v[s:s + 1, :n], None, causal, 1.0)
        assert err(o[sl], ref, f"sequence {s} alone") < TOL_PB2 and err(lse[sl], lse_ref, f"sequence {s} lse alone") < TOL_LSE
    ob = cache.run(qd, causal, nk, lens_d)
    assert err(ob, attention_kv(q, k, v, lens, causal, 1.0)[0], "bf16 out") < TOL_BF16


def test_prefix_sharing():
    """Two sequences whose first 512 keys are the same physical pages, with different tails."""
    group, nq, d, page, shared = 4, 2, 128, 64, 512
    lens = [700, 900]
    nk = 1024
    assert _cabi_paged.lib().fa_paged_splits_for(2, 1, group, nq, nk, d, 1, BF16) > 1
    q, k, v = randn(131, 2 * group, nq, d), randn(132, 2, nk, d), randn(133, 2, nk, d)
    k[1, :shared], v[1, :shared] = k[0, :shared], v[0, :shared]
    cache = Cache(k, v, 2, 1, lens, page, "slab", seed=3)
    own = cache.table_host[1, :shared // page].copy()
    cache.table_host[1, :shared // page] = cache.table_host[0, :shared // page]
    cache.table.copy_(torch.from_numpy(cache.table_host))
    cache.k[own.tolist()] = NAN                      # sequence 1's own copies of the prefix: now pages nobody names
    cache.v[own.tolist()] = NAN
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    for causal in (False, True):
        o, lse = cache.run(to_dev(q), causal, nk, lens_d, out_dtype=torch.float32, return_lse=True)
        for s, n in enumerate(lens):
            sl = slice(s * group, (s + 1) * group)
            ref, lse_ref = attention_kv(q[sl], k[s:s + 1, :n], v[s:s + 1, :n], None, causal, 1.0)
            assert err(o[sl], ref, f"sequence {s}, causal={causal}") < TOL_PB2 and err(lse[sl], lse_ref, f"sequence {s} lse") < TOL_LSE


# ---- bounds: q, both pools, o, lse and the workspace in one guard-band arena at the minimum alignments --------------------------------
def _fill(t, mode, seed):
    if mode == "nan":
        ar.fill_bytes(t, ar.POISON)
    else:
        t.copy_(torch.randn(t.shape, device=t.device, generator=torch.Generator(device=t.device).manual_seed(seed)).to(t.dtype))


BOUNDS = [
    # (batch, heads_kv, group, nq, nk, d, page, seq_lens): S = 1, M = 20 (not a multiple of the 32-row tile)
    (3, 1, 4, 5, 300, 64, 16, [300, 17, 0]),
    (3, 1, 4, 5, 300, 64, 16, None),
    # S = 4, M = 45: two row tiles, the second ragged; sequence 1 leaves whole shares empty; two heads interleaved in every page
    (2, 2, 5, 9, 1100, 128, 32, [1100, 333]),
    (2, 2, 5, 9, 1100, 128, 32, None),
]


@pytest.mark.parametrize("out_f32", [True, False])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", BOUNDS, ids=lambda c: "-".join(map(str, c[:7])) + ("-lens" if c[7] else "-full"))
def test_memory_bounds_and_isolation(case, causal, out_f32):
    batch, H, group, nq, nk, d, page, lens = case
    L = _cabi_paged.lib()
    dt = BF16_F32 if out_f32 else BF16
    bh_kv, bhq = batch * H, batch * H * group
    S = L.fa_paged_splits_for(batch, H, group, nq, nk, d, int(causal), dt)
    assert (S > 1) == (nk >= 512)
    ws = int(L.fa_paged_workspace_bytes(batch, H, group, nq, nk, d, int(causal), dt))
    odt = torch.float32 if out_f32 else torch.bfloat16
    eff = lens if lens else [nk] * batch
    q, k, v = randn(91, bhq, nq, d), randn(92, bh_kv, nk, d), randn(93, bh_kv, nk, d)
    src = Cache(k, v, batch, H, eff, page, "phd", seed=11, spare=7)   # the assignment, the table and the valid rows
    P = src.pages
    bufs = [ar.Buf("q", "in", torch.bfloat16, (bhq, nq, d), "tensor", d * 2),
            ar.Buf("k", "in", torch.bfloat16, (P, page, H, d), "tensor", d * 2), ar.Buf("v", "in", torch.bfloat16, (P, page, H, d), "tensor", d * 2),
            ar.Buf("o", "out", odt, (bhq, nq, d), "tensor", d * (4 if out_f32 else 2)), ar.Buf("lse", "out", torch.float32, (bhq, nq), "lse", 4)]
    if ws:
        bufs.append(ar.Buf("workspace", "out", torch.uint8, (ws,), "workspace", d * 4))
    A = ar.Arena(bufs, dev())
    A.view("q").copy_(to_dev(q))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev()) if lens else None
    ref, lse_ref = attention_kv(q, k, v, [n for n in eff for _ in range(H)], causal, 1.0)
    valid = ~torch.isnan(src.k.float())                                # what the call may read: the same rows in both pools
    runs = []
    for mode, seed in (("nan", 0), ("finite", 7)):
        A.fill_input_surroundings(mode, seed)
        for name, pool in (("k", src.k), ("v", src.v)):
            t = A.view(name)
            _fill(t, mode, seed + 1)                                   # unused pages and the tails of last pages ...
            t[valid] = pool[valid]                                     # ... around the rows the call may read
        table = src.table_host.copy()
        for b, n in enumerate(eff):                                    # entries past the length: another page that exists, per mode
            table[b, -(-n // page):] = src.free[(b + (mode == "finite")) % len(src.free)]
        table_d = torch.from_numpy(table).to(dev())
        A.fill_output_guards()
        ar.fill_bytes(A.view("o"), ar.POISON)
        ar.fill_bytes(A.view("lse"), ar.POISON)
        if ws:
            ar.fill_bytes(A.view("workspace"), ar.POISON)              # the kernels must read nothing of it they did not write
        cache = _cabi_paged.FaPagedCache(A.ptr("k"), A.ptr("v"), P, page, page * H * d, H * d, d, table_d.data_ptr(), table.shape[1],
                                         lens_d.data_ptr() if lens else None)
        rc = L.fa_paged_forward(A.ptr("q"), ctypes.byref(cache), A.ptr("o"), A.ptr("lse"), batch, H, group, nq, nk, d, 1.0, int(causal), dt,
                                A.ptr("workspace") if ws else None, ws, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.fa_paged_last_error()
        torch.cuda.synchronize()
        assert A.guards_intact(), str(A.first_damage())
        runs.append((A.view("o").clone(), A.view("lse").clone()))
        assert err(runs[-1][0], ref, f"o, {mode} surroundings") < (TOL_PB2 if out_f32 else TOL_BF16)
        assert err(runs[-1][1], lse_ref, f"lse, {mode} surroundings") < TOL_LSE
    assert ar.bit_equal(runs[0][0], runs[1][0]) and ar.bit_equal(runs[0][1], runs[1][1]), "the result depends on memory the call must not read"


def test_one_captured_graph_follows_a_cache_that_grows_and_moves():
    batch, group, nq, cap, d, page = 2, 4, 1, 1024, 128, 16
    assert _cabi_paged.lib().fa_paged_splits_for(batch, 1, group, nq, cap, d, 1, BF16_F32) > 1
    q, k, v = randn(101, batch * group, nq, d), randn(102, batch, cap, d), randn(103, batch, cap, d)
    qd, kdev, vdev = to_dev(q), to_dev(k), to_dev(v)
    max_pages = cap // page
    pages = 3 * max_pages + 1
    kp = torch.full((pages, page, d), NAN, dtype=torch.bfloat16, device=dev())
    vp = torch.full_like(kp, NAN)
    free = [int(x) for x in np.random.default_rng(5).permutation(pages)]
    nan_page = free.pop()                                   # stays NaN: what every entry past a length names
    table = torch.full((batch, max_pages), nan_page, dtype=torch.int32, device=dev())
    lens_d = torch.zeros(batch, dtype=torch.int32, device=dev())
    out = torch.empty(batch * group, nq, d, dtype=torch.float32, device=dev())
    ws = torch.empty(fa.workspace_bytes_paged(batch, 1, group, nq, cap, d, True, out_dtype=torch.float32), dtype=torch.uint8, device=dev())
    assert ws.numel() > 0
    fa.forward_paged(qd, kp, vp, table, True, seq_lens=lens_d, out=out, workspace=ws)   # library loaded, allocator warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, lse = fa.forward_paged(qd, kp, vp, table, True, seq_lens=lens_d, out=out, workspace=ws, return_lse=True)
    have, owned = [0, 0], [[], []]

    def replay_and_check(lens, what):
        g.replay()
        torch.cuda.synchronize()
        ref, lse_ref = attention_kv(q, k, v, lens, True, 1.0)
        assert err(out, ref, f"{what} at lengths {lens}") < TOL_PB2 and err(lse, lse_ref, f"{what} lse at lengths {lens}") < TOL_LSE

    for lens in ([100, 300], [101, 640], [1024, 641]):
        for s, n in enumerate(lens):   # the new rows enter the cache page by page, the table and the lengths follow
            while len(owned[s]) * page < n:
                owned[s].append(free.pop())
                table[s, len(owned[s]) - 1] = owned[s][-1]
            for j0 in range(have[s] // page * page, n, page):
                lo, hi = max(j0, have[s]), min(j0 + page, n)
                kp[owned[s][j0 // page], lo - j0:hi - j0] = kdev[s, lo:hi]
                vp[owned[s][j0 // page], lo - j0:hi - j0] = vdev[s, lo:hi]
        have = lens
        lens_d.copy_(torch.tensor(lens, dtype=torch.int32))
        replay_and_check(lens, "replay")
        # sequence 0 moves to other physical pages: copy the data, rewrite the table in place, NaN the old pages
        new = [free.pop() for _ in owned[0]]
        kp[new], vp[new] = kp[owned[0]], vp[owned[0]]
        table[0, :len(new)] = torch.tensor(new, dtype=torch.int32, device=dev())
        kp[owned[0]] = NAN
        vp[owned[0]] = NAN
        owned[0] = new
        replay_and_check(lens, "replay after the move")


def test_a_pool_beyond_four_gigabytes():
    """65 600 pages of 64 KiB per pool: the page base must be formed in 64 bits.  The pools are allocated and not filled."""
    d, page, pages, group, nk = 128, 256, 65600, 8, 1024
    assert pages * page * d * 2 > 1 << 32
    q, k, v = randn(141, group, 1, d), randn(142, 1, nk, d), randn(143, 1, nk, d)
    kp = torch.empty((pages, page, d), dtype=torch.bfloat16, device=dev())
    vp = torch.empty_like(kp)
    where = [65537, 0, 65599, 65536]
    for p, phys in enumerate(where):
        kp[phys] = to_dev(k[0, p * page:(p + 1) * page])
        vp[phys] = to_dev(v[0, p * page:(p + 1) * page])
    table = torch.tensor([where], dtype=torch.int32, device=dev())
    ref, lse_ref = attention_kv(q, k, v, None, False, 1.0)
    o, lse = fa.forward_paged(to_dev(q), kp, vp, table, out_dtype=torch.float32, return_lse=True)
    assert err(o, ref, "pool beyond 2^32 bytes") < TOL_PB2 and err(lse, lse_ref, "pool beyond 2^32 bytes, lse") < TOL_LSE


@pytest.mark.parametrize("nk,page", [(8192, 64), (300, 16)])
def test_a_constant_v_comes_out_exactly(nk, page):
    batch, H, group, nq, d = 1, 2, 4, 1, 128
    assert (_cabi_paged.lib().fa_paged_splits_for(batch, H, group, nq, nk, d, 0, BF16) > 1) == (nk >= 512)
    q, k = randn(114, batch * H * group, nq, d), randn(112, batch * H, nk, d)
    cache = Cache(k, np.ones_like(k), batch, H, [nk - 5], page, "phd")     # V = 1 on every used row, NaN everywhere else
    lens_d = torch.tensor([nk - 5], dtype=torch.int32, device=dev())
    for odt in (torch.float32, torch.bfloat16):
        o1 = cache.run(to_dev(q), False, nk, lens_d, out_dtype=odt)
        assert bool((o1 == 1.0).all()), f"V = 1 must give O = 1 exactly ({odt})"


def test_forward_paged_takes_pools_as_they_are_or_raises():
    """Strides come from the tensors: a pool is never copied, so a layout the kernel cannot address is an error."""
    q = to_dev(randn(151, 4, 1, 64))
    table = torch.zeros((1, 2), dtype=torch.int32, device=dev())
    wide = torch.zeros((3, 16, 128), dtype=torch.bfloat16, device=dev())
    with pytest.raises(ValueError, match="last stride"):
        fa.forward_paged(q, wide[:, :, ::2], wide[:, :, ::2], table)
    odd = torch.zeros((3, 16, 68), dtype=torch.bfloat16, device=dev())
    with pytest.raises(ValueError, match="multiples of 8"):
        fa.forward_paged(q, odd[:, :, :64], odd[:, :, :64], table)
    with pytest.raises(ValueError, match="block_table"):
        fa.forward_paged(q, wide[:, :, :64], wide[:, :, :64], table.long())
    with pytest.raises(ValueError, match="identical shapes and strides"):
        fa.forward_paged(q, wide[:, :, :64], wide[:, :, :64].contiguous(), table)
    o = fa.forward_paged(q, wide[:, :, :64], wide[:, :, 64:], table, kv_len=20)   # a column slice: row stride 128, no copy; V = 0
    assert o.shape == q.shape and not o.any()
