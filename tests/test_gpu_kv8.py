"""GPU: KV-cache attention over an fp8 (e4m3fn) cache (include/flashattn_amd_kv8.h, fa.forward_kv_fp8 / fa.forward_paged_fp8).

Three kinds of claim:
  bit identity   the kernel dequantises to bf16 exactly and runs the bf16 kernel's instruction sequence, so with v_scale a power of two the
                 result IS v_scale x fa.forward_kv on the dequantised cache at scale' = fp32(scale * k_scale); the LSE for any v_scale; and
                 the paged entry IS the contiguous one on the gathered bytes
  accuracy       against the fp64 reference tests/kv_reference.attention_kv on the logical values k_scale * deq(k8), v_scale * deq(v8).  Bars:
                 tests/test_gpu_kv.py's (2e-4 fp32 output, 1e-4 LSE, 2.5e-2 bf16 output) -- the logical values are N(0, 1)-sized and the
                 arithmetic is the bf16 kernel's
  bounds         the guard-band arena of tests/arena.py: nothing is written outside o / lse / workspace, and nothing the call must not read
                 (rows past a length, a neighbouring slab, unused pages, page tails: NaN codes in one run, finite bytes in the other) changes a bit

Data: K, V ~ N(0, 1) quantised with k_scale = 0.013, v_scale = 0.011 (|x / scale| < 448 up to 5.7 sigma; the codes spread over the whole range),
Q ~ N(0, 1) rounded to bf16.  fp8 tensors are built on the CPU and cross to the device as bytes: no fp8 arithmetic of torch's runs on the GPU.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import flashattention_c_amd as fa
from flashattention_c_amd import _cabi_kv8
from tests import arena as ar
from tests.kv8_reference import dequant, quantize
from tests.kv_reference import attention_kv
from tests.paged_reference import gather
from tests.test_gpu_kv import BOUNDS, PARITY, TOL_BF16, TOL_LSE, TOL_PB2, dev, err, randn, to_dev
from tests.test_gpu_paged import BOUNDS as PAGED_BOUNDS

pytestmark = pytest.mark.gpu

BF16, BF16_F32 = _cabi_kv8.FA_DTYPE_BF16, _cabi_kv8.FA_DTYPE_BF16_OUT_F32
KS, VS = 0.013, 0.011
F8 = torch.float8_e4m3fn
ONE = 0x38          # the code of 1.0: exponent field 7 = the bias, mantissa 0
UNREAD = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def codes(seed, scale, *shape):
    """N(0, 1) quantised at `scale`: the uint8 codes (read-only, shared between tests)"""
    a = quantize(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)), scale).view(torch.uint8).numpy()
    assert not np.isin(a, (0x7F, 0xFF)).any()
    a.setflags(write=False)
    return a


def u8(a):
    """uint8 array (possibly read-only, possibly a slice) -> device byte tensor"""
    return torch.from_numpy(np.array(a, dtype=np.uint8)).to(dev())


def to_dev8(a):
    """uint8 array -> fp8 device tensor, the bytes as they are"""
    return u8(a).view(F8)


def cache8(a, capacity, fill=0xFF):
    """(bh, nk, d) codes -> fp8 device cache (bh, capacity, d) whose rows past nk hold a NaN code: nothing may read them"""
    t = torch.full((a.shape[0], capacity, a.shape[2]), fill, dtype=torch.uint8, device=dev())
    t[:, :a.shape[1]] = u8(a)
    return t.view(F8)


def as_bf16(t8):
    """the bf16 twin of an fp8 device cache, converted on the CPU (exact; a NaN code becomes a bf16 NaN)"""
    return t8.view(torch.uint8).cpu().view(F8).to(torch.bfloat16).to(dev())


def folded(scale, ks):
    return float(np.float32(scale) * np.float32(ks))


IDS = dict(ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else None)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape,splits", PARITY, **IDS)
def test_bit_identity_with_the_bf16_kernel_on_the_dequantised_cache(shape, splits, causal):
    bh_kv, group, nq, nk, d = shape
    assert (_cabi_kv8.lib().fa_kv8_splits_for(bh_kv, group, nq, nk, d, int(causal), BF16) > 1) == splits
    qd = to_dev(randn(61, bh_kv * group, nq, d))
    k8, v8 = cache8(codes(62, KS, bh_kv, nk, d), nk + 70), cache8(codes(63, VS, bh_kv, nk, d), nk + 70)
    kb, vb = as_bf16(k8), as_bf16(v8)
    assert bool(torch.isnan(kb[:, nk:].float()).all())
    for scale in (1.0, 0.125):
        for odt in (torch.float32, torch.bfloat16):
            ref, lse_ref = fa.forward_kv(qd, kb, vb, causal, kv_len=nk, scale=folded(scale, KS), out_dtype=odt, return_lse=True)
            for vs in (1.0, 0.5, VS):
                o, lse = fa.forward_kv_fp8(qd, k8, v8, causal, k_scale=KS, v_scale=vs, kv_len=nk, scale=scale, out_dtype=odt, return_lse=True)
                assert o.dtype == odt
                assert ar.bit_equal(lse, lse_ref), f"LSE differs from the bf16 kernel's (scale {scale}, {odt}, v_scale {vs})"
                if vs != VS:   # a power of two: the product is exact in fp32 and in bf16
                    diff = float((o.float() - vs * ref.float()).abs().max())
                    assert ar.bit_equal(o, (vs * ref).to(odt)), f"O differs from v_scale x the bf16 kernel's (scale {scale}, {odt}, v_scale {vs}): {diff:.3e}"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape,splits", PARITY, **IDS)
def test_general_scales_against_the_fp64_reference(shape, splits, causal):
    bh_kv, group, nq, nk, d = shape
    q, kc, vc = randn(61, bh_kv * group, nq, d), codes(62, KS, bh_kv, nk, d), codes(63, VS, bh_kv, nk, d)
    qd, k8, v8 = to_dev(q), cache8(kc, nk + 70), cache8(vc, nk + 70)
    k, v = KS * dequant(kc), VS * dequant(vc)
    for scale in (1.0, 0.125):
        ref, lse_ref = attention_kv(q, k, v, None, causal, scale)
        o, lse = fa.forward_kv_fp8(qd, k8, v8, causal, k_scale=KS, v_scale=VS, kv_len=nk, scale=scale, out_dtype=torch.float32, return_lse=True)
        assert err(o, ref, f"{shape} f32 out scale {scale}") < TOL_PB2
        assert err(lse, lse_ref, f"{shape} lse scale {scale}") < TOL_LSE
        ob, lseb = fa.forward_kv_fp8(qd, k8, v8, causal, k_scale=KS, v_scale=VS, kv_len=nk, scale=scale, return_lse=True)
        assert ob.dtype == torch.bfloat16
        assert err(ob, ref, f"{shape} bf16 out scale {scale}") < TOL_BF16
        assert err(lseb, lse_ref, f"{shape} lse (bf16 out) scale {scale}") < TOL_LSE
    if causal and nq > nk:   # rows i < nq - nk see nothing: exactly 0, LSE -inf (checked in err())
        assert not ref[:, :nq - nk].any() and not o[:, :nq - nk].any()


@pytest.mark.parametrize("nk,group", [(300, 4), (8192, 8)], ids=["unsplit", "split"])
def test_a_constant_v_comes_out_exactly(nk, group):
    """Every V byte is the code of 1.0: the row sum and every column of O are the same instruction sequence, so the quotient is exactly 1 and
    the one multiplication by v_scale gives fp32(v_scale)."""
    bh_kv, nq, d = 1, 1, 128
    assert (_cabi_kv8.lib().fa_kv8_splits_for(bh_kv, group, nq, nk, d, 0, BF16) > 1) == (nk >= 512)
    qd = to_dev(randn(114, group, nq, d))
    k8 = cache8(codes(112, KS, bh_kv, nk, d), nk + 70)
    v8 = cache8(np.full((bh_kv, nk, d), ONE, dtype=np.uint8), nk + 70)
    assert dequant(np.array([ONE]))[0] == 1.0
    for odt in (torch.float32, torch.bfloat16):
        o1 = fa.forward_kv_fp8(qd, k8, v8, k_scale=KS, v_scale=1.0, kv_len=nk, out_dtype=odt)
        assert bool((o1 == 1.0).all()), f"V = 1 must give O = 1 exactly at v_scale = 1 ({odt})"
    o = fa.forward_kv_fp8(qd, k8, v8, k_scale=KS, v_scale=0.37, kv_len=nk, out_dtype=torch.float32)
    want = float(np.float32(0.37))
    off = int((o != want).sum())
    print(f"v_scale = 0.37, nk = {nk}: {off} of {o.numel()} elements differ from fp32(0.37), max |diff| {float((o - want).abs().max()):.3e}")
    assert off == 0, f"V = 1 must give O = fp32(0.37) exactly at v_scale = 0.37 ({off} elements differ)"


@pytest.mark.parametrize("causal", [False, True])
def test_ragged_lengths_from_device_memory(causal):
    bh_kv, group, nq, nk, d = 4, 4, 2, 2048, 128
    lens = [0, 1, 777, 2048]
    assert _cabi_kv8.lib().fa_kv8_splits_for(bh_kv, group, nq, nk, d, int(causal), BF16) > 1
    q, kc, vc = randn(71, bh_kv * group, nq, d), codes(72, KS, bh_kv, nk, d), codes(73, VS, bh_kv, nk, d)
    k, v = KS * dequant(kc), VS * dequant(vc)
    kd, vd = kc.copy(), vc.copy()
    for s, n in enumerate(lens):   # rows at or beyond a length: NaN codes
        kd[s, n:], vd[s, n:] = 0xFF, 0x7F
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    o, lse = fa.forward_kv_fp8(to_dev(q), to_dev8(kd), to_dev8(vd), causal, k_scale=KS, v_scale=VS, kv_lens=lens_d, out_dtype=torch.float32, return_lse=True)
    for s, n in enumerate(lens):   # each slab equals the reference at its own length, computed on its own
        sl = slice(s * group, (s + 1) * group)
        if n == 0:
            assert not o[sl].any() and bool((lse[sl] == float("-inf")).all())
            continue
        ref, lse_ref = attention_kv(q[sl], k[s:s + 1, :n], v[s:s + 1, :n], None, causal, 1.0)
        assert err(o[sl], ref, f"slab {s} alone") < TOL_PB2 and err(lse[sl], lse_ref, f"slab {s} lse alone") < TOL_LSE
    ob = fa.forward_kv_fp8(to_dev(q), to_dev8(kd), to_dev8(vd), causal, k_scale=KS, v_scale=VS, kv_lens=lens_d)
    assert err(ob, attention_kv(q, k, v, lens, causal, 1.0)[0], "bf16 out") < TOL_BF16


# ---- paged ------------------------------------------------------------------------------------------------------------------------------
class Cache8:
    """A paged fp8 cache holding the codes k8, v8 ((batch * H, nk, d) uint8; sequence b has lens[b] keys).  Layouts as in
    tests/test_gpu_paged.py: "phd" (pages, page, H, d), "hpd" the (pages, H, page, d) form seen through permute(0, 2, 1, 3), "slab"
    (pages, page, d) with the batch * H slabs as sequences of one head.  Unused pages and page tails hold the NaN code 0xFF; table entries at
    or beyond ceil(len / page) hold 2^31 - 1 -- they are never read."""

    def __init__(self, k8, v8, batch, H, lens, page, layout="phd", shuffle=True, seed=0, spare=5, unread=UNREAD):
        if layout == "slab":
            batch, lens, H = batch * H, [n for n in lens for _ in range(H)], 1
        self.batch, self.H, self.page, self.lens = batch, H, page, list(lens)
        nk, d = k8.shape[1], k8.shape[2]
        used = [-(-n // page) for n in lens]
        self.max_pages = -(-nk // page) + 2            # two entries no length reaches
        self.pages = sum(used) + spare
        order = np.random.default_rng(seed).permutation(self.pages) if shuffle else np.arange(self.pages)
        self.free = [int(x) for x in order[sum(used):]]
        table = np.full((batch, self.max_pages), unread, dtype=np.int32)
        kp = np.full((self.pages, page, H, d), 0xFF, dtype=np.uint8)
        vp = np.full((self.pages, page, H, d), 0xFF, dtype=np.uint8)
        self.valid = np.zeros((self.pages, page), dtype=bool)
        at = 0
        for b, n in enumerate(lens):
            for p in range(used[b]):
                phys, rows = int(order[at]), min(page, n - p * page)
                at += 1
                table[b, p] = phys
                self.valid[phys, :rows] = True
                for pool, src in ((kp, k8), (vp, v8)):
                    pool[phys, :rows] = src[b * H:(b + 1) * H, p * page:p * page + rows].transpose(1, 0, 2)
        self.table_host, self.canon = table, (kp, vp)
        self.upload(layout)

    def upload(self, layout="phd"):
        self.table = torch.from_numpy(self.table_host).to(dev())
        kd, vd = (u8(t) for t in self.canon)
        if layout == "hpd":
            kd, vd = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (kd, vd))
            assert not kd.is_contiguous()
        elif layout == "slab":
            kd, vd = kd[:, :, 0].contiguous(), vd[:, :, 0].contiguous()
        self.k, self.v = kd.view(F8), vd.view(F8)

    def gathered(self, nk):
        """the contiguous caches (batch * H, nk, d) the table describes, on the device, and the length of each slab"""
        gk, gv = (gather(t, self.table_host, self.lens, nk) for t in self.canon)
        return to_dev8(gk), to_dev8(gv), torch.tensor([n for n in self.lens for _ in range(self.H)], dtype=torch.int32, device=dev())

    def run(self, qd, causal, nk, **kw):
        return fa.forward_paged_fp8(qd, self.k, self.v, self.table, causal, k_scale=KS, v_scale=VS, kv_len=nk,
                                    seq_lens=torch.tensor(self.lens, dtype=torch.int32, device=dev()), **kw)


@pytest.mark.parametrize("layout", ["phd", "hpd", "slab"])
@pytest.mark.parametrize("page", [16, 64, 256])
@pytest.mark.parametrize("nk,d", [(1000, 64), (4099, 128)])
def test_paged_is_the_contiguous_entry_on_the_gathered_bytes(nk, d, page, layout):
    batch, H, group, nq = 4, 2, 2, 3
    lens = [0, 1, 777, nk]
    assert _cabi_kv8.lib().fa_kv8_splits_for(batch * H, group, nq, nk, d, 1, BF16) > 1
    qd = to_dev(randn(121, batch * H * group, nq, d))
    kc, vc = codes(122, KS, batch * H, nk, d), codes(123, VS, batch * H, nk, d)
    cache = Cache8(kc, vc, batch, H, lens, page, layout, seed=page + len(layout))
    assert cache.k.dim() == (3 if layout == "slab" else 4) and int((cache.table_host == UNREAD).sum()) > 0
    gk, gv, slab_lens = cache.gathered(nk)
    for causal, odt in ((False, torch.float32), (True, torch.float32), (True, torch.bfloat16)):
        o, lse = cache.run(qd, causal, nk, out_dtype=odt, return_lse=True)
        oc, lsec = fa.forward_kv_fp8(qd, gk, gv, causal, k_scale=KS, v_scale=VS, kv_len=nk, kv_lens=slab_lens, out_dtype=odt, return_lse=True)
        assert not bool(torch.isnan(o.float()).any()), "a NaN code was read"
        assert ar.bit_equal(o, oc) and ar.bit_equal(lse, lsec), f"forward_paged_fp8 and forward_kv_fp8 on the gathered bytes differ (causal={causal}, {odt}): " \
            f"{float((o.float() - oc.float()).abs().max()):.3e}"
    group_rows = H * group if layout != "slab" else group   # sequence 0 has no key
    assert not o[:group_rows].any() and bool((lse[:group_rows] == float("-inf")).all())


def test_paged_parity_and_prefix_sharing():
    """Two sequences whose first 512 keys are the same physical pages, with different tails; against the fp64 reference and the contiguous entry."""
    group, nq, d, page, shared, nk = 4, 2, 128, 64, 512, 1024
    lens = [700, 900]
    q = randn(131, 2 * group, nq, d)
    kc, vc = codes(132, KS, 2, nk, d).copy(), codes(133, VS, 2, nk, d).copy()
    kc[1, :shared], vc[1, :shared] = kc[0, :shared], vc[0, :shared]
    cache = Cache8(kc, vc, 2, 1, lens, page, "slab", seed=3)
    own = cache.table_host[1, :shared // page].copy()
    cache.table_host[1, :shared // page] = cache.table_host[0, :shared // page]
    for pool in cache.canon:
        pool[own] = 0xFF                             # sequence 1's own copies of the prefix: now pages nobody names
    cache.upload("slab")
    gk, gv, slab_lens = cache.gathered(nk)
    k, v = KS * dequant(kc), VS * dequant(vc)
    qd = to_dev(q)
    for causal in (False, True):
        o, lse = cache.run(qd, causal, nk, out_dtype=torch.float32, return_lse=True)
        ref, lse_ref = attention_kv(q, k, v, lens, causal, 1.0)
        assert err(o, ref, f"shared prefix, causal={causal}") < TOL_PB2 and err(lse, lse_ref, "shared prefix, lse") < TOL_LSE
        oc, lsec = fa.forward_kv_fp8(qd, gk, gv, causal, k_scale=KS, v_scale=VS, kv_len=nk, kv_lens=slab_lens, out_dtype=torch.float32, return_lse=True)
        assert ar.bit_equal(o, oc) and ar.bit_equal(lse, lsec)


# ---- bounds: everything in one guard-band arena at the minimum alignments -------------------------------------------------------------------
def _surround(t, mode, seed):
    """every byte of an fp8 view: NaN codes, or finite codes from a seed"""
    if mode == "nan":
        ar.fill_bytes(t, ar.POISON)
    else:
        t.view(torch.uint8).copy_(u8(codes(seed, 0.02, *t.shape)))


def _arena(bhq, nq, d, kv_shape, out_f32, ws):
    odt = torch.float32 if out_f32 else torch.bfloat16
    bufs = [ar.Buf("q", "in", torch.bfloat16, (bhq, nq, d), "tensor", d * 2),
            ar.Buf("k", "in", F8, kv_shape, "tensor", d), ar.Buf("v", "in", F8, kv_shape, "tensor", d),
            ar.Buf("o", "out", odt, (bhq, nq, d), "tensor", d * (4 if out_f32 else 2)), ar.Buf("lse", "out", torch.float32, (bhq, nq), "lse", 4)]
    if ws:
        bufs.append(ar.Buf("workspace", "out", torch.uint8, (ws,), "workspace", d * 4))
    return ar.Arena(bufs, dev())


def _poison_outputs(A, ws):
    A.fill_output_guards()
    ar.fill_bytes(A.view("o"), ar.POISON)
    ar.fill_bytes(A.view("lse"), ar.POISON)
    if ws:
        ar.fill_bytes(A.view("workspace"), ar.POISON)   # the kernels must read nothing of it they did not write


def _check_runs(A, runs, ref, lse_ref, out_f32, mode):
    torch.cuda.synchronize()
    assert A.guards_intact(), str(A.first_damage())
    runs.append((A.view("o").clone(), A.view("lse").clone()))
    assert err(runs[-1][0], ref, f"o, {mode} surroundings") < (TOL_PB2 if out_f32 else TOL_BF16)
    assert err(runs[-1][1], lse_ref, f"lse, {mode} surroundings") < TOL_LSE


@pytest.mark.parametrize("causal,out_f32", [(False, True), (True, False)])
@pytest.mark.parametrize("case", BOUNDS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}-{'lens' if c[5] else 'full'}")
def test_memory_bounds_and_isolation(case, causal, out_f32):
    bh_kv, group, nq, nk, d, lens = case
    L = _cabi_kv8.lib()
    dt = BF16_F32 if out_f32 else BF16
    cap, bhq = nk + 70, bh_kv * group
    ws = int(L.fa_kv8_workspace_bytes(bh_kv, group, nq, nk, d, int(causal), dt))
    assert (ws > 0) == (nk >= 512)
    A = _arena(bhq, nq, d, (bh_kv + 1, cap, d), out_f32, ws)   # one K/V slab more than the call covers: the cache of a neighbouring call
    q, kc, vc = randn(91, bhq, nq, d), codes(92, KS, bh_kv, nk, d), codes(93, VS, bh_kv, nk, d)
    A.view("q").copy_(to_dev(q))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev()) if lens else None
    eff = lens if lens else [nk] * bh_kv
    ref, lse_ref = attention_kv(q, KS * dequant(kc), VS * dequant(vc), lens, causal, 1.0)
    runs = []
    for mode, seed in (("nan", 0), ("finite", 7)):
        A.fill_input_surroundings(mode, seed)
        for name, src in (("k", kc), ("v", vc)):
            t = A.view(name)
            _surround(t, mode, seed + 1)               # rows [len, capacity) of every slab and the neighbour's slab ...
            for s, n in enumerate(eff):
                t.view(torch.uint8)[s, :n] = u8(src[s, :n])   # ... around the rows the call may read
        _poison_outputs(A, ws)
        rc = L.fa_kv8_forward(A.ptr("q"), A.ptr("k"), A.ptr("v"), A.ptr("o"), A.ptr("lse"), bh_kv, group, nq, nk, cap,
                              lens_d.data_ptr() if lens else None, d, 1.0, KS, VS, int(causal), dt, A.ptr("workspace") if ws else None, ws,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.fa_kv8_last_error()
        _check_runs(A, runs, ref, lse_ref, out_f32, mode)
    assert ar.bit_equal(runs[0][0], runs[1][0]) and ar.bit_equal(runs[0][1], runs[1][1]), "the result depends on memory the call must not read"


@pytest.mark.parametrize("causal,out_f32", [(False, True), (True, False)])
@pytest.mark.parametrize("case", PAGED_BOUNDS, ids=lambda c: "-".join(map(str, c[:7])) + ("-lens" if c[7] else "-full"))
def test_memory_bounds_and_isolation_paged(case, causal, out_f32):
    batch, H, group, nq, nk, d, page, lens = case
    L = _cabi_kv8.lib()
    dt = BF16_F32 if out_f32 else BF16
    bh_kv, bhq = batch * H, batch * H * group
    ws = int(L.fa_kv8_workspace_bytes(bh_kv, group, nq, nk, d, int(causal), dt))
    assert (ws > 0) == (nk >= 512)
    eff = lens if lens else [nk] * batch
    q, kc, vc = randn(91, bhq, nq, d), codes(92, KS, bh_kv, nk, d), codes(93, VS, bh_kv, nk, d)
    src = Cache8(kc, vc, batch, H, eff, page, "phd", seed=11, spare=7)   # the assignment, the table and the valid rows
    P = src.pages
    A = _arena(bhq, nq, d, (P, page, H, d), out_f32, ws)
    A.view("q").copy_(to_dev(q))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev()) if lens else None
    ref, lse_ref = attention_kv(q, KS * dequant(kc), VS * dequant(vc), [n for n in eff for _ in range(H)], causal, 1.0)
    valid = torch.from_numpy(src.valid).to(dev())                       # what the call may read: the same rows in both pools
    runs = []
    for mode, seed in (("nan", 0), ("finite", 7)):
        A.fill_input_surroundings(mode, seed)
        for name, pool in (("k", src.k), ("v", src.v)):
            t = A.view(name)
            _surround(t, mode, seed + 1)                                  # unused pages and the tails of last pages ...
            t.view(torch.uint8)[valid] = pool.view(torch.uint8)[valid]   # ... around the rows the call may read
        table = src.table_host.copy()
        for b, n in enumerate(eff):                                    # entries past the length: another page that exists, per mode
            table[b, -(-n // page):] = src.free[(b + (mode == "finite")) % len(src.free)]
        table_d = torch.from_numpy(table).to(dev())
        _poison_outputs(A, ws)
        cache = _cabi_kv8.FaPagedCache(A.ptr("k"), A.ptr("v"), P, page, page * H * d, H * d, d, table_d.data_ptr(), table.shape[1],
                                       lens_d.data_ptr() if lens else None)
        rc = L.fa_kv8_paged_forward(A.ptr("q"), ctypes.byref(cache), A.ptr("o"), A.ptr("lse"), batch, H, group, nq, nk, d, 1.0, KS, VS, int(causal), dt,
                                    A.ptr("workspace") if ws else None, ws, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.fa_kv8_last_error()
        _check_runs(A, runs, ref, lse_ref, out_f32, mode)
    assert ar.bit_equal(runs[0][0], runs[1][0]) and ar.bit_equal(runs[0][1], runs[1][1]), "the result depends on memory the call must not read"


def test_one_captured_graph_follows_a_paged_fp8_cache_that_grows_and_moves():
    batch, group, nq, cap, d, page = 2, 4, 1, 1024, 128, 16
    assert _cabi_kv8.lib().fa_kv8_splits_for(batch, group, nq, cap, d, 1, BF16_F32) > 1
    q, kc, vc = randn(101, batch * group, nq, d), codes(102, KS, batch, cap, d), codes(103, VS, batch, cap, d)
    k, v = KS * dequant(kc), VS * dequant(vc)
    qd, kdev, vdev = to_dev(q), u8(kc), u8(vc)
    max_pages = cap // page
    pages = 3 * max_pages + 1
    kp = torch.full((pages, page, d), 0xFF, dtype=torch.uint8, device=dev())   # the pools as bytes; the entry sees them as fp8
    vp = torch.full_like(kp, 0xFF)
    free = [int(x) for x in np.random.default_rng(5).permutation(pages)]
    nan_page = free.pop()                                   # stays 0xFF: what every entry past a length names
    table = torch.full((batch, max_pages), nan_page, dtype=torch.int32, device=dev())
    lens_d = torch.zeros(batch, dtype=torch.int32, device=dev())
    out = torch.empty(batch * group, nq, d, dtype=torch.float32, device=dev())
    ws = torch.empty(fa.workspace_bytes_paged(batch, 1, group, nq, cap, d, True, out_dtype=torch.float32), dtype=torch.uint8, device=dev())
    assert ws.numel() > 0
    kw = dict(k_scale=KS, v_scale=VS, seq_lens=lens_d, out=out, workspace=ws)
    fa.forward_paged_fp8(qd, kp.view(F8), vp.view(F8), table, True, **kw)   # library loaded, allocator warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, lse = fa.forward_paged_fp8(qd, kp.view(F8), vp.view(F8), table, True, return_lse=True, **kw)
    have, owned = [0, 0], [[], []]
    for step, lens in enumerate(([100, 300], [101, 640], [1024, 641])):
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
        if step:   # sequence 0 moves to other physical pages: copy the data, rewrite the table in place, NaN the old pages
            new = [free.pop() for _ in owned[0]]
            kp[new], vp[new] = kp[owned[0]], vp[owned[0]]
            table[0, :len(new)] = torch.tensor(new, dtype=torch.int32, device=dev())
            kp[owned[0]] = 0xFF
            vp[owned[0]] = 0xFF
            owned[0] = new
        g.replay()
        torch.cuda.synchronize()
        ref, lse_ref = attention_kv(q, k, v, lens, True, 1.0)
        assert err(out, ref, f"replay {step} at lengths {lens}") < TOL_PB2 and err(lse, lse_ref, f"replay {step} lse") < TOL_LSE


def test_the_python_entries_take_fp8_tensors_as_they_are_or_raise():
    q = to_dev(randn(151, 4, 1, 64))
    k8 = torch.zeros((1, 32, 64), dtype=torch.uint8, device=dev())
    with pytest.raises(TypeError, match=r"view\(torch.float8_e4m3fn\)"):
        fa.forward_kv_fp8(q, k8, k8)
    with pytest.raises(TypeError, match="float8_e4m3fn"):
        fa.forward_kv_fp8(q, k8.to(torch.bfloat16), k8.to(torch.bfloat16))
    table = torch.zeros((1, 2), dtype=torch.int32, device=dev())
    pool = torch.zeros((3, 16, 128), dtype=torch.uint8, device=dev())
    with pytest.raises(TypeError, match=r"view\(torch.float8_e4m3fn\)"):
        fa.forward_paged_fp8(q, pool[:, :, :64], pool[:, :, :64], table)
    odd = torch.zeros((3, 16, 72), dtype=torch.uint8, device=dev()).view(F8)
    with pytest.raises(ValueError, match="multiples of 16"):
        fa.forward_paged_fp8(q, odd[:, :, :64], odd[:, :, :64], table)
    with pytest.raises(fa._cabi.FlashAttnError, match="k_scale"):
        fa.forward_kv_fp8(q, k8.view(F8), k8.view(F8), k_scale=0.0)
    p8 = pool.view(F8)
    o = fa.forward_paged_fp8(q, p8[:, :, :64], p8[:, :, 64:], table, kv_len=20)   # a column slice: row stride 128, no copy; V = 0
    assert o.shape == q.shape and not o.any()
