"""GPU (-m gpu): what a numeric comparison of the output tensor cannot see.

  1. stores outside o / lse / workspace     every buffer sits in a guard-band arena (tests/arena.py: >= 1 MiB of pattern before and after each,
                                            buffers at the minimum alignment of include/flashattn_amd.h); the guards must survive the forward
  2. loads outside a slab's own rows        0xFF bytes (NaN in fp32 and bf16) in the guards of q, k, v and in the neighbouring slabs (run A)
                                            against finite data of another seed there (run B): slab 1's o and lse must be finite and
                                            bit-identical in A, B and a clean run -- P = 0 times a NaN is a NaN
  3. the 32-bit boundaries                  tensors beyond 2^31 elements / 2^32 bytes in one launch of short rows

for every kernel family, every shipped tiling, the key-split launches (workspace of exactly fa_workspace_bytes, and NULL) and the packed
llm.c entry.  Calls go through fa_forward_ws / fa_forward_packed_qkv with raw pointers, so lse and the workspace are the test's buffers too.
References: the rung-0 kernel on plain dense copies (itself pinned to the fp64 oracle here and in tests/test_gpu_parity.py).  Tolerances are
the ones the path already has in tests/test_gpu_parity.py / test_gpu_sweeps.py / test_gpu_head_dims.py; the PATHS table says which.
Non-finite values INSIDE a slab at causally masked positions are out of scope (0 * NaN = NaN in any matrix-core formulation).
"""
import ctypes
import os
import zlib
from dataclasses import dataclass
from typing import Callable, Tuple

import numpy as np
import pytest
import torch

import flashattention_c_amd as fa
from flashattention_c_amd import _cabi
from flashattention_c_amd.flash import _kernel_id
from oracle import oracle as orc
from tests import arena as ar
from tests import test_gpu_sweeps as sweeps
from tests.test_gpu_head_dims import TOL as TOL_EXACT          # 1e-4: fp32 arithmetic against rung 0 / the oracle
from tests.test_gpu_parity import TOL_F32, TOL_PB2, bf16_tol

pytestmark = pytest.mark.gpu

F32, BF16, BF16_F32 = _cabi.FA_DTYPE_F32, _cabi.FA_DTYPE_BF16, _cabi.FA_DTYPE_BF16_OUT_F32
IN_DTYPE = {F32: torch.float32, BF16: torch.bfloat16, BF16_F32: torch.bfloat16}
OUT_DTYPE = {F32: torch.float32, BF16: torch.bfloat16, BF16_F32: torch.float32}
DT_NAME = {F32: "fp32", BF16: "bf16", BF16_F32: "bf16->fp32"}
SHORT = tuple((3, n) for n in (1, 31, 33, 127, 129, 255, 257, 700))    # where a tile overreaches furthest relative to the slab
BOTH, FULL, CAUSAL = (False, True), (False,), (True,)

OBSERVED = []


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _dump_observed():
    yield
    out = os.environ.get("FA_OBSERVED_DIR", "")      # where a run wants its observation files (one line per check); unset: none is written
    if out and os.path.isdir(out):
        with open(os.path.join(out, "bounds_observed.txt"), "w") as f:
            for line in OBSERVED:
                f.write(line + "\n")


def observe(check, path_id, shape, causal, err, tol, intact):
    OBSERVED.append(f"{check:9s} {path_id:34s} shape {'x'.join(map(str, shape)):16s} causal={int(causal)}  worst err {err:.3e}  tol {tol:.1e}  "
                    f"guards intact {'n/a (no arena at this size)' if intact is None else 'yes' if intact else 'NO'}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the paths
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Path:
    dtype: int
    kernel: str                                   # as flash._kernel_id takes it
    d: int
    tol: Callable[[bool, int, float], float]      # (causal, n, max|ref|) -> bound on max|o - rung 0|
    tol_lse: float
    scale: float = 1.0
    causal: Tuple[bool, ...] = BOTH
    shapes: Tuple[Tuple[int, int], ...] = SHORT   # (bh, n)
    keysplit: bool = False                        # every shape must report fa_workspace_bytes > 0

    @property
    def id(self):
        ks = "-keyshares" if self.keysplit else ""
        return f"{DT_NAME[self.dtype]}-{self.kernel}-d{self.d}{ks}" + ("" if self.causal == BOTH else "-causal" if self.causal == CAUSAL else "-full")


def const(t):
    return lambda causal, n, ref_max: t


def bf16_p(scale, out_f32):          # the bf16-P kernels: bf16_tol of tests/test_gpu_parity.py
    return lambda causal, n, ref_max: bf16_tol(scale, out_f32, causal, n)


def one_bf16_rounding(causal, n, ref_max):   # fp32 arithmetic stored as bf16 (tests/test_gpu_sweeps.py, wide head dims; test_gpu_head_dims.py)
    return 2.0 ** -8 * max(1.0, ref_max)


def build_paths():
    P = []
    # ---- fp32 tensors -------------------------------------------------------------------------------------------------------------
    for d in (32, 64, 128):
        P.append(Path(F32, "auto", d, const(sweeps.TOL_F32), sweeps.TOL_F32))            # test_every_sequence_length_of_the_short_range
        for mode in {32: (0, 1, 3, 4), 64: (0, 1, 3, 4), 128: (0, 1, 3, 5)}[d]:           # test_split_kernel_tilings, plus split:0
            P.append(Path(F32, f"split:{mode}", d, const(TOL_F32), TOL_F32))
        P.append(Path(F32, "exact", d, const(TOL_EXACT), TOL_EXACT))                      # test_causal_paired_tiles_in_the_exact_kernel: 1e-4
        P.append(Path(F32, "exact:1", d, const(TOL_EXACT), TOL_EXACT))
        P.append(Path(F32, "exact:2", d, const(TOL_EXACT), TOL_EXACT, causal=CAUSAL))
    for d in (96, 256):                                                                   # test_every_sequence_length_at_the_wide_head_dims
        P.append(Path(F32, "exact", d, const(sweeps.TOL_F32), sweeps.TOL_F32))
    P.append(Path(F32, "naive", 40, const(TOL_EXACT), TOL_EXACT))                         # test_any_other_head_dim_runs_on_the_rung_0_kernel
    P.append(Path(F32, "auto", 64, const(TOL_F32), 1e-3, shapes=((1, 4100),), keysplit=True))                    # test_fp32_key_split_launch
    P.append(Path(F32, "exact", 64, const(TOL_EXACT), TOL_EXACT, shapes=((1, 2049),), keysplit=True))            # test_exact_kernel_key_split_launch
    P.append(Path(F32, "exact", 32, const(TOL_EXACT), TOL_EXACT, shapes=((5, 2200),), keysplit=True))
    # ---- bf16 tensors, both output types ------------------------------------------------------------------------------------------
    for dt in (BF16, BF16_F32):
        f32o = dt == BF16_F32
        for d, variants in ((64, (0, 1, 7, 30, 50)), (128, (0, 1, 10, 50)), (32, (0, 1, 50))):    # test_bf16_*tiling_variants_agree: scale 1/8
            for var in variants:
                P.append(Path(dt, f"mfma:{var}", d, bf16_p(0.125, f32o), 2e-2, scale=0.125, causal=FULL if var == 30 else BOTH))
        for d in (32, 64, 128):
            for kern in ("pb2", "pb2:1"):                                                 # test_pb2_kernel_vs_oracle / the sweeps: TOL_PB2
                P.append(Path(dt, kern, d, const(TOL_PB2) if f32o else bf16_p(1.0, False), TOL_PB2 if f32o else 2e-2))
            for mode in (0, 1, 3):                                                        # test_bf16_tensors_accurate_mode
                P.append(Path(dt, f"split:{mode}", d, const(TOL_F32) if f32o else bf16_p(1.0, False), TOL_F32))
        for d in (96, 192):                                                               # test_every_sequence_length_at_the_wide_head_dims_bf16_tensors
            P.append(Path(dt, "auto", d, const(sweeps.TOL_F32) if f32o else one_bf16_rounding, sweeps.TOL_F32))
        P.append(Path(dt, "naive", 40, const(TOL_EXACT) if f32o else one_bf16_rounding, TOL_EXACT))
        # key shares.  bf16 P, non-causal: test_key_split_launch_for_grids_that_leave_the_chip_idle
        P.append(Path(dt, "mfma", 64, bf16_p(1.0, f32o), 2e-2, causal=FULL, shapes=((1, 4097),), keysplit=True))
        P.append(Path(dt, "mfma", 128, bf16_p(1.0, f32o), 2e-2, causal=FULL, shapes=((1, 4096),), keysplit=True))
    # causal: test_causal_key_split_launch (auto with a bf16 output, mfma and pb2 with an fp32 output)
    for d, shape in ((64, (7, 4097)), (32, (1, 4096))):
        P.append(Path(BF16, "auto", d, bf16_p(1.0, False), 2e-2, causal=CAUSAL, shapes=(shape,), keysplit=True))
        P.append(Path(BF16_F32, "mfma", d, bf16_p(1.0, True), 2e-2, causal=CAUSAL, shapes=(shape,), keysplit=True))
        P.append(Path(BF16_F32, "pb2", d, const(TOL_PB2), 1e-4, causal=CAUSAL, shapes=(shape,), keysplit=True))
    # the two-term kernel's short-row split: test_short_row_key_split_of_the_two_term_kernel
    for d, shape in ((32, (1, 1025)), (64, (3, 1100))):
        for kern in ("auto", "pb2"):
            P.append(Path(BF16_F32, kern, d, const(TOL_PB2), 1e-4, causal=FULL, shapes=(shape,), keysplit=True))
    return P


PATHS = build_paths()
assert len({p.id for p in PATHS}) == len(PATHS)


# ---------------------------------------------------------------------------------------------------------------------------------
# one forward inside the arena
# ---------------------------------------------------------------------------------------------------------------------------------
def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace_bytes(p: Path, bh, n, causal):
    return int(_cabi.lib().fa_workspace_bytes(bh, n, p.d, int(causal), p.dtype, _kernel_id(p.kernel)))


def new_arena(p: Path, bh, n, causal, seed):
    """q, k, v = N(0, 1) of the path's dtype from `seed`; the workspace exactly fa_workspace_bytes, no slack byte."""
    need = workspace_bytes(p, bh, n, causal)
    if p.keysplit:
        assert need > 0, f"{p.id} {bh}x{n}: not a key-split launch"
    a = ar.Arena.for_forward(bh, n, p.d, IN_DTYPE[p.dtype], OUT_DTYPE[p.dtype], need, dev())
    g = torch.Generator(device=dev()).manual_seed(seed)
    for x in ("q", "k", "v"):
        a.view(x).copy_(torch.randn(bh, n, p.d, device=dev(), generator=g).to(IN_DTYPE[p.dtype]))
    return a, need


def run_in_arena(a, p: Path, bh, n, causal, need, ws_byte=0xFF, null_workspace=False):
    """o, lse and the workspace poisoned (NaN; the workspace with `ws_byte`), one forward, synchronised."""
    ar.fill_bytes(a.view("o"), 0xFF)
    ar.fill_bytes(a.view("lse"), 0xFF)
    if need:
        a.view("workspace").fill_(ws_byte)
    use_ws = need > 0 and not null_workspace
    L = _cabi.lib()
    rc = L.fa_forward_ws(a.ptr("q"), a.ptr("k"), a.ptr("v"), a.ptr("o"), a.ptr("lse"), bh, n, p.d, p.scale, int(causal), p.dtype, _kernel_id(p.kernel),
                         a.ptr("workspace") if use_ws else None, need if use_ws else 0, stream())
    assert rc == 0, f"{p.id} {bh}x{n} causal={causal}: {L.fa_last_error().decode()}"
    torch.cuda.synchronize()


def rung0(p: Path, q, k, v, causal):
    """The rung-0 kernel on plain dense copies (fresh allocations): fp32 arithmetic on the same values, fp32 output and LSE."""
    return fa.forward(q.clone(), k.clone(), v.clone(), causal, scale=p.scale, kernel="naive", out_dtype=torch.float32, return_lse=True)


def errors(o, lse, ref, lref):
    return float((o.float() - ref).abs().max()), float((lse - lref).abs().max())


def seed_of(*what):
    return zlib.crc32(repr(what).encode())


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. nothing outside the output buffers is written
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PATHS, ids=[p.id for p in PATHS])
def test_nothing_outside_the_output_buffers_is_written(p):
    bad = []
    for bh, n in p.shapes:
        for causal in p.causal:
            a, need = new_arena(p, bh, n, causal, seed_of(p.id, bh, n, causal))
            ref, lref = rung0(p, a.view("q"), a.view("k"), a.view("v"), causal)
            tol = p.tol(causal, n, float(ref.abs().max()))
            for null_ws in ((False, True) if need else (False,)):       # key shares: once more with the NULL workspace (the unsplit launch)
                a.fill_output_guards()
                run_in_arena(a, p, bh, n, causal, need, null_workspace=null_ws)
                o, lse = a.view("o"), a.view("lse")
                intact = a.guards_intact()
                nan_free = not bool(torch.isnan(o.float()).any()) and not bool(torch.isnan(lse).any())
                eo, el = errors(o, lse, ref, lref)
                observe("writes" + ("/null" if null_ws else ""), p.id, (bh, n, p.d), causal, eo, tol, intact)
                untouched = not null_ws or bool((a.view("workspace") == 0xFF).all())     # a workspace that was not passed is not written
                if not (intact and nan_free and eo < tol and el < p.tol_lse and untouched):
                    bad.append((bh, n, causal, "null ws" if null_ws else "ws", str(a.first_damage()), f"nan_free={nan_free}", eo, tol, el, p.tol_lse,
                                f"workspace untouched={untouched}"))
    assert not bad, bad[:8]


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. nothing outside a slab's own rows influences its output
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PATHS, ids=[p.id for p in PATHS])
def test_a_slab_depends_on_its_own_rows_only(p):
    bad = []
    for bh, n in p.shapes:
        for causal in p.causal:
            a, need = new_arena(p, bh, n, causal, seed_of(p.id, bh, n, causal, "isolation"))
            s = 1 if bh >= 3 else 0                                   # the slab under test; every other slab is a neighbour
            others = [b for b in range(bh) if b != s]
            ref, lref = rung0(p, a.view("q")[s:s + 1], a.view("k")[s:s + 1], a.view("v")[s:s + 1], causal)     # slab s alone
            tol = p.tol(causal, n, float(ref.abs().max()))
            runs = []
            for what, ws_byte in (("clean", 0x00), ("clean again", 0x00), ("A", 0xFF), ("B", 0x00)):
                if what == "A":
                    a.fill_input_surroundings("nan", slabs=others)
                elif what == "B":
                    a.fill_input_surroundings("finite", seed=seed_of(p.id, n, "other data"), slabs=others)
                run_in_arena(a, p, bh, n, causal, need, ws_byte=ws_byte)
                runs.append((a.view("o")[s].clone(), a.view("lse")[s].clone()))
            clean, again, run_a, run_b = runs
            # premise: two identical clean runs are bit-identical
            if not (ar.bit_equal(clean[0], again[0]) and ar.bit_equal(clean[1], again[1])):
                bad.append((bh, n, causal, "PREMISE: two clean runs differ"))
                continue
            fails = ar.isolation_failures(clean, run_a, run_b)
            eo, el = errors(run_a[0][None], run_a[1][None], ref, lref)
            observe("isolation", p.id, (bh, n, p.d), causal, eo, tol, a.guards_intact())
            if fails or not (eo < tol and el < p.tol_lse):
                bad.append((bh, n, causal, fails, eo, tol, el, p.tol_lse))
    assert not bad, bad[:8]


# ---------------------------------------------------------------------------------------------------------------------------------
# the packed llm.c entry
# ---------------------------------------------------------------------------------------------------------------------------------
PACKED_T = (1, 33, 129, 257, 700)


def unpack(inp, nh, hs):
    B, T = inp.shape[:2]
    return tuple(inp[:, :, i * nh * hs:(i + 1) * nh * hs].reshape(B, T, nh, hs).permute(0, 2, 1, 3).reshape(B * nh, T, hs).contiguous() for i in range(3))


def packed_rung0(inp, nh, hs):
    B, T = inp.shape[:2]
    q, k, v = unpack(inp, nh, hs)
    return fa.forward(q, k, v, True, scale=hs ** -0.5, kernel="naive").reshape(B, nh, T, hs).permute(0, 2, 1, 3).reshape(B, T, nh * hs)


def run_packed(a, B, T, C, nh):
    ar.fill_bytes(a.view("out"), 0xFF)
    L = _cabi.lib()
    rc = L.fa_forward_packed_qkv(a.ptr("inp"), a.ptr("out"), B, T, C, nh, stream())
    assert rc == 0, L.fa_last_error().decode()
    torch.cuda.synchronize()


@pytest.mark.parametrize("nh", [1, 3])
@pytest.mark.parametrize("hs", [32, 64, 128, 96])
def test_packed_qkv_writes_nothing_outside_out(hs, nh):
    """inp and out in the arena; against rung 0 on the unpacked tensors at the entry's own 1e-4 (tests/test_gpu_sweeps.py)."""
    B, C, bad = 2, nh * hs, []
    for T in PACKED_T:
        a = ar.Arena.for_packed(B, T, C, dev())
        a.view("inp").copy_(torch.randn(B, T, 3 * C, device=dev(), generator=torch.Generator(device=dev()).manual_seed(seed_of(hs, nh, T))))
        a.fill_output_guards()
        run_packed(a, B, T, C, nh)
        out = a.view("out")
        intact, nan_free = a.guards_intact(), not bool(torch.isnan(out).any())
        e = float((out - packed_rung0(a.view("inp").clone(), nh, hs)).abs().max())
        observe("writes", f"packed-qkv-hs{hs}-nh{nh}", (B, T, 3 * C), True, e, 1e-4, intact)
        if not (intact and nan_free and e < 1e-4):
            bad.append((T, str(a.first_damage()), nan_free, e))
    assert not bad, bad


@pytest.mark.parametrize("nh", [1, 3])
@pytest.mark.parametrize("hs", [32, 64, 128, 96])
def test_packed_qkv_block_depends_on_its_own_batch_and_head_only(hs, nh):
    """All heads but one and all batches but one are 0xFF bytes (run A) or finite data of another seed (run B), and so are the guards of inp:
    the surviving (batch, head) block of out is finite and bit-identical to the all-finite clean run."""
    B, C, bad = 2, nh * hs, []
    b0, h0 = 1, nh // 2
    cols = [i * C + h0 * hs + c for i in range(3) for c in range(hs)]      # the block's q, k and v columns of a token row
    for T in PACKED_T:
        a = ar.Arena.for_packed(B, T, C, dev())
        inp = a.view("inp")
        inp.copy_(torch.randn(B, T, 3 * C, device=dev(), generator=torch.Generator(device=dev()).manual_seed(seed_of(hs, nh, T, "isolation"))))
        block = inp[b0][:, cols].clone()
        want = packed_rung0(inp[b0:b0 + 1].clone(), nh, hs)[0, :, h0 * hs:(h0 + 1) * hs]
        runs = []
        for what in ("clean", "clean again", "A", "B"):
            if what in ("A", "B"):
                a.fill_input_surroundings("nan" if what == "A" else "finite", seed=seed_of(hs, nh, T, "other data"), slabs=range(B))
                inp[b0][:, cols] = block
            run_packed(a, B, T, C, nh)
            runs.append((a.view("out")[b0, :, h0 * hs:(h0 + 1) * hs].clone(),))
        clean, again, run_a, run_b = runs
        if not ar.bit_equal(clean[0], again[0]):
            bad.append((T, "PREMISE: two clean runs differ"))
            continue
        fails = ar.isolation_failures(clean, run_a, run_b)
        e = float((run_a[0] - want).abs().max())
        observe("isolation", f"packed-qkv-hs{hs}-nh{nh}", (B, T, 3 * C), True, e, 1e-4, a.guards_intact())
        if fails or not e < 1e-4:
            bad.append((T, fails, e))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the 32-bit boundaries
# ---------------------------------------------------------------------------------------------------------------------------------
GIB = 1 << 30


def need_memory(nbytes):
    """Skip ONLY when the device reports less free memory than 1.25 x what the case allocates."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 1.25 * nbytes:
        pytest.skip(f"free device memory {free} bytes < 1.25 x the {nbytes} bytes this case allocates")


def randn_big(shape, dtype, gen, step=2048):
    t = torch.empty(shape, dtype=dtype, device=dev())
    for i in range(0, shape[0], step):
        j = min(i + step, shape[0])
        t[i:j] = torch.randn((j - i,) + tuple(shape[1:]), device=dev(), generator=gen).to(dtype)
    return t


def whole_tensor_check(o, ref, step=2048):
    """(max |o - ref|, any NaN in o) over the whole tensor, a few thousand slabs at a time."""
    worst = torch.zeros((), device=dev())
    nan = torch.zeros((), dtype=torch.bool, device=dev())
    for i in range(0, o.shape[0], step):
        c = o[i:i + step].float()
        nan |= torch.isnan(c).any()
        worst = torch.maximum(worst, (c - ref[i:i + step]).abs().max())
    return float(worst), bool(nan)


def boundary_slabs(bh, slab_elems):
    """First and last slab and the two slabs on either side of the element offsets 2^30 and 2^31 (= byte offsets 2^32 of an fp32 tensor,
    2^31 / 2^32 of a bf16 tensor, 2^33 of the fp32 output of bf16 tensors)."""
    s = {0, bh - 1}
    for off in (1 << 30, 1 << 31):
        b = off // slab_elems
        s |= {x for x in (b - 1, b) if 0 <= x < bh}
    return sorted(s)


def raw_forward(q, k, v, o, causal, scale, dtype, kernel):
    bh, n, d = q.shape
    L = _cabi.lib()
    assert L.fa_workspace_bytes(bh, n, d, int(causal), dtype, _kernel_id(kernel)) == 0
    rc = L.fa_forward_ws(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), None, bh, n, d, scale, int(causal), dtype, _kernel_id(kernel), None, 0, stream())
    assert rc == 0, L.fa_last_error().decode()
    torch.cuda.synchronize()


# (name, bh, n, d, input dtype, ((kernel, fa_dtype, threshold), ...)) -- thresholds: test_long_sequences_and_many_slabs_against_rung0 (fp32 tensors and
# the accurate P: TOL_F32; bf16 P with a bf16 output: the suite's threshold for that output type, bf16_tol(., False))
BIG = [
    ("fp32-over-2^32-bytes", 65600, 128, 128, torch.float32, (("auto", F32, TOL_F32), ("exact", F32, TOL_F32))),
    ("bf16-over-2^31-elements-d128", 131200, 128, 128, torch.bfloat16, (("mfma", BF16, bf16_tol(1.0, False)), ("auto", BF16_F32, TOL_F32))),
    ("bf16-over-2^31-elements-d32", 262400, 256, 32, torch.bfloat16, (("mfma", BF16, bf16_tol(1.0, False)), ("auto", BF16_F32, TOL_F32))),
    ("fp32-d256-over-2^32-bytes", 65600, 64, 256, torch.float32, (("auto", F32, TOL_F32),)),
]


def test_the_two_bf16_boundary_cases_run_different_kernel_families():
    L = _cabi.lib()
    for causal in (0, 1):
        assert L.fa_kernel_name_for(BF16, 128, causal, 131200, 128) != L.fa_kernel_name_for(BF16, 32, causal, 262400, 256)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("name,bh,n,d,in_dtype,kernels", BIG, ids=[b[0] for b in BIG])
def test_tensors_beyond_the_32_bit_boundaries(name, bh, n, d, in_dtype, kernels, causal):
    """One launch over short rows whose tensors cross 2^31 elements / 2^32 bytes (the fp32 output of bf16 tensors: 2^33): NaN-poisoned outputs,
    the whole tensor against rung 0, and rung 0 itself pinned slab by slab around the boundaries -- which is how its own launch of more than
    2^32 threads (262 400 slabs of 256 rows) was found to compute the first 256 slabs only and report success (fa_naive.hip: launch_naive)."""
    elems = bh * n * d
    assert elems > (1 << 31 if in_dtype == torch.bfloat16 else 1 << 30)
    es = 2 if in_dtype == torch.bfloat16 else 4
    need_memory(3 * elems * es + 2 * elems * 4 + 2 * GIB)        # q, k, v; rung 0's output and one o at a time; the comparisons' temporaries
    scale = d ** -0.5
    try:
        g = torch.Generator(device=dev()).manual_seed(seed_of(name))
        q, k, v = (randn_big((bh, n, d), in_dtype, g) for _ in range(3))
        ref = torch.full((bh, n, d), float("nan"), dtype=torch.float32, device=dev())
        raw_forward(q, k, v, ref, causal, scale, F32 if in_dtype == torch.float32 else BF16_F32, "naive")
        # rung 0 itself at these offsets: the same slabs in a small dense tensor, bit for bit (one wave per row: no shape-dependent tiling)
        idx = boundary_slabs(bh, n * d)
        assert len(idx) >= 4
        small = fa.forward(q[idx].contiguous(), k[idx].contiguous(), v[idx].contiguous(), causal, scale=scale, kernel="naive", out_dtype=torch.float32)
        for i, b in enumerate(idx):
            assert ar.bit_equal(small[i], ref[b]), f"rung 0 differs at slab {b}"
        b = idx[-2]                                               # the slab right behind the last boundary inside the tensor
        r64 = orc.attention_f64(*(t[b:b + 1].float().cpu().numpy() for t in (q, k, v)), causal=causal, scale=scale)
        e64 = float(np.abs(ref[b:b + 1].cpu().numpy().astype(np.float64) - r64).max())
        assert e64 < 1e-4, e64
        for kernel, dtype, tol in kernels:
            o = torch.full((bh, n, d), float("nan"), dtype=OUT_DTYPE[dtype], device=dev())
            raw_forward(q, k, v, o, causal, scale, dtype, kernel)
            err, nan = whole_tensor_check(o, ref)
            observe("32-bit", f"{name}-{kernel}-{DT_NAME[dtype]}", (bh, n, d), causal, err, tol, None)
            assert not nan, f"{kernel}: NaN (unwritten or invalid elements)"
            assert err < tol, f"{kernel}: {err:.3e}"
            del o
    finally:
        q = k = v = ref = small = o = None
        torch.cuda.empty_cache()


def test_packed_qkv_with_more_than_2_31_input_elements():
    B, T, C, nh = 3700, 256, 768, 12
    hs = C // nh
    assert B * T * 3 * C > 1 << 31
    need_memory(B * T * 3 * C * 4 + B * T * C * 4 + 2 * GIB)
    try:
        inp = randn_big((B, T, 3 * C), torch.float32, torch.Generator(device=dev()).manual_seed(31), step=64)
        out = torch.full((B, T, C), float("nan"), device=dev())
        L = _cabi.lib()
        assert L.fa_forward_packed_qkv(inp.data_ptr(), out.data_ptr(), B, T, C, nh, stream()) == 0, L.fa_last_error().decode()
        torch.cuda.synchronize()
        nan = torch.zeros((), dtype=torch.bool, device=dev())
        for i in range(0, B, 64):
            nan |= torch.isnan(out[i:i + 64]).any()
        assert not bool(nan), "NaN (unwritten or invalid elements)"
        straddling = (1 << 31) // (T * 3 * C)                      # the batch the 2^31-element offset of inp falls into
        worst = 0.0
        for b in (B - 1, straddling, 0):
            want = packed_rung0(inp[b:b + 1].clone(), nh, hs)[0]
            for h in (0, 5, 11):                                   # three (batch, head) blocks of each, the last batch first
                worst = max(worst, float((out[b, :, h * hs:(h + 1) * hs] - want[:, h * hs:(h + 1) * hs]).abs().max()))
        observe("32-bit", "packed-qkv", (B, T, 3 * C), True, worst, 1e-4, None)
        assert worst < 1e-4, worst
    finally:
        inp = out = None
        torch.cuda.empty_cache()
