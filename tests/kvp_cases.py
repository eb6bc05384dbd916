"""Structured softmax inputs for the chunked-prefill kernels at d = 128 (numpy only; tests/test_kvp_cases.py asserts what is claimed here,
tests/test_gpu_kvp_edges.py runs the kernels on them).

The kernels take a softmax step per 32 keys and rescale their accumulators only in a step where the maximum of some row of a 32-row block
moved.  N(0, 1) data moves some maximum of every block in nearly every step, so which rows decide that branch is never varied.  Here every
packed query row is given a logit profile over the keys:

  Q   row i of a slab is a * e_c, c = (i + shift * slab) % 128 (shift = 0 unless asked for), a a power of two: logit(i, j) = a * K[j, c],
      one product and 127 exact zeros, so the fp32 logit IS the fp64 logit
  K   column c of K is profile number c.  Every value is an e4m3 code (never 0x7F / 0xFF) times the power of two k_scale: one data set
      serves the bf16 libraries (dequantised, exact in bf16) and the fp8 libraries (the codes)
  V   N(0, 1) quantised to e4m3 at the power of two v_scale

With u = a * k_scale the logits are u x (values of the e4m3 grid).  Families (make(name, nk, seed), deterministic):

  staircase_up      the largest logit of every 32-key half block lies above everything before it: every full softmax step moves every row's
                    maximum.  Peaks climb the grid one level per half from 16 u (u = 1/8: logits 2 .. 56); where a half's peak sits varies
                    with the column; the other keys of a half lie up to 24 levels below its peak
  first_key_wins    key 0 carries the largest logit of the column, everything else is strictly smaller: no maximum moves after step 0
  lone_mover        a background that never rises (key 0 strictly above the rest, then non-increasing over the grid's levels in [-1, 1]: the
                    grid has 253 values, so "strictly decreasing" holds only across levels) and one spike per column at pos(c, nk), worth
                    48 u = 6: delta = 5.875 above key 0, the weight of ~350 background keys.  A step moves the maximum of the few rows whose
                    spike lies in it and of no other row
  lone_mover_large  the same with u = 2^12: the spike is 2^20, the background the 15 subnormal levels (|logit| <= 56): delta >= 2^19, every
                    other key weighs 0 beside the spike

late_start() is a length pattern, not data: causal lengths below nq, so that whole 32-row blocks see no key at all beside blocks that do
(every row that sees a key sees key 0, so "starts later" can only mean "starts in a later row block": the first block of a wave stays at
m = -inf through a step in which the second one moves).
"""
from dataclasses import dataclass

import numpy as np

from tests.kv8_reference import TABLE

D = 128
HALF = 32                                     # keys per softmax step of the kernels
FAMILIES = ("staircase_up", "first_key_wins", "lone_mover", "lone_mover_large")

_FINITE = [c for c in range(256) if c not in (0x7F, 0xFF, 0x80)]        # one zero
_ORDER = sorted(_FINITE, key=lambda c: TABLE[c])
GRID_CODES = np.array(_ORDER, dtype=np.uint8)                           # the 253 finite e4m3 values, ascending, as codes ...
GRID = TABLE[GRID_CODES]                                                # ... and as values
_ZERO = int(np.searchsorted(GRID, 0.0))
_L16 = int(np.searchsorted(GRID, 16.0))                                 # staircase_up starts here: 39 levels up to 448


def _level(value):
    i = int(np.searchsorted(GRID, value))
    assert GRID[i] == value, value
    return i


def pos(c, nk):
    """Key of column c's spike: the edges first (key 0, 31, 32, the last key, the first and the last key of the last 64-key block), then
    every half block in turn at an offset that varies with the column."""
    edges = [0, 31, 32, nk - 1, (nk - 1) // 64 * 64, nk - 1 - (nk - 1) % HALF]
    if c < len(edges):
        return int(min(max(edges[c], 0), nk - 1))
    halves = -(-nk // HALF)
    h = (c - len(edges)) % halves
    return int(min(HALF * h + (5 * c + 3) % HALF, nk - 1))


@dataclass
class Case:
    name: str
    nk: int
    a: float               # the non-zero component of every query row
    k_scale: float
    v_scale: float
    k_codes: np.ndarray    # (nk, D) uint8, read-only
    v_codes: np.ndarray

    @property
    def u(self):
        return self.a * self.k_scale

    def k(self):
        """logical K (nk, D), fp64"""
        return self.k_scale * TABLE[self.k_codes]

    def v(self):
        return self.v_scale * TABLE[self.v_codes]

    def q(self, bhq, nq, shift=0):
        """(bhq, nq, D) fp64: row i of slab s is a * e_((i + shift * s) % D)"""
        q = np.zeros((bhq, nq, D))
        for s in range(bhq):
            q[s, np.arange(nq), (np.arange(nq) + shift * s) % D] = self.a
        return q

    def logits(self):
        """(D, nk): row c is the logit profile of a query row a * e_c at scale 1"""
        return self.a * self.k().T


def _v_codes(nk, seed, v_scale):
    import torch   # the quantiser of the fp8 tests: torch's own cast
    from tests.kv8_reference import quantize
    v = torch.randn(nk, D, generator=torch.Generator().manual_seed(1000 + seed))
    return quantize(v, v_scale).view(torch.uint8).numpy().copy()


def make(name, nk, seed=0):
    assert name in FAMILIES and nk >= 1
    rng = np.random.default_rng([FAMILIES.index(name), nk, seed])
    halves = -(-nk // HALF)
    lev = np.empty((nk, D), dtype=np.int64)                     # indices into GRID
    a, k_scale = 4.0, 2.0 ** -5                                 # u = 1/8: |logit| <= 448 / 8 = 56
    if name == "staircase_up":
        top = len(GRID) - 1
        assert _L16 + halves - 1 <= top, "nk beyond the 39 levels from 16 to 448"
        for c in range(D):
            start = _L16 + (c * 7) % (top - _L16 - halves + 2)  # the column's first peak: start + halves - 1 <= top
            for h in range(halves):
                lo, hi = HALF * h, min(HALF * h + HALF, nk)
                peak = start + h
                lev[lo:hi, c] = rng.integers(peak - 24, peak, size=hi - lo)
                lev[lo + (7 * c + 3 * h) % (hi - lo), c] = peak
    elif name == "first_key_wins":
        for c in range(D):
            peak = _L16 + 8 + (c * 5) % 24                      # 32 .. 256: logits 4 .. 32
            lev[:, c] = rng.integers(peak - 24, peak, size=nk)
            lev[0, c] = peak
    else:
        large = name == "lone_mover_large"
        if large:
            a, k_scale = 1024.0, 4.0                            # u = 2^12
            hi_l, lo_l, spike = _level(7 * 2.0 ** -9), _level(-7 * 2.0 ** -9), _level(256.0)     # 15 levels, logits -56 .. 56 in steps of 8
        else:
            hi_l, lo_l, spike = _level(1.0), _level(-1.0), _level(48.0)                          # 113 levels, logits -1/8 .. 1/8
        n = hi_l - lo_l                                         # levels below the top one, which key 0 alone holds
        back = hi_l - 1 - (np.arange(nk) * n) // max(nk, 1)     # non-increasing, never the top level
        back[0] = hi_l
        for c in range(D):
            lev[:, c] = back
            lev[pos(c, nk), c] = spike
    k_codes = GRID_CODES[lev]
    v_scale = 2.0 ** -6
    v_codes = _v_codes(nk, seed, v_scale)
    assert not np.isin(k_codes, (0x7F, 0xFF)).any() and not np.isin(v_codes, (0x7F, 0xFF)).any()
    k_codes.setflags(write=False)
    v_codes.setflags(write=False)
    return Case(name, nk, a, k_scale, v_scale, k_codes, v_codes)


def moves(logits, last):
    """logits (rows, nk) fp64; last (rows,): the last key each row sees (-1: none).  Returns bool (rows, halves): the running maximum of the
    row over its visible keys rose in that 32-key step (the first step with a visible key counts)."""
    rows, nk = logits.shape
    halves = -(-nk // HALF)
    out = np.zeros((rows, halves), dtype=bool)
    run = np.full(rows, -np.inf)
    for h in range(halves):
        j = np.arange(HALF * h, min(HALF * h + HALF, nk))
        mx = np.where(j[None, :] <= np.asarray(last)[:, None], logits[:, j], -np.inf).max(axis=1)
        out[:, h] = mx > run
        run = np.maximum(run, mx)
    return out


def late_start():
    """bh_kv = 5, group = 2 (M = 320: a full tile and a 64-row one), causal: slab lengths below nq leave the rows i < nq - len without a key,
    whole 32-row blocks among them, the first block of a wave beside a second one that sees keys, and blocks cut in the middle."""
    return dict(nq=160, nk=224, group=2, kv_lens=[224, 160, 100, 37, 1])
