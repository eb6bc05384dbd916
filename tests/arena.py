"""Guard-band arena for the memory-bounds tests (tests/test_gpu_memory_bounds.py; self-test: tests/test_arena.py).

One byte tensor holds every buffer of a forward -- q, k, v, o, lse, workspace (or inp, out of the packed entry) -- each with a guard of at
least GUARD_BYTES before and after it, and each at the MINIMUM alignment include/flashattn_amd.h allows: q, k, v, o at an odd multiple of
16 bytes, lse at 4 bytes and no better (address = 4 mod 16), the workspace at an odd multiple of 256.  1 MiB is twice the furthest a tile
of any kernel can overreach (512 rows x d = 256 x 4 B = 512 KiB), so a kernel that stores or loads past a buffer lands in a guard of the
same allocation: the test fails an assertion, nothing is arranged to fault.

  output side   the guards of o, lse, workspace hold a byte pattern; guards_intact() / first_damage() say whether they still do
  input side    the guards of q, k, v (and chosen slabs) hold either 0xFF bytes -- a NaN in fp32 and in bf16 -- or finite N(0, 1) data from
                a seed: a load past a slab that is multiplied by P = 0 gives NaN in the first case and the right number in the second, so
                the two runs differ (isolation_failures)

Works on CPU tensors too (the self-test runs fake kernels there).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

GUARD_BYTES = 1 << 20
PATTERN = 0xA5                      # output-side guards (as fp32 / bf16 a finite value: a kernel that reads one does not turn it into a NaN by itself)
POISON = 0xFF                       # input-side guards: 0xFFFFFFFF / 0xFFFF are NaNs
# address = rem (mod `mod`): the weakest alignment the header promises, and no better
ALIGNMENT = {"tensor": (32, 16), "lse": (16, 4), "workspace": (512, 256)}


@dataclass
class Buf:
    name: str
    kind: str                       # "in" | "out"
    dtype: torch.dtype
    shape: Tuple[int, ...]
    align: str                      # key of ALIGNMENT
    row_bytes: int                  # what "one row" of this buffer is, for the damage report
    start: int = 0                  # byte offsets into the arena
    end: int = 0
    before: Tuple[int, int] = (0, 0)
    after: Tuple[int, int] = (0, 0)

    @property
    def nbytes(self) -> int:
        n = torch.empty((), dtype=self.dtype).element_size()
        for s in self.shape:
            n *= s
        return n


@dataclass
class Damage:
    name: str                       # buffer whose guard was written
    side: str                       # "before" | "after"
    rows: int                       # distance of the first (lowest-address) damaged byte from the buffer's edge, in rows of the buffer (>= 1)
    byte: int                       # the same distance in bytes

    def __str__(self) -> str:
        return f"guard {self.side} {self.name} damaged {self.rows} row(s) ({self.byte} bytes) from the buffer"


def _elsize(dtype: torch.dtype) -> int:
    return torch.empty((), dtype=dtype).element_size()


class Arena:
    def __init__(self, bufs: Sequence[Buf], device, guard_bytes: int = GUARD_BYTES):
        assert guard_bytes >= GUARD_BYTES and guard_bytes % 16 == 0
        self.bufs: Dict[str, Buf] = {}
        self.guard_bytes = guard_bytes
        total = 1024 + sum((b.nbytes + 15) // 16 * 16 + 2 * guard_bytes + 1024 for b in bufs)
        self.raw = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.raw.data_ptr()
        assert base % 16 == 0
        cur = base                                          # absolute addresses; always a multiple of 16
        for b in bufs:
            assert b.name not in self.bufs and b.kind in ("in", "out")
            mod, rem = ALIGNMENT[b.align]
            start = cur + guard_bytes
            start += (rem - start) % mod                    # the first address >= cur + guard with address = rem (mod `mod`)
            end = start + b.nbytes
            nxt = end + guard_bytes
            nxt += (-nxt) % 16
            b.start, b.end = start - base, end - base
            b.before, b.after = (cur - base, b.start), (b.end, nxt - base)
            assert b.start - b.before[0] >= guard_bytes and b.after[1] - b.end >= guard_bytes
            assert start % mod == rem and (b.align != "lse" or start % 8 != 0)
            self.bufs[b.name] = b
            cur = nxt
        assert cur - base <= total
        # what is between and around the buffers starts out as the output-side pattern everywhere; the input side is filled per run
        self.raw.fill_(PATTERN)

    # ---- the two layouts the tests use ------------------------------------------------------------------------------------------
    @classmethod
    def for_forward(cls, bh: int, n: int, d: int, in_dtype: torch.dtype, out_dtype: torch.dtype, workspace_bytes: int, device) -> "Arena":
        ein, eout = _elsize(in_dtype), _elsize(out_dtype)
        bufs = [Buf(x, "in", in_dtype, (bh, n, d), "tensor", d * ein) for x in ("q", "k", "v")]
        bufs.append(Buf("o", "out", out_dtype, (bh, n, d), "tensor", d * eout))
        bufs.append(Buf("lse", "out", torch.float32, (bh, n), "lse", 4))
        if workspace_bytes:
            bufs.append(Buf("workspace", "out", torch.uint8, (int(workspace_bytes),), "workspace", d * 4))
        return cls(bufs, device)

    @classmethod
    def for_packed(cls, B: int, T: int, C: int, device) -> "Arena":
        return cls([Buf("inp", "in", torch.float32, (B, T, 3 * C), "tensor", 3 * C * 4), Buf("out", "out", torch.float32, (B, T, C), "tensor", C * 4)], device)

    # ---- views ------------------------------------------------------------------------------------------------------------------
    def view(self, name: str) -> torch.Tensor:
        b = self.bufs[name]
        return self.raw[b.start:b.end].view(b.dtype).view(b.shape)

    def ptr(self, name: str) -> int:
        return self.raw.data_ptr() + self.bufs[name].start

    def names(self, kind: str) -> List[str]:
        return [b.name for b in self.bufs.values() if b.kind == kind]

    def _guards(self, kind: str):
        for b in self.bufs.values():
            if b.kind == kind:
                yield b, "before", b.before
                yield b, "after", b.after

    # ---- output side ------------------------------------------------------------------------------------------------------------
    def fill_output_guards(self) -> None:
        for _, _, (lo, hi) in self._guards("out"):
            self.raw[lo:hi].fill_(PATTERN)

    def _damaged_counts(self) -> List[int]:
        counts = [torch.count_nonzero(self.raw[lo:hi] != PATTERN) for _, _, (lo, hi) in self._guards("out")]
        return torch.stack(counts).tolist() if counts else []

    def guards_intact(self) -> bool:
        """True when every byte of every output-side guard still holds the pattern."""
        return not any(self._damaged_counts())

    def first_damage(self) -> Optional[Damage]:
        """The lowest-address damaged guard byte: which buffer it belongs to, on which side, and how many rows from the buffer's edge."""
        for (b, side, (lo, hi)), cnt in zip(self._guards("out"), self._damaged_counts()):
            if cnt:
                at = lo + int(torch.nonzero(self.raw[lo:hi] != PATTERN)[0])
                dist = b.start - at if side == "before" else at - b.end + 1
                return Damage(b.name, side, (dist + b.row_bytes - 1) // b.row_bytes, dist)
        return None

    # ---- input side -------------------------------------------------------------------------------------------------------------
    def _fill(self, lo: int, hi: int, dtype: torch.dtype, mode: str, gen: Optional[torch.Generator]) -> None:
        if mode == "nan":
            self.raw[lo:hi].fill_(POISON)
            return
        assert mode == "finite" and gen is not None
        es = _elsize(dtype)
        lo += (-lo) % es
        cnt = (hi - lo) // es
        self.raw[lo:lo + cnt * es].view(dtype).copy_(torch.randn(cnt, device=self.raw.device, generator=gen).to(dtype))

    def fill_input_surroundings(self, mode: str, seed: int = 0, slabs: Sequence[int] = ()) -> None:
        """Guards before and after every input buffer, and slabs `slabs` (first-axis indices) of every input buffer: mode "nan" = 0xFF bytes,
        mode "finite" = N(0, 1) values of the buffer's dtype drawn from `seed`."""
        gen = torch.Generator(device=self.raw.device).manual_seed(seed) if mode == "finite" else None
        for b, _, (lo, hi) in self._guards("in"):
            self._fill(lo, hi, b.dtype, mode, gen)
        for name in self.names("in"):
            b = self.bufs[name]
            slab_bytes = b.nbytes // b.shape[0]
            for s in slabs:
                self._fill(b.start + s * slab_bytes, b.start + (s + 1) * slab_bytes, b.dtype, mode, gen)


def fill_bytes(t: torch.Tensor, byte: int) -> None:
    """Every byte of a contiguous tensor (0xFF: NaN in fp32 and in bf16)."""
    t.view(torch.uint8).fill_(byte)


def bit_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit for bit (torch.equal calls two NaNs different and +0 / -0 equal)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def isolation_failures(clean: Sequence[torch.Tensor], run_a: Sequence[torch.Tensor], run_b: Sequence[torch.Tensor]) -> List[str]:
    """The A/B comparison: `clean`, `run_a` (everything around the slab is NaN), `run_b` (... is finite data of another seed) are the slab's
    outputs (o, lse, ...) of three runs of the same call.  Run A must be finite and all three bit-identical; returns what is not."""
    bad = []
    for i, (c, a, b) in enumerate(zip(clean, run_a, run_b)):
        if not bool(torch.isfinite(a.float()).all()):
            bad.append(f"output {i}: not finite with NaN around the slab ({int((~torch.isfinite(a.float())).sum())} elements)")
        if not bool(torch.isfinite(b.float()).all()):
            bad.append(f"output {i}: not finite with finite data around the slab")
        if not bit_equal(a, b):
            bad.append(f"output {i}: differs between NaN and finite surroundings")
        if not bit_equal(b, c):
            bad.append(f"output {i}: finite surroundings differ from the clean run")
    return bad
