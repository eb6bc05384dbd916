"""CPU: the guard-band arena of tests/arena.py detects what it is there to detect -- fake "kernels" on CPU tensors that store one element
next to an output buffer, or that multiply an element of an input guard by zero, must be caught (tests/test_gpu_memory_bounds.py relies on it)."""
import pytest
import torch

from tests import arena as ar

BH, N, D = 3, 33, 64


def make(in_dtype=torch.float32, out_dtype=torch.float32, workspace_bytes=4096):
    a = ar.Arena.for_forward(BH, N, D, in_dtype, out_dtype, workspace_bytes, "cpu")
    g = torch.Generator().manual_seed(5)
    for name in ("q", "k", "v"):
        a.view(name).copy_(torch.randn(BH, N, D, generator=g).to(in_dtype))
    return a


def attention(q, k, v):
    return torch.softmax(q.double() @ k.double().transpose(-1, -2), dim=-1) @ v.double()


def fake_forward(a, leak=None):
    """O = softmax(Q K^T) V per slab into the arena's o (and a row sum into lse); `leak` = (buffer, side): additionally 0 * the guard element
    next to that input buffer is added to every output element -- the load past a slab that a numeric comparison never sees."""
    extra = 0.0
    if leak is not None:
        b = a.bufs[leak[0]]
        es = b.nbytes // (BH * N * D)
        at = b.start - es if leak[1] == "before" else b.end
        extra = 0.0 * a.raw[at:at + es].view(b.dtype)[0].double()
    q, k, v = (a.view(x) for x in ("q", "k", "v"))
    a.view("o").copy_((attention(q, k, v) + extra).to(a.view("o").dtype))
    a.view("lse").copy_(torch.logsumexp(q.double() @ k.double().transpose(-1, -2), dim=-1).float())


@pytest.mark.parametrize("in_dtype,out_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)])
def test_layout_minimum_alignment_and_guard_sizes(in_dtype, out_dtype):
    a = make(in_dtype, out_dtype)
    spans = []
    for name, b in a.bufs.items():
        p = a.ptr(name)
        if b.align == "tensor":
            assert p % 16 == 0 and p % 32 != 0, name            # an odd multiple of 16
        elif b.align == "lse":
            assert p % 16 == 4, name                            # 4 bytes and no better
        else:
            assert p % 256 == 0 and p % 512 != 0, name          # an odd multiple of 256
        assert b.start - b.before[0] >= ar.GUARD_BYTES and b.after[1] - b.end >= ar.GUARD_BYTES, name
        assert b.before[1] == b.start and b.after[0] == b.end and b.end - b.start == b.nbytes
        assert tuple(a.view(name).shape) == b.shape and a.view(name).dtype == b.dtype and a.view(name).data_ptr() == p
        spans.append((b.before[0], b.after[1]))
    assert a.bufs["workspace"].nbytes == 4096
    assert all(hi <= lo2 for (_, hi), (lo2, _) in zip(spans, spans[1:])) and spans[-1][1] <= a.raw.numel()     # no guard is shared
    assert "workspace" not in ar.Arena.for_forward(1, 1, 32, in_dtype, out_dtype, 0, "cpu").bufs
    p = ar.Arena.for_packed(2, 5, 96, "cpu")
    assert tuple(p.view("inp").shape) == (2, 5, 288) and tuple(p.view("out").shape) == (2, 5, 96) and p.names("out") == ["out"]


def test_a_clean_forward_leaves_the_guards_intact():
    a = make()
    a.fill_output_guards()
    for name in ("o", "lse", "workspace"):
        ar.fill_bytes(a.view(name), 0xFF)          # writing every byte of the buffers themselves, first to last, is no damage
    fake_forward(a)
    assert a.guards_intact() and a.first_damage() is None
    assert not torch.isnan(a.view("o")).any()


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("side", ["before", "after"])
@pytest.mark.parametrize("name", ["o", "lse", "workspace"])
def test_one_element_stored_next_to_an_output_buffer_is_found(name, side, out_dtype):
    a = make(torch.bfloat16 if out_dtype == torch.bfloat16 else torch.float32, out_dtype)
    a.fill_output_guards()
    fake_forward(a)
    assert a.guards_intact()
    b = a.bufs[name]
    dt = torch.float32 if name == "workspace" else b.dtype       # (the workspace holds fp32 partials)
    es = torch.empty((), dtype=dt).element_size()
    at = b.start - es if side == "before" else b.end
    a.raw[at:at + es].view(dt).fill_(1.0)                        # the fake kernel's stray store: the element directly next to the buffer
    assert not a.guards_intact()
    dmg = a.first_damage()
    assert (dmg.name, dmg.side, dmg.rows) == (name, side, 1), str(dmg)
    assert name in str(dmg) and side in str(dmg)
    a.fill_output_guards()                                       # refilled: intact again
    assert a.guards_intact()


def test_a_store_rows_away_is_reported_in_rows():
    a = make()
    a.fill_output_guards()
    b = a.bufs["o"]
    a.raw[b.end + 5 * b.row_bytes + 8] = 0                       # inside the sixth row past the end
    a.raw[b.after[1] - 1] = 0                                    # and the last byte of the guard
    dmg = a.first_damage()
    assert (dmg.name, dmg.side, dmg.rows) == ("o", "after", 6)
    a.fill_output_guards()
    a.raw[a.bufs["lse"].before[0]] = 0                           # the guard's first byte, 1 MiB before lse
    dmg = a.first_damage()
    assert (dmg.name, dmg.side) == ("lse", "before") and dmg.rows >= ar.GUARD_BYTES // 4


def run_abc(a, leak):
    """The three runs of the isolation test: clean, A (NaN bytes around slab 1), B (finite data of another seed around it)."""
    keep = {x: a.view(x)[1].clone() for x in ("q", "k", "v")}
    outs = []
    for mode in ("clean", "nan", "finite"):
        if mode != "clean":
            a.fill_input_surroundings(mode, seed=77, slabs=(0, 2))
        for x in ("q", "k", "v"):
            assert ar.bit_equal(a.view(x)[1], keep[x])            # the slab under test is never touched
        fake_forward(a, leak)
        outs.append((a.view("o")[1].clone(), a.view("lse")[1].clone()))
    return outs


@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16])
def test_input_fills_are_nan_or_finite(in_dtype):
    a = make(in_dtype, torch.float32)
    a.fill_input_surroundings("nan", slabs=(0, 2))
    for x in ("q", "k", "v"):
        b = a.bufs[x]
        assert torch.isnan(a.view(x)[0]).all() and torch.isnan(a.view(x)[2]).all() and torch.isfinite(a.view(x)[1]).all()
        for lo, hi in (b.before, b.after):
            assert bool((a.raw[lo:hi] == 0xFF).all())
            assert torch.isnan(a.raw[hi - 1024:hi].view(in_dtype)).all()
    a.fill_input_surroundings("finite", seed=3, slabs=(0, 2))
    first = a.view("k")[0].clone()
    for x in ("q", "k", "v"):
        b = a.bufs[x]
        assert torch.isfinite(a.view(x)).all() and float(a.view(x)[0].float().std()) > 0.5
        for lo, hi in (b.before, b.after):
            g = a.raw[lo:hi].view(in_dtype).float()
            assert torch.isfinite(g).all() and 0.5 < float(g.std()) < 2.0
    a.fill_input_surroundings("finite", seed=3, slabs=(0, 2))
    assert ar.bit_equal(a.view("k")[0], first)                    # the seed decides
    a.fill_input_surroundings("finite", seed=4, slabs=(0, 2))
    assert not ar.bit_equal(a.view("k")[0], first)
    assert a.guards_intact()                                      # filling the input side leaves the output side alone


def test_isolation_comparison_passes_a_kernel_that_stays_inside_its_slab():
    clean, run_a, run_b = run_abc(make(), None)
    assert ar.isolation_failures(clean, run_a, run_b) == []


@pytest.mark.parametrize("side", ["before", "after"])
@pytest.mark.parametrize("name", ["q", "k", "v"])
def test_zero_times_a_guard_element_fails_the_isolation_comparison(name, side):
    """The numbers of run B (finite surroundings) and of the clean run are right -- 0 * x = 0 --, which is why no numeric comparison sees this
    load; run A turns it into a NaN."""
    clean, run_a, run_b = run_abc(make(), (name, side))
    assert ar.bit_equal(clean[0], run_b[0]) and torch.isfinite(run_b[0]).all()
    bad = ar.isolation_failures(clean, run_a, run_b)
    assert any("not finite with NaN around the slab" in s for s in bad) and any("differs between NaN and finite" in s for s in bad), bad


def test_isolation_comparison_sees_single_bit_differences():
    clean, run_a, run_b = run_abc(make(), None)
    flipped = run_b[1].clone()
    flipped.view(torch.int32)[7] ^= 1
    assert any("output 1" in s for s in ar.isolation_failures(clean, run_a, (run_b[0], flipped)))
    neg_zero = (torch.zeros(4), ), (torch.zeros(4), ), (-torch.zeros(4), )
    assert ar.isolation_failures(*neg_zero) != []                 # +0 / -0: not bit-identical
