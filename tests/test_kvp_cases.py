"""CPU: the structured softmax inputs of tests/kvp_cases.py have the properties tests/test_gpu_kvp_edges.py relies on: every value is on the
e4m3 grid and exact in bf16, every logit is exact in fp32, and each family moves the running maximum of exactly the rows and 32-key steps its
description names (computed in fp64 from the data)."""
import numpy as np
import pytest
import torch

from tests import kvp_cases as kc

NKS = [321, 256, 33, 1100]     # the GPU shapes, one half block and a key, the largest nk the families are asked for


@pytest.mark.parametrize("nk", NKS)
@pytest.mark.parametrize("name", kc.FAMILIES)
def test_values_round_trip_through_e4m3_and_bf16_and_logits_are_exact_in_fp32(name, nk):
    case = kc.make(name, nk)
    again = kc.make(name, nk)
    assert np.array_equal(case.k_codes, again.k_codes) and np.array_equal(case.v_codes, again.v_codes)     # deterministic in (name, nk, seed)
    assert not np.array_equal(case.v_codes, kc.make(name, nk, seed=1).v_codes)
    for codes, scale, x in ((case.k_codes, case.k_scale, case.k()), (case.v_codes, case.v_scale, case.v())):
        assert codes.shape == (nk, kc.D) and codes.dtype == np.uint8 and not np.isin(codes, (0x7F, 0xFF)).any()
        assert np.log2(scale) == int(np.log2(scale))
        t = torch.from_numpy(x)
        back = (t / scale).to(torch.float8_e4m3fn)
        assert np.array_equal(back.view(torch.uint8).numpy(), codes), "not on the e4m3 grid at the stated scale"
        assert np.array_equal(back.to(torch.float64).numpy() * scale, x)
        assert np.array_equal(t.to(torch.bfloat16).to(torch.float64).numpy(), x), "not exact in bf16"
    for shift in (0, 32):
        q = case.q(3, 70, shift)
        assert np.array_equal(torch.from_numpy(q).to(torch.bfloat16).to(torch.float64).numpy(), q)
        assert (np.count_nonzero(q, axis=-1) == 1).all() and set(np.unique(q)) == {0.0, case.a}
        s64 = np.einsum("bid,jd->bij", q, case.k())
        s32 = np.einsum("bid,jd->bij", q.astype(np.float32), case.k().astype(np.float32))
        assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), s64), "a logit rounds in fp32"
        cols = (np.arange(70)[None, :] + shift * np.arange(3)[:, None]) % kc.D
        assert np.array_equal(s64, case.logits()[cols])
    if name != "lone_mover_large":
        assert np.abs(case.logits()).max() <= 64.0


@pytest.mark.parametrize("nk", NKS)
def test_pos_covers_every_half_block_and_the_edges(nk):
    at = [kc.pos(c, nk) for c in range(kc.D)]
    assert all(0 <= p < nk for p in at)
    assert {p // kc.HALF for p in at} == set(range(-(-nk // kc.HALF)))
    assert {p // kc.HALF for p in at[:70]} == set(range(-(-nk // kc.HALF))) or nk > 321     # nq = 70 rows of one head reach every half of nk = 321
    last_block = (nk - 1) // 64 * 64
    assert {0, min(31, nk - 1), min(32, nk - 1), nk - 1, last_block} <= set(at)
    assert at == [kc.pos(c, nk) for c in range(kc.D)]


def full(nk):
    return np.full(kc.D, nk - 1)


@pytest.mark.parametrize("nk", NKS)
def test_staircase_up_moves_every_maximum_in_every_full_step(nk):
    s = kc.make("staircase_up", nk).logits()
    assert kc.moves(s, full(nk)).all()
    where = np.array([[int(np.argmax(s[c, h * kc.HALF:(h + 1) * kc.HALF])) for h in range(-(-nk // kc.HALF))] for c in range(kc.D)])
    assert len(np.unique(where[:, 0])) > 8, "the peak of a half must not sit at one place for every column"
    for last in (nk // 2, nk - 2, 40 % nk):      # causal: every step the row sees in full moves its maximum
        mv = kc.moves(s, np.full(kc.D, last))
        assert mv[:, :(last + 1) // kc.HALF].all() and not mv[:, last // kc.HALF + 1:].any()


@pytest.mark.parametrize("nk", NKS)
def test_first_key_wins_moves_no_maximum_after_the_first_step(nk):
    s = kc.make("first_key_wins", nk).logits()
    assert (s[:, :1] > s[:, 1:]).all()
    for last in (nk - 1, nk // 2, 0):
        mv = kc.moves(s, np.full(kc.D, last))
        assert mv[:, 0].all() and not mv[:, 1:].any()


@pytest.mark.parametrize("nk", NKS)
@pytest.mark.parametrize("name", ["lone_mover", "lone_mover_large"])
def test_lone_mover_moves_only_the_rows_whose_spike_lies_in_the_step(name, nk):
    case = kc.make(name, nk)
    s = case.logits()
    at = np.array([kc.pos(c, nk) for c in range(kc.D)])
    halves = -(-nk // kc.HALF)
    want = np.zeros((kc.D, halves), dtype=bool)
    want[:, 0] = True
    want[np.arange(kc.D), at // kc.HALF] = True
    mv = kc.moves(s, full(nk))
    assert np.array_equal(mv, want)
    for b in range(kc.D // 32):                   # a 32-row block of consecutive columns: in no later step do all of its rows move
        cnt = mv[32 * b:32 * b + 32, 1:].sum(axis=0)
        assert (cnt < 32).all()
        if halves <= 12:
            assert ((cnt > 0) & (cnt < 32)).sum() >= (halves - 1) // 2, "steps in which a few rows move and the rest do not"
    assert mv.any(axis=0).all()                   # every step moves some row
    for c in range(kc.D):                         # the background alone: key 0 strictly above the rest, never rising
        b = np.delete(s[c], at[c])
        assert (np.diff(b) <= 0).all() and (at[c] == 0 or (b[0] > b[1:]).all())
    # causal: a spike above the row's diagonal is masked, and then only the first step moves
    mv = kc.moves(s, np.minimum(full(nk), at - 1).clip(0))
    assert mv[:, 0].all() and not mv[at > 0][:, 1:].any()
    # the size of delta
    spike, key0 = s[np.arange(kc.D), at], s[:, 0]
    c = at > 0
    if name == "lone_mover":
        ratio = np.exp(spike[c]) / (np.exp(s[c]).sum(axis=1) - np.exp(spike[c]))
        print(f"{name} nk={nk}: spike weight / background weight {ratio.min():.3f} .. {ratio.max():.3f}")
        # within 16x either way for 33 .. 1100 keys: a rescale skipped or applied wrongly misweighs at least 1/17 of O, orders above any bar
        assert (spike[c] - key0[c] == 5.875).all() and (ratio > 1 / 16).all() and (ratio < 16.0).all(), "comparable to the background's total"
    else:
        assert (spike[c] - key0[c] >= 2.0 ** 19).all() and (spike == 2.0 ** 20).all() and np.abs(np.delete(s[5], at[5])).max() <= 56.0


def test_late_start_leaves_whole_row_blocks_without_a_key_beside_blocks_with_one():
    p = kc.late_start()
    nq, nk, group, lens = p["nq"], p["nk"], p["group"], p["kv_lens"]
    assert max(lens) == nk and any(n < nq for n in lens) and len(lens) * group * nq <= 2000
    M = group * nq
    seen = {"empty beside seeing": 0, "cut": 0, "second of a wave only": 0}
    for n in lens:
        sees = np.array([(n - nq + r % nq) >= 0 for r in range(M)] + [False] * (-M % 64))     # packed row r, causal
        blocks = sees.reshape(-1, 32)
        some, every = blocks.any(axis=1), blocks.all(axis=1)
        seen["cut"] += int((some & ~every).sum())
        seen["empty beside seeing"] += int((~some[:-1] & some[1:]).sum())
        waves = some.reshape(-1, 2)
        seen["second of a wave only"] += int((~waves[:, 0] & waves[:, 1]).sum())
    assert all(seen.values()), seen
