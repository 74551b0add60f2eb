"""The decisiveness conditions of tests/policy_edges.py, checked without a GPU: on the crafted table the reference's f64 semantics alone decide every
discrete output (the f64 and the device-order fp32 oracle agree on every argmaxima set, find_max, find_min and mode index), so a device test may ask
for exact indices; the fp32 formulation of the Softmax probabilities stays within 3e-7 of f64 for tau > 0 and saturates where f64 does; and the share
of Softmax samples that the 2e-6 band around a cumulative probability leaves out is small.  Measured here: worst |p_f32d - p_f64| = 6.1e-8 / 1.18e-7 /
1.41e-7 at A = 2 / 3 / 4; left out 0 of 3 836 / 4 550 / 9 184 (vector, draw) pairs (expected share about 1e-5).

The last test records what the fp32 formulation does for a NEGATIVE temperature: exp((q - max q) / tau) has exponents >= 0 there and overflows once
(max q - min q) / |tau| > 88.7, where f64 still returns ordinary probabilities.  rsrl_hip_create therefore refuses tau < 0 (DESIGN "Limits that
remain"); the oracle restates the reference and keeps accepting it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_edges as pe  # noqa: E402

TABLES = [(2, False), (3, False), (4, False), (2, True), (3, True)]
IDS = ["A2", "A3", "A4", "A2-bf16", "A3-bf16"]


def same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize("A,bf16", TABLES, ids=IDS)
def test_table_is_fixed_and_every_group_is_there(A, bf16):
    Q, g = pe.table(A, bf16)
    assert Q.dtype == np.float32 and Q.shape[1] == A and 200 <= len(Q) <= 700
    assert set(g) == {"tie", "chain", "mag", "nonfinite", "spread"}
    assert len({q.tobytes() for q in Q}) == len(Q)
    if bf16:
        assert pe.is_bf16(Q)
    assert pe.moderate(Q).sum() >= 100
    nomax = [q for q in Q if pe.no_maximum(q)]
    assert len(nomax) >= 2 + A                                  # all NaN, all -inf, and the mixed ones
    with np.errstate(invalid="ignore"):
        assert any(np.isnan(q[0]) and np.isfinite(q[1:]).all() for q in Q) and any(q[0] == -np.inf and np.isfinite(q[1:]).all() for q in Q)


@pytest.mark.parametrize("A,bf16", TABLES, ids=IDS)
def test_discrete_outputs_agree_between_f64_and_the_fp32_formulation(orc, A, bf16):
    Q, _ = pe.table(A, bf16)
    for q in Q:
        s64, s32 = orc.argmaxima(q, "f64")[0], orc.argmaxima(q, "f32d")[0]
        assert s64 == s32, (q, s64, s32)
        assert (len(s64) == 0) == pe.no_maximum(q), q
        (i64, v64), (i32, v32) = orc.find_max(q, "f64"), orc.find_max(q, "f32d")
        assert i64 == i32 and same(np.float32(v64), np.float32(v32)), q
        assert pe.find_max(q.astype(np.float64))[0] == i64                      # the helper's transcription of core.rs against the oracle's
        (j64, w64), (j32, w32) = pe.find_min(q.astype(np.float64)), pe.find_min(q)
        assert j64 == j32 and same(np.float32(w64), w32), q
        for pol in (pe.GREEDY, pe.EGREEDY):
            assert orc.policy_mode(pol, q, prec="f64") == orc.policy_mode(pol, q, prec="f32d") == i64
        for tau in pe.TAUS:
            assert orc.policy_mode(pe.SOFTMAX, q, tau=tau, prec="f64") == orc.policy_mode(pe.SOFTMAX, q, tau=tau, prec="f32d"), (q, tau)


@pytest.mark.parametrize("A,bf16", TABLES, ids=IDS)
def test_no_maximum_rule_is_the_oracles_too(orc, A, bf16):
    """the written-out rule of policy_edges (no maximum: mulhi(x, A) among all actions, greedy part 0) is what both oracle instantiations compute"""
    Q, _ = pe.table(A, bf16)
    xs = [orc.draw(7, 40 + k, 0, orc.BLK_API) for k in range(8)]
    for q in Q:
        if not pe.no_maximum(q):
            continue
        for pol in (pe.GREEDY, pe.EGREEDY):
            want = pe.ref_probs(orc, pol, q)
            assert np.array_equal(want, np.zeros(A) if pol == pe.GREEDY else np.full(A, pe.EPSILON / A))
            for prec in ("f64", "f32d"):
                assert np.allclose(orc.policy_probs(pol, q, eps=pe.EPSILON, prec=prec), want, rtol=0, atol=1e-7)
                for x in xs:
                    assert orc.policy_sample(pol, q, x, eps=pe.EPSILON, prec=prec) == pe.ref_sample(orc, pol, q, x)


@pytest.mark.parametrize("A,bf16", TABLES, ids=IDS)
def test_softmax_probabilities_of_the_fp32_formulation(orc, A, bf16):
    Q, _ = pe.table(A, bf16)
    worst, nsat = 0.0, 0
    dmax = np.finfo(np.float64).max
    for q in Q:
        for tau in pe.TAUS:
            p64 = orc.policy_probs(pe.SOFTMAX, q, tau=tau, prec="f64")
            p32 = orc.policy_probs(pe.SOFTMAX, q, tau=tau, prec="f32d")
            sat = p64 == dmax
            nsat += int(sat.any())
            assert np.all(p32[sat] == pe.FLT_MAX) and not np.any(p32[~sat] == pe.FLT_MAX), (q, tau, p64, p32)
            if (~sat).any():
                worst = max(worst, float(np.abs(p64[~sat] - p32[~sat]).max()))
    print(f"A={A} bf16={bf16}: worst |p_f32d - p_f64| = {worst:.3g} over {len(Q) * len(pe.TAUS)} (vector, tau) pairs; {nsat} saturate")
    assert worst <= 3e-7, worst
    assert nsat > 0


@pytest.mark.parametrize("A,bf16", TABLES, ids=IDS)
def test_softmax_sample_left_out_share(orc, A, bf16):
    """f64 oracle and orc.draw alone: how many (vector, draw) pairs have u within 2e-6 of a cumulative probability (expected about
    2 * 2e-6 * (A - 1) where the probabilities are ordinary, less on the saturated part of the table)"""
    Q, _ = pe.table(A, bf16)
    out = total = 0
    for tau in pe.TAUS:
        for i, q in enumerate(Q):
            for call in range(2):
                total += 1
                out += pe.softmax_in_band(orc, q, orc.draw(11, 5000 + i, call, orc.BLK_API), tau)
    print(f"A={A} bf16={bf16}: left out {out} of {total} = {out / total:.3g}")
    assert out / total <= 1e-3


@pytest.mark.parametrize("tau,q", [(-1.0, (0.0, 89.0, 1.0)), (-0.05, (0.0, 4.5, 1.0))])
def test_negative_temperature_overflows_the_fp32_formulation(orc, tau, q):
    p64 = orc.policy_probs(pe.SOFTMAX, q, tau=tau, prec="f64")
    assert np.all(np.isfinite(p64)) and np.all(p64 < 1.0) and abs(p64.sum() - 1.0) < 1e-12
    for prec in ("f32", "f32d"):
        p32 = orc.policy_probs(pe.SOFTMAX, q, tau=tau, prec=prec)
        assert p32[0] == pe.FLT_MAX and p32[1] == 0.0 and p32[2] == 0.0, (prec, p32)
        xs = [orc.draw(1, k, 0, orc.BLK_API) for k in range(64)]
        assert all(orc.policy_sample(pe.SOFTMAX, q, x, tau=tau, prec=prec) == 0 for x in xs)             # every sample is action 0
        if p64[2] > 0.01:                                                                                # (tau = -1: 0.27 of the reference's samples are action 2)
            assert len({orc.policy_sample(pe.SOFTMAX, q, x, tau=tau, prec="f64") for x in xs}) > 1
