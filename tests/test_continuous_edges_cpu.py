"""tests/continuous_edges.py on the CPU: the table is what it claims to be, its bars are attainable in fp32 (a float32 numpy evaluation of the reference
meets every one of them on every row that is not declared) and they can see the gap they were built for (the literal float32 ln(1 + e^x) misses the
sd bar on the `floor` group, by a factor of six).  No GPU."""
import json
import os

import numpy as np

from tests import beta_numpy as bn
from tests import continuous_edges as ce

G, B = ce.GAUSSIAN, ce.BETA
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "philox_extremes.json")


def test_the_table_is_fixed_and_holds_every_row_once():
    for policy in (G, B):
        p0, p1, a, g = ce.table(policy)
        assert 1500 <= len(a) <= 4000 and all(x.dtype == np.float32 for x in (p0, p1, a))
        keys = {np.array(r, dtype=np.float32).tobytes() for r in zip(p0, p1, a)}
        assert len(keys) == len(a), "a row twice"
        ce.table.cache_clear()                                                               # built again: the same rows in the same order
        q0, q1, qa, qg = ce.table(policy)
        assert all(x.tobytes() == y.tobytes() for x, y in zip((p0, p1, a), (q0, q1, qa))) and np.array_equal(g, qg)
        assert np.isfinite(p0).all() and np.isfinite(p1).all() and np.isfinite(a).all()
        n0, n1, na = ce.nonfinite(policy)
        assert np.all(~np.isfinite(n0) ^ ~np.isfinite(n1)) and np.isfinite(na).all(), "one non-finite preference at a time"
        for bad in (np.isnan, np.isposinf, np.isneginf):
            assert bad(n0).any() and bad(n1).any()


def test_every_group_is_there_for_both_policies():
    for policy in (G, B):
        g = ce.table(policy)[3]
        assert set(g) == set(ce.GROUPS), (policy, set(g))
        print({k: int((g == k).sum()) for k in ce.GROUPS})


def test_the_preferences_are_fp32_values_on_the_intended_side_of_ten():
    assert float(ce.B10) < 10.0 < float(ce.A10) and np.nextafter(ce.B10, np.float32(20)) == np.float32(10) == np.nextafter(ce.A10, np.float32(0))
    for policy, cols in ((G, (1,)), (B, (0, 1))):
        t = ce.table(policy)
        for k in cols:
            x = t[k]
            assert {float(ce.B10), 10.0, float(ce.A10)} <= set(x.astype(np.float64)), "both sides of the switch and the switch itself"
            assert np.array_equal(x.astype(np.float64).astype(np.float32), x)
            # the side decides the branch: Softplus is the identity from 10 on and ln(1 + e^x) below
            sp = bn.softplus(x.astype(np.float64))
            assert np.all(sp[x >= 10] == x[x >= 10]) and np.all(sp[x < 10] > x[x < 10])
    xs = set(ce.table(G)[1].astype(np.float64))
    assert {float(np.float32(v)) for v in ce.XS} == xs
    xm = set(ce.table(G)[0].astype(np.float64))
    assert {float(np.float32(v)) for v in ce.XM} == xm and np.signbit(ce.table(G)[0][ce.table(G)[0] == 0]).any()
    a, g = ce.table(B)[2], ce.table(B)[3]
    for v in (0.0, 2.0 ** -149, 2.0 ** -25, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0, -0.5, 1.5):
        assert np.any(a == np.float32(v)), v
    assert np.signbit(a[a == 0]).any()


def test_float32_numpy_meets_the_sd_bar_and_the_literal_softplus_does_not():
    _, xs, _, g = ce.table(G)
    want = ce.sd64(xs)
    good, literal = ce.rel_self(ce.sd32(xs), want), ce.rel_self(ce.sd32(xs, literal=True), want)
    print("sd relative to sd: log1p %.4g (recorded %.4g, bar %.4g); literal %.4g, on the floor group %.4g at x_s = %g" %
          (good.max(), ce.SD_NUMPY, ce.sd_bar(), literal.max(), literal[g == "floor"].max(), xs[g == "floor"][literal[g == "floor"].argmax()]))
    assert good.max() <= ce.sd_bar()                                                         # attainable ...
    assert good.max() <= 2 * ce.SD_NUMPY, "the recorded figure is no longer this numpy's: measure it again"      # (another libm may differ by an ulp or two)
    assert literal[g == "floor"].max() > ce.sd_bar(), "the bar cannot see the literal form's error at the floor"
    assert literal[g == "floor"].max() > 5e-6                                                # (the issue's figure: 5.99e-6 on a dense sweep)
    # ... while under the old normalisation, |d sd| / max(1, sd), the same error is 6e-8: invisible to a 5e-7 bound
    assert np.max(np.abs(ce.sd32(xs, literal=True).astype(np.float64) - want)[g == "floor"]) < 1e-7


def _gauss_figures(literal):
    p0, p1, a, g = ce.table(G)
    gid = ce.OFFSET + np.arange(len(a))
    got = ce.gauss_f32(p0, p1, a, literal=literal)
    u = ce.stage_b(G, p0, p1, a, got)
    z, rad = ce.normal_parts(ce.SEED, gid, 0, bn.BLK_API)
    with np.errstate(over="ignore", invalid="ignore"):
        smp = (got["sd"] * ce.normal32(ce.SEED, gid, 0, bn.BLK_API) + got["mu"]).astype(np.float32)
    u["sample"] = ce.units(smp, *ce.gauss_sample_b(got["mu"], got["sd"], z, rad))
    return u, g


def test_the_recorded_numpy_figures_are_the_literal_reference_on_the_rows_it_can_evaluate():
    u, g = _gauss_figures(literal=True)
    for q, v in u.items():
        fig = v[g != "range"].max()
        print("gaussian %s: %.4g units of 2^-24 cond (recorded %.4g)" % (q, fig, ce.K_NUMPY[(G, q)]))
        assert fig <= 2 * ce.K_NUMPY[(G, q)], "the recorded figure is no longer this numpy's: measure it again"       # (loose: another libm may differ)
    assert np.isinf(u["cs"][g == "range"]).any(), "the literal form overflows nowhere: the `range` group is empty of its purpose"
    p0, p1, a, g = ce.table(B)
    u = ce.stage_b(B, p0, p1, a, ce.beta_f32(p0, p1, a))
    for q, v in u.items():
        print("beta %s: %.4g units of 2^-24 cond (recorded %.4g)" % (q, v.max(), ce.K_NUMPY[(B, q)]))
        assert v.max() <= 2 * ce.K_NUMPY[(B, q)], "the recorded figure is no longer this numpy's: measure it again"


def test_float32_numpy_meets_every_bar_on_every_row_that_is_not_declared():
    """the rearranged Gaussian form (no square before the division) and the Beta formulas as they stand, each at its OWN fp32 parameters"""
    u, _ = _gauss_figures(literal=False)
    for q, v in u.items():
        fig = v[~ce.declared_mask(G, q)].max()
        print("gaussian %s: %.4g (bar %.4g)" % (q, fig, ce.bar(G, q)))
        assert fig <= ce.bar(G, q), (q, fig)
    p0, p1, a, _ = ce.table(B)
    got = ce.beta_f32(p0, p1, a)
    al, be = bn.beta_params(p0.astype(np.float64), p1.astype(np.float64))
    assert ce.rel_self(got["alpha"], al).max() <= ce.PARAM_BAR and ce.rel_self(got["beta"], be).max() <= ce.PARAM_BAR
    # Beta keeps the literal ln(1 + e^x) on the device (its agents' runs keep their bits): beside the + 1 it meets the same bar
    lit = (ce.softplus32(p0, literal=True) + np.float32(1.0)).astype(np.float32)
    print("alpha, literal Softplus: %.4g (bar %.4g)" % (ce.rel_self(lit, al).max(), ce.PARAM_BAR))
    assert ce.rel_self(lit, al).max() <= ce.PARAM_BAR
    for q, v in ce.stage_b(B, p0, p1, a, got).items():
        fig = v[~ce.declared_mask(B, q)].max()
        print("beta %s: %.4g (bar %.4g)" % (q, fig, ce.bar(B, q)))
        assert fig <= ce.bar(B, q), (q, fig)


def test_units_states_the_rules_of_the_range_rows():
    big, tiny = 1e39, 1e-46
    u = ce.units(np.float32([np.inf, 3e38, -np.inf, np.inf, 0.0, 1e-45, np.nan, 1.0, 0.0, 1e-10]),
                 np.array([big, big, -big, -big, tiny, tiny, np.nan, np.nan, 0.0, 0.0]), np.array([big, big, big, big, tiny, tiny, 1.0, 1.0, 0.0, 1.0]))
    assert list(u[:8]) == [0.0, np.inf, 0.0, np.inf, 0.0, np.inf, 0.0, np.inf] and u[8] == 0.0 and 0 < u[9] < np.inf      # (u[9]: an exact cancellation is no underflow)


def test_the_declared_rows_are_few_and_each_has_its_reason():
    for policy in (G, B):
        n = len(ce.table(policy)[0])
        total = np.zeros(n, dtype=bool)
        for q, entries in ce.declared(policy).items():
            assert (policy, q) in ce.K_NUMPY
            for mask, rule in entries:
                assert mask.dtype == bool and mask.shape == (n,) and mask.any() and len(rule) > 20
                total |= mask
        print("declared: %d of %d rows" % (total.sum(), n))
        assert total.sum() <= 0.02 * n


def test_the_f64_beta_sampler_leaves_out_at_most_five_percent_of_the_table():
    p0, p1, a, _ = ce.table(B)
    al, be = bn.beta_params(p0.astype(np.float64), p1.astype(np.float64))
    for t in range(2):
        x, margin = bn.beta_sample(ce.SEED, ce.OFFSET + np.arange(len(a)), t, bn.BLK_API, al, be)
        assert (margin < ce.BETA_MARGIN).mean() <= ce.BETA_LEFT_OUT and np.all((x >= bn.LO) & (x <= bn.HI))


def test_the_driver_loop_rows_have_finite_coefficients_at_any_sample():
    for policy in (G, B):
        keep = ce.finite_coefficients(policy)
        p0, p1 = (x[keep] for x in ce.table(policy)[:2])
        assert len(p0) >= 20 and len({(float(x), float(y)) for x, y in zip(p0, p1)}) == len(p0)
        if policy == G:                                                                     # |a - mu| <= 5.77 sd: |c_m| <= 5.77 / sd, |c_s| <= 17 / sd^2
            assert float(np.max(5.77 / ce.sd64(p1))) < 1e3 and set(ce.SWITCH) <= set(p1.astype(np.float64))


def test_the_philox_fixture_re_derives():
    with open(GOLDEN) as f:
        fix = json.load(f)
    assert fix["t"] == 0 and fix["block_word"] == bn.BLK_API + 256
    seen = {}
    for h in fix["hits"]:
        w = bn.philox_block(h["seed"], np.array([h["id"]]), 0, bn.BLK_API + 256)[0]
        assert [int(v) for v in w] == h["words"], h
        x, y = int(w[0]) >> 8, int(w[1]) >> 8
        ok = {"u1_min": x <= 3, "u1_one": x == (1 << 24) - 1, "u2_zero": y == 0, "u2_quarter": abs(y - (1 << 22)) <= 16,
              "u2_three_quarters": abs(y - 3 * (1 << 22)) <= 16}[h["class"]]
        assert ok and 0 <= h["id"] < 1 << 24, h
        seen[h["class"]] = seen.get(h["class"], 0) + 1
    assert set(seen) == {"u1_min", "u1_one", "u2_zero", "u2_quarter", "u2_three_quarters"} and min(seen.values()) >= 2 and len(fix["hits"]) <= 40, seen
    assert sum(h["class"] == "u1_min" and h["words"][0] >> 8 == 0 for h in fix["hits"]) >= 2, "u1 = 2^-24 itself"
