"""The crafted-state tables of tests/state_edges.py on the CPU: the oracle's device-order instantiation (f32d: the device's polynomials and operation
order, what tests/test_gpu_state_edges.py compares the HIP path with bit for bit) against f64 at the measured bars, with the three decision assertions;
against _f32 at the recorded figure; the tile coder against a plain numpy restatement; and the tables' own hygiene (every class present, every clip,
wrap direction and threshold actually crossed according to f64, the recorded figures the measured ones, at most 5 % of a domain's pairs undecided)."""
import numpy as np
import pytest

from tests import state_edges as se

F32, F64 = np.float32, np.float64
CLASSES = {
    se.MC: {"bound", "zero", "scaled", "out", "limit", "cross", "quadrant", "goal", "wall", "vclip", "start"},
    se.CP: {"bound", "zero", "scaled", "out", "limit", "clip", "thr", "onthr"},
    se.AC: {"bound", "zero", "scaled", "out", "wrap", "pi", "vclip", "line"},
}
CLASSES[se.CMC] = CLASSES[se.MC]


sets = se.sets


def close(measured, recorded):
    return abs(measured - recorded) <= 0.01 * recorded + 1e-12


@pytest.mark.parametrize("domain", se.DOMAINS)
def test_table_hygiene(domain):
    S, names = se.table(domain)
    D, n = S.shape
    assert n % 64 != 0 and 64 < n <= 600 and np.all(np.isfinite(S))
    assert len(np.unique(se.bits(S), axis=1).T) == n                                   # no row twice (by bit pattern: 0.0 and -0.0 are two rows)
    assert set(se.classes(domain)) >= CLASSES[domain], CLASSES[domain] - set(se.classes(domain))
    lo64, hi64, lo, hi = se.bounds(domain)
    for d in range(D):
        col = S[d]
        for v in (lo[d], hi[d], np.nextafter(lo[d], hi[d]), np.nextafter(hi[d], lo[d]), np.nextafter(lo[d], F32(-np.inf)), np.nextafter(hi[d], F32(np.inf)), se.SUB):
            assert np.any(se.bits(col) == se.bits(F32(v))), (d, v)
        assert np.any(se.bits(col) == 0) and np.any(se.bits(col) == 0x80000000)        # 0.0 and -0.0
        # the scaled positions: the fp32 s~ (the device's (s - lo) * fl(1 / (hi - lo))) IS p, or p's two neighbours are both there (MountainCar's
        # x never gives 3/4 exactly: 0.74999994 and 0.75000006 are adjacent results)
        sc = ((col - lo[d]).astype(F32) * (F32(1.0) / F32(hi[d] - lo[d]))).astype(F32)
        for p in (0.0, 0.25, 0.5, 0.75, 1.0):
            p = F32(p)
            assert np.any((sc >= np.nextafter(p, F32(-1.0))) & (sc <= p)) and np.any((sc >= p) & (sc <= np.nextafter(p, F32(2.0)))), (d, p)
        w = hi64[d] - lo64[d]
        for f in (0.5, 3.0):
            assert np.any(col == F32(lo64[d] - f * w)) and np.any(col == F32(hi64[d] + f * w)), (d, f)
    if domain != se.AC:                                                                # one row at the ABI's admission limit (1000 widths)
        assert np.any(S == F32(lo64[0] - 1000.0 * (hi64[0] - lo64[0])))
    else:
        assert np.all(np.abs(S[:2]) <= 7.0 * np.pi * (1.0 + 1e-6))                     # no angle beyond 3 widths


@pytest.mark.parametrize("domain", (se.MC, se.CMC))
def test_mountain_car_rows_cross_what_they_name(domain):
    S, names = se.table(domain)
    a = se.answers(domain, "f64")
    raw, cls = a["raw"], np.array([n.split(":")[0] for n in names])
    assert np.any(raw[..., 0] > 0.6) and np.any(raw[..., 0] < -1.2) and np.any(raw[..., 1] > 0.07) and np.any(raw[..., 1] < -0.07)
    for c, edge, k in (("goal", 0.6, 0), ("wall", -1.2, 0), ("vclip", 0.07, 1), ("vclip", -0.07, 1)):
        r = raw[cls == c][..., k]
        e32, u = float(F32(edge)), float(np.spacing(F32(abs(edge))))
        places = np.round((r - e32) / u)
        near = np.abs(r - e32 - places * u) < 0.26 * u                                 # lands ON the place (the crafted v is rounded: within a quarter)
        for j in range(-2, 3):
            assert np.any(near & (places == j)), (c, edge, j)
    assert np.any(se.bits(S[0]) == se.bits(F32(0.6))) and a["term"][S[0] == F32(0.6)].any()
    assert np.any(a["term"]) and not np.all(a["term"])
    t = 3.0 * S[0].astype(F64) / (np.pi / 2.0)                                         # sincos_cw's n = rint(3x * 2 / pi): both sides of each tie
    for tie in (0.5, -0.5, 1.5, -1.5):
        assert np.any((t > tie - 1e-6) & (t < tie)) and np.any((t < tie + 1e-6) & (t > tie)), tie


def test_cart_pole_rows_cross_what_they_name():
    a = se.answers(se.CP, "f64")
    raw = a["raw"]
    for k, b in ((1, 6.0), (3, 2.0), (0, 2.4), (2, se.TW64)):
        for sgn in (1.0, -1.0):
            m = sgn * raw[..., k] - b                                                  # > 0: past the clip / threshold on that side
            assert np.any(m > 1e-3) and np.any(m < -1e-3), (k, sgn)
            assert np.any((m > 0) & (m < 1e-6)) and np.any((m < 0) & (m > -1e-6)), (k, sgn, m[np.abs(m) < 1e-5])
    S, names = se.table(se.CP)
    on = np.array([n.startswith("onthr") for n in names])
    assert a["term"][on].any() and np.any(S[0] == F32(2.4)) and np.any(S[0] == F32(-2.4)) and np.any(S[2] == F32(se.TW64)) and np.any(S[2] == -F32(se.TW64))


def test_acrobot_rows_cross_what_they_name():
    a = se.answers(se.AC, "f64")
    raw = a["raw"]
    up1, dn1, up2, dn2 = raw[..., 0] > np.pi, raw[..., 0] < -np.pi, raw[..., 1] > np.pi, raw[..., 1] < -np.pi
    assert up1.any() and dn1.any() and up2.any() and dn2.any()
    assert np.any(up1 & up2) and np.any(dn1 & dn2) and np.any(up1 & dn2) and np.any(dn1 & up2)
    for k, b in ((2, 4.0 * np.pi), (3, 9.0 * np.pi)):
        for sgn in (1.0, -1.0):
            m = sgn * raw[..., k] - b
            assert np.any((m > 0) & (m < 1e-4)) and np.any((m < 0) & (m > -1e-4)) and np.any(m > 1e-2) and np.any((m < -1e-2) & (m > -1.0)), (k, sgn)
    S, names = se.table(se.AC)
    for d in (0, 1):
        assert np.any(S[d] == se.PI32) and np.any(S[d] == -se.PI32)
    line = np.array([n.startswith("line") for n in names])
    q, band = se.margin(se.AC)[line], se.band(se.AC)[line][:, None]
    assert np.any((q > 0) & (q < 1e-6)) and np.any((q < 0) & (q > -1e-6)) and np.any(q > band) and np.any(q < -band)


@pytest.mark.parametrize("domain", se.DOMAINS)
def test_recorded_f32_figures_are_the_measured_ones(domain):
    a64, a32, ad = (se.answers(domain, p) for p in ("f64", "f32", "f32d"))
    for which, m in sets(domain):
        got = se.err(domain, a32["next"], a64["next"])[m].max()
        print("domain %d %s: _f32 / f64 %.4g (recorded %.4g, bar %.4g)" % (domain, which, got, se.F32_STEP[(domain, which)], se.step_bar(domain, which)))
        assert close(got, se.F32_STEP[(domain, which)]), (which, got)
    for order in se.PHI_ORDERS[domain]:
        for which, m in sets(domain):
            got = np.abs(se.phi(domain, order, "f32") - se.phi(domain, order, "f64"))[:, m].max()
            print("domain %d order %d %s: _f32 / f64 %.4g (bar %.4g)" % (domain, order, which, got, se.phi_bar(domain, order, which)))
            assert close(got, se.F32_PHI[(domain, order, which)]), (order, which, got)


@pytest.mark.parametrize("domain", se.DOMAINS)
def test_f32d_transition_against_f64_and_f32(domain):
    S, names = se.table(domain)
    a64, a32, ad = (se.answers(domain, p) for p in ("f64", "f32", "f32d"))
    e = se.err(domain, ad["next"], a64["next"]).max(axis=(1, 2))
    bars = se.row_bars(domain)
    for which, m in sets(domain):
        print("domain %d %s: f32d / f64 %.4g (bar %.4g)" % (domain, which, e[m].max(), se.step_bar(domain, which)))
    assert np.all(e <= bars), (names[e > bars], e[e > bars])
    e32 = se.err(domain, ad["next"], a32["next"].astype(F64)).max(axis=(1, 2))
    for which, m in sets(domain):
        print("domain %d %s: f32d / _f32 %.4g (recorded %.4g)" % (domain, which, e32[m].max(), se.DEV_F32[(domain, which)]))
        assert e32[m].max() <= 1.01 * se.DEV_F32[(domain, which)] + 1e-12, (which, e32[m].max())
    # the decisions
    assert np.array_equal(ad["term"], se.predicate(domain, ad["next"], "f32d"))
    assert np.array_equal(se.bits(ad["reward"]), se.bits(se.reward_of(domain, ad["term"])))
    ok = se.decided(domain)
    assert np.array_equal(ad["term"][ok], a64["term"][ok]), names[np.any((ad["term"] != a64["term"]) & ok, axis=1)]


@pytest.mark.parametrize("domain", se.DOMAINS)
def test_at_most_five_per_cent_of_the_pairs_are_left_undecided(domain):
    und = ~se.decided(domain)
    print("domain %d: %d of %d pairs inside the band: %s" % (domain, und.sum(), und.size, sorted(set(se.table(domain)[1][und.any(axis=1)]))))
    assert und.mean() <= se.LEFT_OUT, und.mean()


@pytest.mark.parametrize("domain,order", [(d, o) for d in se.DOMAINS for o in se.PHI_ORDERS[d]])
def test_f32d_features_against_f64(domain, order):
    pd, p64 = se.phi(domain, order, "f32d"), se.phi(domain, order, "f64")
    e = np.abs(pd - p64).max(axis=0)
    for which, m in sets(domain):
        print("domain %d order %d %s: f32d / f64 %.4g (bar %.4g)" % (domain, order, which, e[m].max(), se.phi_bar(domain, order, which)))
    assert np.all(e <= se.phi_row_bars(domain, order)), se.table(domain)[1][e > se.phi_row_bars(domain, order)]
    assert np.all(se.bits(pd[-1]) == se.bits(F32(1.0)))
    if (se.basis_domain(domain), order) in se.PHI_CAP:
        assert se.phi_bar(domain, order, "in") <= se.PHI_CAP[(se.basis_domain(domain), order)]
    assert se.phi_bar(domain, order, "in") <= se.PHI_CAP_OTHER


@pytest.mark.parametrize("domain", (se.MC, se.CP, se.AC))
def test_tile_indices_against_the_numpy_restatement(orc, domain):
    for T, B in se.tile_configs(domain):
        S = se.tile_table(domain, T, B)
        assert S.shape[1] % 64 != 0
        ag = orc.make_agent(domain=domain, basis=orc.TILE, n_tilings=T, tiles_per_dim=B)
        got = np.stack([orc.tile_indices(ag, S[:, i]) for i in range(S.shape[1])], axis=1)
        want = se.tile_numpy(domain, T, B, S)
        assert np.array_equal(got, want), (T, B, np.argwhere(got != want)[:5])
        assert got.min() >= 0 and got.max() < T * B ** S.shape[0]
        if B > 1:                                                                      # (the rows spread over the cells: many distinct index vectors)
            assert len(np.unique(got, axis=1).T) > 4 * T
