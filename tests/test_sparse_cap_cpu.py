"""What the cap on the sparse trace costs, on the CPU: the oracle's capped list (orc_run_train_sparse_lambda: 512 entries per learner, 512 / T per tiling,
the smallest |v| overwritten) against the reference's unbounded trace rebuilt from the oracle's own tape, held to the bound B of tests/sparse_lambda_numpy.py:
    0 <= z_capped <= z_ref elementwise,      ||z_ref - z_capped||_1 <= B per (learner, tiling)
-- in f64 to rounding, in f32d with the fp32 slack u(z) = 2 * 2^-23 / (1 - rate) * max(1, z_ref) per entry -- and the restated loop itself against the
oracle's while nothing is evicted (all three rules, both agents)."""
import numpy as np
import pytest

from tests.sparse_lambda_numpy import DenseLambdaTeacher, DenseTraces, CutWatch, deficit, follow_tape, fp32_slack, trace_rate

MC = dict(domain=0, tiles_per_dim=8, algo=3, policy=1, epsilon=0.3, gamma=0.99, max_episode_steps=0)
EVICTING = {
    "t8_dutch": (64, 900, dict(MC, n_tilings=8, lam=0.97, trace=2)),
    "t16_saturate": (77, 500, dict(MC, n_tilings=16, lam=0.95, trace=1)),
    "t16_accumulate": (32, 400, dict(MC, n_tilings=16, lam=0.95, trace=0)),
}
LEGS = dict(EVICTING, not_evicting=(32, 600, dict(MC, n_tilings=4, tiles_per_dim=10, lam=0.97, trace=0)))      # 128 slots per sub-list: none fills


@pytest.mark.parametrize("prec", ["f64", "f32d"])
@pytest.mark.parametrize("leg", list(LEGS))
def test_capped_trace_is_within_the_bound_of_the_unbounded_one(orc, leg, prec):
    N, K, kw = LEGS[leg]
    T = kw["n_tilings"]
    kw = dict(kw, alpha=0.1 / T / N)
    ag = orc.make_agent(**dict(kw, basis=orc.TILE, shared_w=True, seed=7))
    run = orc.Run(ag, N, prec)
    run.reset()
    rate = trace_rate(kw["gamma"], kw["lam"], kw["alpha"], kw["trace"])
    tr = DenseTraces(N, T, run.F, run.A, rate, kw["trace"])
    worst = dict(DB=0.0, Bz=0.0, Dz=0.0, over=-np.inf, held=0)
    for k in range(K):
        follow_tape(orc, ag, tr, run.teacher_step_sparse_lambda())
        if (k + 1) % 50 and k + 1 != K:
            continue
        z = np.stack([run.sparse_trace(i) for i in range(N)]).astype(np.float64)
        D, diff = deficit(tr, z)
        Zt, l1 = tr.tilings(), tr.tilings().sum(-1)
        assert z.min() >= 0 and not np.any((z != 0) & (tr.Z == 0))                     # inside the reference's support
        if prec == "f64":                                                               # (1e-12 per held entry: the roundings of the two f64 loops)
            u, slack = 1e-12, 1e-12 * tr.live
            assert np.all(D <= tr.B * (1 + 1e-9) + slack), (k, (D - tr.B).max())
        else:
            u, slack = fp32_slack(Zt, rate), tr.slack()
            assert np.all(D <= tr.B + slack), (k, (D - tr.B - slack).max())
        assert np.all(diff <= u), (k, (diff - u).max())
        has = tr.B > 0
        worst["DB"] = max(worst["DB"], float((D[has] / (tr.B + slack)[has]).max()) if has.any() else 0.0)
        worst["Bz"] = max(worst["Bz"], float((tr.B[l1 > 0] / l1[l1 > 0]).max()))
        worst["Dz"] = max(worst["Dz"], float((D[l1 > 0] / l1[l1 > 0]).max()))
        worst["held"] = max(worst["held"], int((z != 0).sum((1, 2)).max()))
    print(f"sparse cap {leg} {prec}: D/(B+slack) {worst['DB']:.3f}  B/|z| {worst['Bz']:.2e}  D/|z| {worst['Dz']:.2e}  held {worst['held']}")
    if leg in EVICTING:
        assert worst["held"] == 512                                                     # the cap did take effect
        assert 0 < worst["Bz"] <= 0.1, worst["Bz"]                                      # and the bound says something
    else:
        assert worst["Bz"] == 0 and worst["held"] < 512


Q_CP = dict(domain=1, n_tilings=8, tiles_per_dim=5, algo=4, policy=1, epsilon=0.2, gamma=0.99, lam=0.8, trace=1, max_episode_steps=60)
Q_ACRO = dict(domain=2, n_tilings=4, tiles_per_dim=6, algo=4, policy=2, tau=0.5, gamma=0.95, lam=0.7, trace=0, max_episode_steps=50)
RESTATED = [("cartpole_q_saturate", 48, 200, 2.0, Q_CP), ("acrobot_q_accumulate_softmax", 48, 120, 0.1, Q_ACRO),
            ("mountaincar_sarsa_dutch", 32, 60, 0.1, dict(MC, n_tilings=16, lam=0.97, trace=2))]


@pytest.mark.parametrize("name,N,K,a,kw", RESTATED, ids=[c[0] for c in RESTATED])
def test_restated_loop_is_the_oracles_while_nothing_is_evicted(orc, name, N, K, a, kw):
    # the numpy loop the GPU tests use as their teacher against orc_run_teacher_sparse_lambda in f64: the same tape, the same table, the same traces -- and, for
    # Q(lambda), the seeds of tests/test_gpu_sparse_cap.py leave at most 5 % of the learner-steps out of a trace comparison (CutWatch)
    kw = dict(kw, alpha=a / kw["n_tilings"] / N)
    te = DenseLambdaTeacher(orc, N, 3, **kw)
    run = orc.Run(te.ag, N, "f64")
    run.reset()
    watch = CutWatch(N)
    for k in range(K):
        o, t = te.step(), run.teacher_step_sparse_lambda()
        for f in ("frm", "action", "reward", "to", "terminal"):
            assert np.array_equal(o[f], t[f]), (k, f)
        assert np.allclose(o["td"], t["td"], rtol=0, atol=1e-12)
        assert o["B"].max() == 0
        watch.step(o)
    assert np.allclose(run.weights, te.W, rtol=0, atol=1e-13) and np.abs(te.W).max() > 0
    for i in range(N):
        assert np.allclose(run.sparse_trace(i), te.tr.Z[i], rtol=0, atol=1e-13)
    if kw["algo"] == 4:
        assert 0 < watch.fraction <= 0.05, watch.fraction
