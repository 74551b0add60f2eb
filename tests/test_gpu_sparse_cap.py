"""What the cap on the sparse trace costs, on the device: SARSALambda / QLambda over one shared tile table (rsrl_amd/csrc/kernels_sparse_lambda.hpp: 512 entries
per learner, 512 / T per tiling, the smallest |v| overwritten) against the reference's UNBOUNDED trace (traces.rs:188-240 over params/sparse.rs:13-97).
The teacher is the f64 numpy loop with dense traces of tests/sparse_lambda_numpy.py; every batch-step goes to the device through Handler::handle (transition i =
learner i), so both sides learn from identical inputs, and the device's lists are read back every 50 steps and at the end.
  not evicting (the bound B is 0 throughout): the device IS the reference's rule to fp32 rounding -- all three trace rules, Watkins's cut, 4 / 8 / 16 tilings;
  evicting: 0 <= z_dev <= z_ref elementwise and ||z_ref - z_dev||_1 <= B per (learner, tiling), B computed from the reference's trace alone, and the table
  within the ceiling that follows from B.  Measured figures: profiles/sparse_cap_cost.md."""
import numpy as np
import pytest

from tests.sparse_lambda_numpy import CutWatch, DenseLambdaTeacher, deficit, fp32_slack

pytestmark = pytest.mark.gpu

READ_EVERY = 50


@pytest.fixture(scope="module")
def ra():
    import rsrl_amd
    return rsrl_amd


def run_leg(ra, orc, N, K, a, kw, evicting):
    """K teacher-forced batch-steps -> the worst figures over the run (the assertions on the traces are made here, at every read)"""
    T = kw["n_tilings"]
    kw = dict(kw, alpha=a / T / N)
    te = DenseLambdaTeacher(orc, N, 3, **kw)
    tr, watch = te.tr, CutWatch(N)
    fig = dict(td=0.0, DB=0.0, Dz=0.0, Bz=0.0, z=0.0, held=0, ceiling=0.0, B=0.0)
    with ra.Context(basis=ra.TILE_CODING, weight_mode=ra.W_SHARED, seed=3, n_envs=N, **kw) as c:
        assert (c.F, c.A) == (te.F, te.A)
        c.reset()
        for k in range(K):
            o = te.step(want_slack=evicting)
            frm, to = np.ascontiguousarray(o["frm"].T, dtype=np.float32), np.ascontiguousarray(o["to"].T, dtype=np.float32)
            td = c.handle(frm, o["action"], o["reward"].astype(np.float32), to, o["terminal"]).astype(np.float64)
            fig["td"] = max(fig["td"], float(np.max(np.abs(td - o["td"]) / (1 + np.abs(o["td"])))))
            fig["B"] = max(fig["B"], float(o["B"].max()))
            if evicting:                                                               # what this step's update can have moved the table apart by
                fig["ceiling"] += kw["alpha"] * float(np.sum(np.abs(td - o["td"]) * o["z_l1"] + np.abs(td) * (o["B"].sum(1) + o["slack"].sum(1))))
            out = watch.step(o) if kw["algo"] == 4 else watch.out
            if (k + 1) % READ_EVERY and k + 1 != K:
                continue
            z = np.stack([c.get_traces(i) for i in range(N)]).astype(np.float64)
            D, diff = deficit(tr, z)
            Zt, l1 = tr.tilings(), tr.tilings().sum(-1)
            u, slack = fp32_slack(Zt, te.rate), tr.slack()
            ok = ~out
            assert z.min() >= 0 and not np.any((z != 0) & (tr.Z == 0))                 # the support of z_dev lies inside z_ref's
            assert np.all(diff[ok] <= u[ok]), (k, float((diff - u)[ok].max()))          # z_dev <= z_ref + u
            if evicting:
                assert np.all(D <= tr.B + slack), (k, float((D - tr.B - slack).max()))
                fig["DB"] = max(fig["DB"], float((D / (tr.B + slack))[l1 > 0].max()))
                fig["Bz"] = max(fig["Bz"], float((tr.B[l1 > 0] / l1[l1 > 0]).max()))
                fig["Dz"] = max(fig["Dz"], float((D[l1 > 0] / l1[l1 > 0]).max()))
            else:
                assert np.all(np.abs(diff[ok]) <= u[ok]), (k, float((np.abs(diff) - u)[ok].max()))
                fig["z"] = max(fig["z"], float((np.abs(diff) / u)[ok].max()))
            fig["held"] = int((z != 0).sum((1, 2)).max())                              # (at the last read)
        W = c.get_weights().astype(np.float64)
    fig.update(wmax=float(np.abs(te.W).max()), dW=float(np.abs(W - te.W).max()), dW1=float(np.abs(W - te.W).sum()), W1=float(np.abs(te.W).sum()),
               left_out=watch.fraction)
    fig["ceiling"] += K * 2.0 ** -24 * fig["W1"]
    return fig


CP = dict(domain=1, n_tilings=8, tiles_per_dim=8, policy=1, gamma=0.99, max_episode_steps=60)
MC = dict(domain=0, tiles_per_dim=8, algo=3, policy=1, epsilon=0.3, gamma=0.99, max_episode_steps=0)
NOT_EVICTING = [
    # name, N, K, alpha * T * N, kwargs
    ("cartpole_t8_sarsa_accumulate", 48, 200, 0.1, dict(CP, algo=3, epsilon=0.1, lam=0.9, trace=0)),
    # (CartPole pays only at the fall: on a finer grid or at a smaller step most Q(s, .) stay within 1e-5 of a tie for these 200 steps)
    ("cartpole_t8_q_saturate", 48, 200, 2.0, dict(CP, tiles_per_dim=5, algo=4, epsilon=0.2, lam=0.8, trace=1)),
    ("acrobot_t4_q_accumulate_softmax", 48, 120, 0.1, dict(domain=2, n_tilings=4, tiles_per_dim=6, algo=4, policy=2, tau=0.5, gamma=0.95, lam=0.7, trace=0,
                                                             max_episode_steps=50)),
    ("mountaincar_t4_sarsa_accumulate", 32, 600, 0.1, dict(MC, n_tilings=4, tiles_per_dim=10, lam=0.97, trace=0)),      # 128 slots per sub-list, none fills
    ("mountaincar_t16_sarsa_dutch", 32, 60, 0.1, dict(MC, n_tilings=16, lam=0.97, trace=2)),
]


@pytest.mark.parametrize("name,N,K,a,kw", NOT_EVICTING, ids=[c[0] for c in NOT_EVICTING])
def test_device_trace_is_the_unbounded_trace_while_nothing_is_evicted(ra, orc, name, N, K, a, kw):
    # the bars of test_gpu_sparse_lambda.py's teacher-forced test; the trace per entry within u(z) = 2 * 2^-23 / (1 - rate) * max(1, z_ref).  Q(lambda): a learner whose
    # Watkins cut the reference decides by less than 1e-5 (1 + |Q|) is left out of the trace comparison until its next reset (CutWatch), at most 5 % of the learner-steps
    f = run_leg(ra, orc, N, K, a, kw, evicting=False)
    print(f"sparse cap {name}: td {f['td']:.2e}  w {f['dW'] / f['wmax']:.2e} of max|W| {f['wmax']:.2e}  z {f['z']:.3f} of u(z)  held {f['held']}  left out {f['left_out']:.4f}")
    assert f["B"] == 0 and f["held"] < 512
    assert f["wmax"] > 1e-4
    assert f["td"] <= 2e-5, f["td"]
    assert f["dW"] <= 4e-6 * f["wmax"], (f["dW"], f["wmax"])
    assert f["left_out"] <= 0.05, f["left_out"]


EVICTING = [
    ("mountaincar_t8_dutch", 64, 900, dict(MC, n_tilings=8, lam=0.97, trace=2)),
    ("mountaincar_t16_saturate", 77, 500, dict(MC, n_tilings=16, lam=0.95, trace=1)),
    ("mountaincar_t16_accumulate", 32, 400, dict(MC, n_tilings=16, lam=0.95, trace=0)),
]


@pytest.mark.parametrize("name,N,K,kw", EVICTING, ids=[c[0] for c in EVICTING])
def test_capped_device_trace_is_within_the_bound_of_the_unbounded_one(ra, orc, name, N, K, kw):
    # the table: dz * d - dz' * d' = (d_dev - d_ref) z_ref - d_dev (z_ref - z_dev) per learner and step, so
    #   ||W_dev - W_ref||_1 <= sum_t alpha sum_i (|td_dev - td_ref| ||z_ref,i||_1 + |td_dev| (B_i + slack_i)) + K 2^-24 ||W||_1
    f = run_leg(ra, orc, N, K, 0.1, kw, evicting=True)
    print(f"sparse cap {name}: D/(B+slack) {f['DB']:.3f}  D/|z_ref| {f['Dz']:.2e}  B/|z_ref| {f['Bz']:.2e}  max|dW|/max|W| {f['dW'] / f['wmax']:.2e}  "
          f"|dW|_1 {f['dW1']:.3e} of its ceiling {f['ceiling']:.3e}  td {f['td']:.2e}  held {f['held']}")
    assert f["held"] == 512                                                            # the cap did take effect: some learner's list is full
    assert f["B"] > 0
    assert f["dW1"] <= f["ceiling"], (f["dW1"], f["ceiling"])
