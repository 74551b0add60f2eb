"""NAC over the Gibbs policy (RSRL_GIBBS_NAC = 37, examples/nac_softmax.rs) without a GPU: the constants in the header, the binding and the Rust
block; admission (every supported configuration reaches the device query, every other one is refused with the agent's name in the message, 36,
38 and 1000 are no algos); the restatement the GPU tests compare against (tests/gnac_numpy.py) on identities that pin psi and the actor's
reshape; and the GPU rule test's bars on the GPU test's exact cases -- a float32 emulation of the rule in the device's operation order stays
inside them for every learner, each of the two deliberately wrong rules leaves them for at least half of the learners -- and the driver-loop
test's seed."""
import importlib.util
import os
import re

import numpy as np
import pytest

import rsrl_amd
from tests import gnac_numpy as gq
from tests.agent_contract import compile_example, create_rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
GNAC = 37
BASE = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=GNAC, policy=rsrl_amd.SOFTMAX, n_envs=4, n_steps=100)
REG = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- the interface
def test_header_binding_constants_and_rust_block_agree():
    gen = _load("gen_rust_sys")
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_GIBBS_NAC\s*=\s*37\b", h) and "(36 is no algo, and neither is 38.)" in h
    assert rsrl_amd.GIBBS_NAC == 37 and rsrl_amd.context.GIBBS_NAC == 37 and rsrl_amd.NAC == 28
    assert re.search(r"#define\s+RSRL_HIP_ABI_VERSION\s+9\b", h)
    block = gen.doc_block()
    assert "pub const RSRL_GIBBS_NAC: i32 = 37;" in block and block == gen.generate()
    assert len(gen.parse_header()[0]) == len(dict(gen.declared_functions(block))) == 96      # no new entry point
    # the header cites the reference's lines and the defect, and no longer lists the example as not built
    assert "fa/linear.rs:91-102" in h and "CompatibleBasis::project (:42-46)" in h and "index_axis_move" in h and "Not built: nac_softmax.rs" not in h


def test_thirty_six_thirty_eight_and_a_thousand_are_no_algos():
    for algo in (36, 38, 1000):
        for kw in (dict(), dict(policy=rsrl_amd.GREEDY), dict(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, policy=rsrl_amd.BETA)):
            rc, msg = create_rc(BASE, algo=algo, **kw)
            assert rc == EINVAL and "unknown algo %d" % algo in msg, (algo, kw, rc, msg)


def test_supported_configurations_reach_the_device_query():
    for domain, order in REG:
        for extra in (dict(), dict(steps_per_launch=1), dict(max_episode_steps=1000, lr=0.01, alpha=0.01, gamma=0.999, tau=1.0), dict(n_steps=1),
                      dict(n_steps=65536), dict(max_episode_steps=0, tau=0.5)):
            rc, msg = create_rc(BASE, domain=domain, order=order, **extra)
            assert rc == 0 or (rc == EHIP and "device" in msg), (domain, order, extra, rc, msg)


def test_other_configurations_are_refused_with_the_agents_name():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(domain=rsrl_amd.CART_POLE, order=2), dict(domain=rsrl_amd.CART_POLE, order=7),
           dict(domain=rsrl_amd.ACROBOT, order=3), dict(weight_mode=rsrl_amd.W_SHARED), dict(weight_dtype=rsrl_amd.W_BF16),
           dict(domain=rsrl_amd.CART_POLE, order=7, weight_dtype=rsrl_amd.W_BF16), dict(agent_policy=rsrl_amd.SOFTMAX), dict(agent_policy=rsrl_amd.GREEDY),
           dict(epsilon_decay=0.99), dict(domain=rsrl_amd.HIV_TREATMENT, order=1), dict(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR),
           dict(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, policy=rsrl_amd.BETA), dict(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, policy=6),
           dict(policy=rsrl_amd.GREEDY), dict(policy=rsrl_amd.EPSILON_GREEDY), dict(policy=rsrl_amd.RANDOM), dict(policy=rsrl_amd.BETA), dict(policy=6)]
    for b in bad:
        rc, msg = create_rc(BASE, **b)
        assert rc == EINVAL and "RSRL_GIBBS_NAC" in msg, (b, rc, msg)
    for n in (0, -1, 65537):
        rc, msg = create_rc(BASE, n_steps=n)
        assert rc == EINVAL and "RSRL_GIBBS_NAC" in msg and "n_steps" in msg and "65536" in msg, (n, rc, msg)
    # RSRL_NAC itself keeps refusing Softmax and the discrete domains, exactly as before
    for b in (dict(algo=rsrl_amd.NAC), dict(algo=rsrl_amd.NAC, domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR), dict(algo=rsrl_amd.NAC, policy=rsrl_amd.BETA)):
        rc, msg = create_rc(BASE, **b)
        assert rc == EINVAL and "RSRL_NAC" in msg and "RSRL_GIBBS_NAC" not in msg, (b, rc, msg)


def test_example_compiles(tmp_path):
    compile_example(tmp_path, "nac_softmax")


# ---- the restatement
def _random_learner(rng, F, A):
    return rng.normal(size=(A + 1) * F), rng.normal(size=(F, A)), rng.uniform(-1.0, 1.0, size=F)


@pytest.mark.parametrize("F,A", [(4, 3), (9, 3), (16, 2), (36, 3)])
def test_compatible_features_average_to_zero_under_the_policy(F, A):
    """sum_b p_b Q(s, b) == <w_v, phi>: sum_b p_b (1[c==b] - p_c) = 0 for every c.  It pins psi: the score blocks, their signs, and the basis block"""
    rng = np.random.default_rng(F * 10 + A)
    for tau in (1.0, 0.5):
        w, Th, phi = _random_learner(rng, F, A)
        p = gq.probs(Th, phi, tau)
        assert abs(p.sum() - 1.0) < 1e-15
        v = sum(p[b] * gq.q_value(w, Th, phi, b, tau) for b in range(A))
        wv = w[F * A:] @ phi
        scale = np.abs(w).sum()
        assert abs(v - wv) <= 1e-14 * scale, (F, A, v, wv)
        # the reference's column-0-only psi does not have the property against (A+1) F weights
        v0 = sum(p[b] * gq.q_value(w, Th, phi, b, tau, gq.psi_column0) for b in range(A))
        assert abs(v0 - wv) > 1e-6 * scale
        # psi's layout: index f * A + b, then the basis
        ps = gq.psi(Th, phi, 1, tau)
        c = -p.copy()
        c[1] += 1.0
        assert ps.shape == ((A + 1) * F,) and np.array_equal(ps[F * A:], phi)
        for f in (0, F - 1):
            for b in range(A):
                assert ps[f * A + b] == c[b] * phi[f]


def test_score_coefficients_at_zero_theta():
    F, A = 4, 3
    phi = np.array([1.0, -0.5, 0.25, 1.0])
    c = gq.score_coefs(np.zeros((F, A)), phi, 0, 1.0)
    assert np.allclose(c, [2.0 / 3.0, -1.0 / 3.0, -1.0 / 3.0], rtol=1e-15, atol=0)
    assert np.allclose(gq.score_coefs(np.zeros((F, A)), phi, 2, 0.5), [-1.0 / 3.0, -1.0 / 3.0, 2.0 / 3.0], rtol=1e-15, atol=0)      # no 1 / tau
    w = np.arange(1.0, 17.0)
    q = gq.q_value(w, np.zeros((F, A)), phi, 0, 1.0)
    d = [w[:12].reshape(F, A)[:, b] @ phi for b in range(A)]
    assert abs(q - (2.0 / 3.0 * d[0] - d[1] / 3.0 - d[2] / 3.0 + w[12:] @ phi)) < 1e-13


@pytest.mark.parametrize("F,A", [(4, 3), (16, 2), (36, 3)])
def test_actor_step_is_the_row_major_reshape(F, A):
    rng = np.random.default_rng(F + A)
    w, Th, _ = _random_learner(rng, F, A)
    alpha = 0.01
    T2, norm = gq.nac_handle(w, Th, alpha)
    assert abs(norm - np.linalg.norm(w[:F * A])) <= 1e-14 * norm
    assert np.allclose(T2 - Th, alpha / norm * w[:F * A].reshape(F, A), rtol=0, atol=1e-15)
    assert T2[2, 1] - Th[2, 1] == pytest.approx(alpha / norm * w[2 * A + 1], rel=1e-12)
    # an all-zero gradient: the floor, and theta stays
    T0, n0 = gq.nac_handle(np.concatenate([np.zeros(F * A), w[F * A:]]), Th, alpha)
    assert n0 == 1e-3 and np.array_equal(T0, Th)
    # the float32 restatement follows it, and the column-major reshape is another rule
    T32, n32 = gq.nac_handle_f32(w, Th, alpha)
    w32, Th32 = w.astype(np.float32).astype(np.float64), Th.astype(np.float32).astype(np.float64)
    T64, n64 = gq.nac_handle(w32, Th32, float(np.float32(alpha)))
    assert T32.dtype == np.float32 and abs(float(n32) - n64) <= (F * A + 2) * gq.U * n64 and np.max(np.abs(T32 - T64)) <= 1e-6
    Tc, _ = gq.nac_handle_colmajor(w, Th, alpha)
    assert np.max(np.abs(Tc - T2)) > 1e-4


def test_sarsa_handle_by_hand():
    F, A = 4, 3
    rng = np.random.default_rng(2)
    w, Th, phi = _random_learner(rng, F, A)
    phi_n, a, na, r, gamma, lr, tau = rng.uniform(-1, 1, size=F), 2, 0, -1.0, 0.9, 0.01, 0.5
    q, qn = gq.q_value(w, Th, phi, a, tau), gq.q_value(w, Th, phi_n, na, tau)
    d, w2 = gq.sarsa_handle(w, Th, phi, a, r, phi_n, na, True, gamma, lr, tau)
    assert d == r - q and np.allclose(w2, w + lr * d * gq.psi(Th, phi, a, tau), rtol=1e-15, atol=0)
    d, w2 = gq.sarsa_handle(w, Th, phi, a, r, phi_n, na, False, gamma, lr, tau)
    assert abs(d - (r + gamma * qn - q)) <= 1e-15 * abs(d) and np.allclose(w2[F * A:] - w[F * A:], lr * d * phi, rtol=1e-12, atol=0)
    assert gq.sarsa_handle(w, Th, phi, a, r, 7.0 * phi_n, 1, True, gamma, lr, tau)[0] == r - q      # the terminal rule reads neither s' nor the draw


# ---- the GPU rule test's bars on its exact cases
@pytest.mark.parametrize("domain,order", gq.CASES)
def test_the_bars_are_neither_vacuous_nor_blind(orc, domain, order):
    case = gq.handle_case(orc, domain, order)
    N, F, A = len(case["a"]), case["F"], case["A"]
    assert N == 67 and case["w"].shape == (N, (A + 1) * F) and case["theta"].shape == (N, F, A)
    assert 0 < case["term"].sum() < N and N // 8 <= case["term"].sum() <= N // 2
    phi_s, phi_n = (gq.project(orc, domain, order, S).astype(np.float32) for S in (case["frm"], case["nxt"]))
    assert np.abs(phi_s).max() <= 1.0 and np.all(phi_s[-1] == 1.0)
    delta, w2, e_d, e_w, out = gq.rule_reference(orc, case, gq.RULE_SEED, phi_s, phi_n)
    assert (~out).sum() >= 3 * N // 4
    # the bars are small against what they hold: the median |delta| is a thousand times the widest bar (CartPole's rewards are 0 until the pole
    # falls: its errors are the smallest), the widest w bar a hundredth of the median learner's largest move
    moved = np.abs(w2 - case["w"].astype(np.float64)).max(axis=1)
    assert np.median(np.abs(delta)) > 1e3 * e_d.max() and e_d.max() < 1e-4 and np.median(moved) > 100 * e_w.max()
    print("(%d, %d): delta bar max %.3g, w bar max %.3g" % (domain, order, e_d.max(), e_w.max()))
    # the premise of the probability's bound holds on these cases: the emulated f32 probabilities are within EP of the f64 ones
    p, tau = gq.RULE, gq.RULE["tau"]
    worst_d = worst_w = worst_p = 0.0
    for i in range(N):
        x = orc.draw(gq.RULE_SEED, i, 0, orc.BLK_INNER)
        d32, w32, na32, pn32 = gq.rule_f32(orc, case["w"][i], case["theta"][i], phi_s[:, i], int(case["a"][i]), case["rew"][i], phi_n[:, i],
                                           bool(case["term"][i]), x, p["gamma"], p["lr"], tau)
        worst_p = max(worst_p, np.max(np.abs(pn32 - gq.probs(case["theta"][i], phi_n[:, i], tau))))
        if out[i]:
            continue
        assert d32.dtype == np.float32 and w32.dtype == np.float32
        worst_d = max(worst_d, abs(float(d32) - delta[i]) / e_d[i])
        worst_w = max(worst_w, np.max(np.abs(w32 - w2[i]) / e_w[i]))
        assert abs(float(d32) - delta[i]) <= e_d[i] and np.all(np.abs(w32 - w2[i]) <= e_w[i]), i
    print("float32 emulation: delta at %.3g of its bar, w at %.3g, p within %.3g" % (worst_d, worst_w, worst_p))
    assert worst_p <= gq.EP
    # the reference's column-0-only psi leaves the bars for at least half of the learners
    d0, w0, _, _, _ = gq.rule_reference(orc, case, gq.RULE_SEED, phi_s, phi_n, psi_fn=gq.psi_column0)
    keep = ~out
    assert (np.abs(d0 - delta) > e_d)[keep].sum() >= keep.sum() / 2 and (np.abs(w0 - w2) > e_w).any(axis=1)[keep].sum() >= keep.sum() / 2
    # the column-major reshape leaves nac_update's bit-for-bit comparison for at least half of the learners
    differs = 0
    for i in range(N):
        right, _ = gq.nac_handle_f32(case["w"][i], case["theta"][i], 0.01)
        wrong, _ = gq.nac_handle_colmajor(case["w"][i], case["theta"][i], float(np.float32(0.01)))
        differs += wrong.astype(np.float32).tobytes() != right.tobytes()
    assert differs >= N / 2


def test_the_driver_loop_seed(orc):
    """the restated loop alone flags at most a quarter of the learners near a cumulative boundary at LOOP_SEED; terminals and caps both occur"""
    L = gq.LOOP
    rng = np.random.default_rng(8)
    S0, A0 = gq.loop_start(orc, rsrl_amd.MOUNTAIN_CAR, L["N"], rng)
    acts, ws, ths, near = gq.gnac_restated_loop(orc, rsrl_amd.MOUNTAIN_CAR, 3, L["N"], L["K"], L["cap"], L["P"], gq.LOOP_SEED, L["gamma"], L["lr"], L["alpha"],
                                                L["tau"], S0, A0)
    assert L["N"] == 67 and L["K"] <= 60 and L["P"] == 3 and L["cap"] == 20
    assert near.sum() <= L["N"] // 4, near.sum()
    assert acts.shape == (L["K"], L["N"]) and set(np.unique(acts)) == {0, 1, 2}
    assert all(np.isfinite(w).all() and np.abs(w).max() > 0 for w in ws) and all(np.abs(t).max() > 0 for t in ths)
