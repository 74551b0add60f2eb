"""NAC over the Gibbs policy with the SCB SARSA critic (RSRL_GIBBS_NAC, train_gibbs_nac.hip) on the device, against tests/gnac_numpy.py: handle
against the f64 rule within the derived bars (tests/test_gibbs_nac_cpu.py shows they are neither vacuous nor blind), the actor's update bit for
bit against the float32 restatement, q_evaluate and the policy side, the driver loop against the restated loop, and the agent contract through
tests/agent_contract.py (train against the host trait loop / launch depths / shards, the checkpoint, foreign files, the checksum, the ESTATE
list, the C++ example).  N = 67: one wavefront and a tail.  Every test prints its figures before it asserts."""
import functools
import os

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import RsrlHipError, _abi
from tests import gnac_numpy as gq
from tests.ac_numpy import near_boundary
from tests.agent_contract import check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, rand_states, run_example

pytestmark = pytest.mark.gpu

MC, GNAC, SOFTMAX = rsrl_amd.MOUNTAIN_CAR, 37, rsrl_amd.SOFTMAX
N = 67
ESTATE, EINVAL = -5, -1
BASE = dict(domain=MC, order=3, algo=GNAC, policy=SOFTMAX, n_envs=N, seed=5, gamma=0.95, lr=0.01, alpha=0.01, tau=1.0, n_steps=100)


class Ctx(rsrl_amd.Context):
    """tests/agent_contract.snapshot compares an agent's `weights`; it does not know this agent's theta.  Here get_weights shows both of a
    learner's matrices, w's (A+1) F values then theta's F A -- so the harness holds the actor to the same bits as the critic"""

    def get_weights(self, env_index=0):
        return np.concatenate([super().get_weights(env_index).ravel(), self.get_policy_weights(env_index).ravel()])


def ctx(**kw):
    return Ctx(**dict(BASE, **kw))


def plain(**kw):
    return rsrl_amd.Context(**dict(BASE, **kw))


def _install(c, case):
    for i in range(c.N):
        c.set_weights(case["w"][i].reshape(-1, 1), i)
        c.set_policy_weights(case["theta"][i], i)


# ---- 1. handle against the f64 rule within the derived bars
@functools.lru_cache(maxsize=None)
def _handled(orc, domain, order):
    """one pass per case, shared and left unchanged: the device's td errors, weights and features, and the f64 rule on those features"""
    case = gq.handle_case(orc, domain, order)
    p = gq.RULE
    with plain(domain=domain, order=order, seed=gq.RULE_SEED, gamma=p["gamma"], lr=p["lr"], tau=p["tau"]) as c:
        assert c.n_weight_rows == (case["A"] + 1) * case["F"] and c.n_out == 1 and c.n_policy_out == case["A"] == c.A and c.F == case["F"]
        assert not c.get_weights(0).any() and not c.get_policy_weights(0).any()                      # both zero at create
        _install(c, case)
        phi_s, phi_n = c.project(case["frm"]), c.project(case["nxt"])
        before = c.checksum()
        td = c.handle(case["frm"], case["a"], case["rew"], case["nxt"], case["term"])
        got = dict(td=td, w=np.stack([c.get_weights(i).ravel() for i in range(N)]), theta=np.stack([c.get_policy_weights(i) for i in range(N)]),
                   steps=c.step_count, moved=c.checksum() != before)
    ref = gq.rule_reference(orc, case, gq.RULE_SEED, phi_s, phi_n)
    oracle_phi = gq.project(orc, domain, order, case["frm"]).astype(np.float32)
    print("(%d, %d): the device's features against the oracle's device-order ones: max |d| %.3g" % (domain, order, np.abs(phi_s - oracle_phi).max()))
    return case, got, ref


@pytest.mark.parametrize("domain,order", gq.CASES)
def test_handle_against_the_f64_rule_within_the_derived_bars(orc, domain, order):
    case, got, (delta, w2, e_d, e_w, out) = _handled(orc, domain, order)
    keep = ~out
    assert got["steps"] == 1 and got["moved"] and keep.sum() >= 3 * N // 4 and N // 8 <= case["term"].sum() <= N // 2
    assert got["theta"].tobytes() == case["theta"].tobytes()                                         # critic.handle does not move the actor
    rel_d = np.abs(got["td"].astype(np.float64) - delta) / e_d
    rel_w = (np.abs(got["w"].astype(np.float64) - w2) / e_w).max(axis=1)
    print("(%d, %d): delta at %.3g of its bar (max %.3g), w at %.3g of its bar (max %.3g), %d learners" %
          (domain, order, rel_d[keep].max(), e_d.max(), rel_w[keep].max(), e_w.max(), keep.sum()))
    assert np.all(rel_d[keep] <= 1.0), np.flatnonzero(keep & (rel_d > 1.0))
    assert np.all(rel_w[keep] <= 1.0), np.flatnonzero(keep & (rel_w > 1.0))
    assert np.abs(w2 - case["w"]).max() > 1e-3                                                       # w moved far more than the bars


# ---- 2. nac_update against nac_handle_f32, bit for bit
@pytest.mark.parametrize("domain,order", gq.CASES)
def test_actor_update_is_the_float32_restatement_bit_for_bit(domain, order):
    rng = np.random.default_rng(90 + domain * 10 + order)
    with plain(domain=domain, order=order) as c:
        F, A = c.F, c.A
        FA = F * A
        w = (rng.normal(size=(N, (A + 1) * F, 1)) * rng.uniform(0.01, 3.0, size=(N, 1, 1))).astype(np.float32)
        w[0] = 0.0                                                                       # an all-zero w: norm = 1e-3, theta unmoved
        unit = w[1, :FA, 0].astype(np.float64) / np.linalg.norm(w[1, :FA, 0].astype(np.float64))
        w[1, :FA, 0] = (unit * 0.9999e-3).astype(np.float32)                             # ||g|| just below the floor
        w[2, :FA, 0] = (unit * 1.0001e-3).astype(np.float32)                             # ... and just above
        w[3, :FA, 0] = (unit * 1e3).astype(np.float32)                                   # ||g|| near 1e3
        w[4, :FA, 0] = 0.0                                                               # g = 0 next to a live basis block
        th = rng.normal(size=(N, F, A)).astype(np.float32)
        for i in range(N):
            c.set_weights(w[i], i)
            c.set_policy_weights(th[i], i)
        mask = (np.arange(N) % 3 != 2).astype(np.uint8)
        mask[:5] = 1
        norm = c.nac_update(mask)
        for i in range(N):
            got = c.get_policy_weights(i)
            if mask[i]:
                want, wn = gq.nac_handle_f32(w[i], th[i], BASE["alpha"])
                assert got.tobytes() == want.tobytes(), (i, np.abs(got - want).max())
                assert norm[i].tobytes() == wn.tobytes(), (i, norm[i], wn)
            else:
                assert got.tobytes() == th[i].tobytes() and norm[i] == 0.0, i             # a masked-out learner keeps its bytes and reports 0
            assert c.get_weights(i).tobytes() == w[i].tobytes(), i                       # the critic is not reset
        assert norm[0] == np.float32(1e-3) and norm[4] == np.float32(1e-3) and norm[1] == np.float32(1e-3) and norm[2] > np.float32(1e-3)
        assert np.array_equal(c.get_policy_weights(0), th[0]) and np.array_equal(c.get_policy_weights(4), th[4])
        assert abs(norm[3] - 1e3) < 1.0 and c.step_count == 0
        after = np.stack([c.get_policy_weights(i) for i in range(N)])
        norm2 = c.nac_update()                                                           # mask = NULL: every learner
        for i in range(N):
            want, wn = gq.nac_handle_f32(w[i], after[i], BASE["alpha"])
            assert c.get_policy_weights(i).tobytes() == want.tobytes() and norm2[i].tobytes() == wn.tobytes(), i
        assert np.all(norm2 > 0) and not np.array_equal(c.get_policy_weights(5), th[5])


# ---- 3. q_evaluate against the restatement; the policy side reads theta, the value side does not read theta's bytes as weights
@pytest.mark.parametrize("domain,order", gq.CASES)
def test_q_evaluate_and_the_policy_side(orc, domain, order):
    case, _, _ = _handled(orc, domain, order)
    A, F, tau = case["A"], case["F"], gq.RULE["tau"]
    S = case["frm"]
    with plain(domain=domain, order=order, tau=tau, seed=23) as c:
        _install(c, case)
        phi = c.project(S)
        before = c.checksum()
        q = c.q_evaluate(S)
        assert q.shape == (A, N) and q.dtype == np.float32
        assert np.array_equal(c.q_evaluate(S), q) and c.checksum() == before and c.step_count == 0      # read-only
        worst = 0.0
        for i in range(N):
            Th, w, ph = case["theta"][i].astype(np.float64), case["w"][i].astype(np.float64), phi[:, i].astype(np.float64)
            for b in range(A):
                want, bar, _, _ = gq._q_bar(gq.blocks(w, F, A), Th, ph, b, tau)
                assert abs(want - gq.q_value(w, Th, ph, b, tau)) <= 1e-14 * np.abs(w).sum()
                worst = max(worst, abs(float(q[b, i]) - want) / bar)
                assert abs(float(q[b, i]) - want) <= bar, (i, b, q[b, i], want, bar)
        print("(%d, %d): q_evaluate at %.3g of its bar" % (domain, order, worst))
        # the policy side reads theta: probabilities within 1e-6 of the oracle's, modes equal
        h = np.array([case["theta"][i].astype(np.float64).T @ orc.fourier_project(domain, order, S[:, i]) for i in range(N)]).T
        want_p = np.array([orc.policy_probs(orc.SOFTMAX, h[:, i], tau=tau) for i in range(N)]).T
        probs = c.policy_probs(S)
        print("(%d, %d): probabilities within %.3g" % (domain, order, np.max(np.abs(probs - want_p))))
        assert np.max(np.abs(probs - want_p)) <= 1e-6
        assert np.array_equal(c.policy_mode(S), [orc.argmax_first(probs[:, i], prec="f32") for i in range(N)])
        pa = c.policy_prob(S, case["a"])
        assert np.max(np.abs(pa - h[case["a"], np.arange(N)])) <= 1e-5                     # (Softmax's Function<(S, A)> is the raw preference, softmax.rs:84-92: theta's)
        sample = c.policy_sample(S)                                                      # the first API call: BLK_API, call 0
        for i in range(N):
            x = orc.draw(23, i, 0, orc.BLK_API)
            if not near_boundary(want_p[:, i], x):
                assert sample[i] == orc.policy_sample(orc.SOFTMAX, h[:, i], x, tau=tau), i
        # reset's initial sample on BLK_INIT reads theta, and leaves both matrices alone
        c.reset()
        s0 = orc.domain_reset(domain, prec="f32")
        phi0 = orc.fourier_project(domain, order, s0)
        acts = c.actions
        for i in range(N):
            h0 = case["theta"][i].astype(np.float64).T @ phi0
            x = orc.draw(23, i, 0, orc.BLK_INIT)
            if not near_boundary(orc.policy_probs(orc.SOFTMAX, h0, tau=tau), x):
                assert acts[i] == orc.policy_sample(orc.SOFTMAX, h0, x, tau=tau), i
        assert c.checksum()[0] == before[0]
        # the value side does not read theta's bytes as weights: another theta of the same probabilities (a constant added to every preference
        # through the bias feature, the last one) leaves Q within its bar, and zero w gives Q = 0 whatever theta holds
        for i in range(N):
            t2 = case["theta"][i].copy()
            t2[-1, :] += np.float32(0.5)
            c.set_policy_weights(t2, i)
        q2 = c.q_evaluate(S)
        assert np.max(np.abs(q2 - q)) <= 1e-5
        for i in range(N):
            c.set_weights(np.zeros(((A + 1) * F, 1), dtype=np.float32), i)
        assert not c.q_evaluate(S).any()
        # and theta = 0, w's basis block alone: Q(s, b) = <w_v, phi> for every b
        wv = np.zeros(((A + 1) * F, 1), dtype=np.float32)
        wv[F * A:, 0] = np.linspace(-1.0, 1.0, F, dtype=np.float32)
        c.set_weights(wv, 3)
        q3 = c.q_evaluate(S)
        want = phi[:, 3].astype(np.float64) @ wv[F * A:, 0].astype(np.float64)
        assert np.all(np.abs(q3[:, 3] - want) <= 1e-5) and q3[0, 3] != 0 and not q3[:, :3].any()


# ---- 4. the driver loop against the restated loop
def test_driver_loop_against_the_restated_loop(orc):
    L = gq.LOOP
    n, K, cap, P, domain, order = L["N"], L["K"], L["cap"], L["P"], MC, 3
    rng = np.random.default_rng(8)
    S0, A0 = gq.loop_start(orc, domain, n, rng)
    with plain(n_envs=n, order=order, seed=gq.LOOP_SEED, gamma=L["gamma"], lr=L["lr"], alpha=L["alpha"], tau=L["tau"], max_episode_steps=cap, n_steps=P) as c:
        c.states, c.actions = S0, A0
        dev_acts, episodes, truncated = [], 0, 0
        for _ in range(K):                                            # one batch-step per call: the same bits as train(K), every action seen
            st = c.train(1)
            episodes += st["episodes"]; truncated += st["episodes_truncated"]
            dev_acts.append(c.actions)
        acts, ws, ths, near = gq.gnac_restated_loop(orc, domain, order, n, K, cap, P, gq.LOOP_SEED, L["gamma"], L["lr"], L["alpha"], L["tau"], S0, A0)
        same = (np.array(dev_acts) == acts).all(axis=0)               # an fp32 rounding may flip a softmax draw: that learner leaves the comparison
        print("agree on every action: %.3f of the learners; near: %d; episodes %d, truncated %d" % (same.mean(), near.sum(), episodes, truncated))
        assert same.mean() >= 0.9, same
        assert near.sum() <= n // 4
        worst = 0.0
        for i in np.flatnonzero(same & ~near):
            for got, want in ((c.get_weights(i).ravel(), ws[i]), (c.get_policy_weights(i), ths[i])):
                bar = 3e-6 * (1 + np.max(np.abs(want))) * K * 16
                worst = max(worst, np.max(np.abs(got - want)) / bar)
                assert np.max(np.abs(got - want)) <= bar, i
        print("w and theta at %.3g of the loop bar" % worst)
        assert episodes > truncated > 0                               # terminals and caps both happened
        assert np.abs(c.get_policy_weights(0)).max() > 0              # the actor moved


# ---- 5. the contract
P, CAP, K = 3, 7, 48


def _start_near_the_goal(c, off):
    """reset, then every fourth learner (by global id) beside the goal on MountainCar: terminal ends occur as well as cut ones"""
    c.reset()
    if c.cfg.domain == MC:
        s = c.states
        s[:, (np.arange(c.N) + off) % 4 == 0] = np.array([[0.49], [0.06]], dtype=np.float32)
        c.states = s


def _gnac_trait(c, k_steps, cap):
    """the loop of nac_softmax.rs through the trait calls: domain_step -> handle -> domain_reset(ended) -> policy_sample(NULL) -> nac_update for
    the learners whose step was a multiple of P in its episode, counted from 0"""
    ep = c.episode_steps.astype(np.int64)
    for _ in range(k_steps):
        update = (ep % P == 0).astype(np.uint8)
        a = c.actions
        frm, nxt, rew, term = c.domain_step(a)
        c.handle(frm, a, rew, nxt, term)
        ep += 1
        mask = (term.astype(bool) | ((ep >= cap) if cap > 0 else False)).astype(np.uint8)
        c.domain_reset(mask)
        ep[mask == 1] = 0
        c.policy_sample()
        c.nac_update(update)
    c.episode_steps = ep.astype(np.uint32)


@pytest.mark.parametrize("domain,order", gq.CASES)
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(domain, order):
    """(66 learners: the harness joins two shards of N / 2.)"""
    n = 66
    kw = dict(domain=domain, order=order, n_envs=n, max_episode_steps=CAP, n_steps=P, lr=0.02, alpha=0.05, gamma=0.97, tau=0.7)
    st, ref = check_train_invariance(ctx, kw, K, CAP, depths=(1, 3, 0), first_split=13, kernel="k_train_gibbs_nac", setup=_start_near_the_goal,
                                     trait=_gnac_trait)
    A = 2 if domain == rsrl_amd.CART_POLE else 3
    F = (order + 1) ** (2 if domain == MC else 4)
    assert st["env_steps"] == n * K and st["episodes"] >= st["episodes_truncated"] > 0
    if domain == MC:
        assert st["episodes"] > st["episodes_truncated"] and st["sum_abs_td_error"] > 0      # terminals and truncations both occur
    both = ref["weights"]
    assert both.shape == (n, (A + 1) * F + F * A) and np.isfinite(both).all()
    if domain != rsrl_amd.CART_POLE:                                  # (CartPole's reward is 0 until the pole falls: from zero weights nothing moves before)
        assert np.abs(both[:, :(A + 1) * F]).max() > 0 and np.abs(both[:, (A + 1) * F:]).max() > 0
    assert ref["actions"].dtype == np.int32 and ref["actions"].min() >= 0 and ref["actions"].max() < A


def test_checkpoint_resumes_bitwise_and_foreign_files_are_refused(tmp_path):
    kw = dict(n_envs=32, order=3, max_episode_steps=17, n_steps=P, lr=0.02, alpha=0.05)
    path = os.path.join(str(tmp_path), "gnac.ckpt")
    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"))
    with open(path, "rb") as f:
        head = f.read(72)
    F, A = 16, 3
    assert int.from_bytes(head[8:12], "little") == 10 and int.from_bytes(head[12:16], "little") == MC
    assert int.from_bytes(head[44:48], "little") == GNAC and int.from_bytes(head[52:56], "little") == 18
    assert os.path.getsize(path) == 72 + 32 * 4 * (A + 1) * F + 32 * 4 * F * A
    mc = dict(domain=MC, order=3, n_envs=32, policy=SOFTMAX)
    cmc = dict(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, order=3, n_envs=32)
    others = [dict(mc, algo=rsrl_amd.ACTOR_CRITIC), dict(mc, algo=rsrl_amd.TD_ACTOR_CRITIC), dict(cmc, algo=rsrl_amd.NAC, policy=rsrl_amd.BETA, n_steps=P),
              dict(cmc, algo=rsrl_amd.NAC, policy=6, n_steps=P), dict(mc, algo=rsrl_amd.QLEARNING, policy=rsrl_amd.GREEDY)]
    check_foreign_checkpoints_refused(ctx, kw, path, others, tmp_path)


def test_checksum_covers_both_matrices():
    with plain(n_envs=8, max_episode_steps=9, n_steps=P) as c:
        c.reset()
        c.train(5)
        before = c.checksum()
        th = c.get_policy_weights(3)
        th[2, 1] += 0.25
        c.set_policy_weights(th, 3)
        mid = c.checksum()
        assert mid[0] != before[0] and mid[1] == before[1]
        w = c.get_weights(3)
        w[-1, 0] += 0.25                                              # the basis block's last row: beyond F rows, inside (A+1) F
        c.set_weights(w, 3)
        assert c.checksum()[0] != mid[0] and c.checksum()[1] == mid[1]


def test_refusals():
    L = _abi.lib()
    S = np.zeros((2, N), dtype=np.float32)
    S[0] = -0.5
    ai, af = np.zeros(N, dtype=np.int32), np.full(N, 0.5, dtype=np.float32)
    r, t, out_i, out_f = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.float32)
    p = lambda x: x.ctypes.data_as(_abi.C.c_void_p)      # noqa: E731

    def refused(call, code=ESTATE):
        try:
            rc = call()
        except RsrlHipError as e:
            rc = e.code
        assert rc == code and L.rsrl_hip_last_error(), (rc, L.rsrl_hip_last_error())

    with plain(max_episode_steps=20) as c:
        h, F, A = c._h, c.F, c.A
        c.reset()
        before, acts = c.checksum(), c.actions
        for call in (lambda: c.q_find_max(S), lambda: c.q_find_min(S),
                     lambda: L.rsrl_hip_q_expected_value(h, p(S), N, p(np.full((3, N), 1.0 / 3.0, dtype=np.float32)), p(out_f)),
                     # every *_f32 call
                     lambda: L.rsrl_hip_get_actions_f32(h, p(out_f)), lambda: L.rsrl_hip_set_actions_f32(h, p(af)),
                     lambda: L.rsrl_hip_domain_step_f32(h, p(af), None, None, None, None),
                     lambda: L.rsrl_hip_handle_f32(h, p(S), p(af), p(r), p(S), p(t), N, p(out_f)),
                     lambda: L.rsrl_hip_policy_sample_f32(h, p(S), N, p(out_f)), lambda: L.rsrl_hip_policy_mode_f32(h, p(S), N, p(out_f)),
                     lambda: L.rsrl_hip_q_evaluate_f32(h, p(S), p(af), N, p(out_f)),
                     lambda: c.handle_batch(np.zeros((1, 2, N)), np.zeros((1, N)), np.zeros((1, N)), np.zeros(N)),
                     lambda: c.handle_transitions(np.zeros((1, 2, N)), np.zeros((1, N)), np.zeros((1, 2, N)), np.zeros((1, N)), np.zeros(N)),
                     lambda: c.get_traces(0), lambda: c.set_traces(np.zeros((F, 1)), 0),
                     lambda: L.rsrl_hip_get_td_weights(h, 0, p(out_f)), lambda: c.get_behaviour_weights(0), lambda: c.get_lstd_state(0),
                     lambda: c.get_lstd_batch_state(0), lambda: c.episode_record):
            refused(call)
        refused(lambda: L.rsrl_hip_set_q_carry(h, p(np.zeros((A, N), dtype=np.float32))), EINVAL)      # the q carry
        assert c.checksum() == before and c.step_count == 0 and c.actions.tobytes() == acts.tobytes()
        assert c.n_weight_rows == (A + 1) * F and c.get_weights(0).shape == ((A + 1) * F, 1) and c.get_policy_weights(0).shape == (F, A)
    # rsrl_hip_nac_update keeps its ESTATE message for the other algos
    with rsrl_amd.Context(domain=MC, order=3, algo=rsrl_amd.ACTOR_CRITIC, policy=SOFTMAX, n_envs=4) as c:
        with pytest.raises(RsrlHipError) as e:
            c.nac_update()
        assert e.value.code == ESTATE and "only NAC (RSRL_NAC) has a critic over the stable compatible basis and an actor update of its own" in str(e.value)
    # refused at create, with the agent's name
    for kw in (dict(policy=rsrl_amd.GREEDY), dict(order=6), dict(weight_mode=rsrl_amd.W_SHARED), dict(n_steps=0), dict(domain=rsrl_amd.HIV_TREATMENT, order=1)):
        with pytest.raises(RsrlHipError) as e:
            plain(**kw)
        assert e.value.code == EINVAL and "RSRL_GIBBS_NAC" in str(e.value), kw
    for algo in (36, 38):
        with pytest.raises(RsrlHipError) as e:
            plain(algo=algo)
        assert e.value.code == EINVAL and "unknown algo" in str(e.value), algo


def test_example_builds_and_runs(tmp_path):
    out = run_example(tmp_path, "nac_softmax", [64, 2, 300])
    lines = out.strip().splitlines()
    assert len(lines) == 4 and lines[0].startswith("Batch 1:") and lines[1].startswith("Batch 2:") and lines[3].startswith("OOS:")
    tmax = float(out.split("max |theta| of learner 0:")[1].split()[0])
    assert np.isfinite(tmax) and tmax > 0.0 and "nan" not in out.lower()
