"""NAC with the Beta policy and the SCB SARSA critic (RSRL_NAC, train_nac.hip) on the device, against tests/nac_numpy.py: the actor's update bit
for bit against the float32 restatement, the critic's rule and Q(s, a) against the f64 one, the agent contract through tests/agent_contract.py
(train against the host trait loop / launch depths / shards, the checkpoint, foreign files, the C++ example), the refusals and the loop's 2a - 1.

The f32 chain of psi, ln and exp has no derivable bound: the bounds of MEASURED below are four times the maxima profiles/nac_beta_rate.md records
(the factor covers inputs the measurement did not see); every test prints its figure before it asserts.

The contract's adapter: the contract tests run on NacCtx, a thin subclass of Context whose get_weights(i) returns the (5F, 1) stack of the critic's w
and the policy's two columns, and assert on that stack.  (tests/agent_contract.learner_state has since learnt algo 28 -- `weights` and `theta` -- so
the snapshot carries the columns a second time under `theta`; the adapter stays for what these tests assert on the stack.)  Every other test uses
the plain Context."""
import functools
import os

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import RsrlHipError, _abi
from tests import beta_numpy as bn
from tests import nac_numpy as nn
from tests.agent_contract import check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, run_example

pytestmark = pytest.mark.gpu

CMC, NAC, BETA = rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, rsrl_amd.NAC, rsrl_amd.BETA
ORDERS = [1, 3, 5]           # F = 4, 16, 36
N = 67                       # one full wave and a partial one
ESTATE, EINVAL = -5, -1

# four times the measured maxima (profiles/nac_beta_rate.md)
MEASURED = {
    ("w", 1): 4 * 6.134e-8, ("w", 3): 4 * 1.168e-7, ("w", 5): 4 * 6.448e-8,                  # max |dw| / max(1, |w|) after three rounds of handle
    ("delta", 1): 4 * 5.823e-7, ("delta", 3): 4 * 4.896e-7, ("delta", 5): 4 * 2.611e-7,      # max |d delta| / max(1, |delta|) over the three rounds
    ("q", 1): 4 * 1.842e-7, ("q", 3): 4 * 1.647e-7, ("q", 5): 4 * 9.224e-8,                  # max |dQ| / max(1, |Q|)
}

BASE = dict(domain=CMC, order=3, algo=NAC, policy=BETA, n_envs=N, seed=5, gamma=0.95, lr=0.01, alpha=0.1, n_steps=100)


def ctx(**kw):
    return rsrl_amd.Context(**dict(BASE, **kw))


class NacCtx(rsrl_amd.Context):
    """the contract's adapter (the module's docstring)"""

    def get_weights(self, env_index=0):
        return np.concatenate([super().get_weights(env_index), self.get_policy_weights(env_index).T.reshape(-1, 1)])


def nac_ctx(**kw):
    return NacCtx(**dict(BASE, **kw))


def hold(name, figure):
    print("measured %s: %.4g (bound %.4g)" % (name, figure, MEASURED[name]))
    assert figure <= MEASURED[name], (name, figure, MEASURED[name])


# ---- 1. the actor's update
@pytest.mark.parametrize("order", ORDERS)
def test_actor_update_is_the_float32_restatement_bit_for_bit(order):
    rng = np.random.default_rng(70 + order)
    with ctx(order=order) as c:
        F = c.F
        assert c.n_weight_rows == 3 * F and c.n_out == 1 and c.n_policy_out == 2 and c.A == 0
        w = (rng.normal(size=(N, 3 * F, 1)) * rng.uniform(0.01, 3.0, size=(N, 1, 1))).astype(np.float32)
        w[0] = 0.0                                                                       # g = 0: norm = 1e-3, no movement
        unit = w[1, :2 * F, 0].astype(np.float64) / np.linalg.norm(w[1, :2 * F, 0].astype(np.float64))
        w[1, :2 * F, 0] = (unit * 0.9999e-3).astype(np.float32)                          # ||g|| just below the floor
        w[2, :2 * F, 0] = (unit * 1.0001e-3).astype(np.float32)                          # ... and just above
        w[3, :2 * F, 0] = (unit * 1e3).astype(np.float32)                                # |g| near 1e3
        w[4, :2 * F, 0] = 0.0                                                            # g = 0 next to a live basis block
        pol = rng.normal(size=(N, F, 2)).astype(np.float32)
        for i in range(N):
            c.set_weights(w[i], i)
            c.set_policy_weights(pol[i], i)
        mask = (np.arange(N) % 3 != 2).astype(np.uint8)
        mask[:5] = 1
        norm = c.nac_update(mask)
        for i in range(N):
            got = c.get_policy_weights(i)
            if mask[i]:
                want, wn = nn.nac_handle_f32(w[i], pol[i], BASE["alpha"])
                assert got.tobytes() == want.tobytes(), (i, np.abs(got - want).max())
                assert norm[i].tobytes() == wn.tobytes(), (i, norm[i], wn)
            else:
                assert got.tobytes() == pol[i].tobytes() and norm[i] == 0.0, i
            assert c.get_weights(i).tobytes() == w[i].tobytes(), i                       # the critic's weights are not reset
        assert norm[0] == np.float32(1e-3) and norm[4] == np.float32(1e-3) and norm[1] == np.float32(1e-3) and norm[2] > np.float32(1e-3)
        assert np.array_equal(c.get_policy_weights(0), pol[0]) and np.array_equal(c.get_policy_weights(4), pol[4])
        assert abs(norm[3] - 1e3) < 1.0 and c.step_count == 0
        # mask = NULL: every learner
        norm2 = c.nac_update()
        assert np.all(norm2 > 0) and not np.array_equal(c.get_policy_weights(2 + 3), pol[5])


# ---- 2., 3. the critic
@functools.lru_cache(maxsize=None)
def _case(order):
    return nn.handle_case(order)


@pytest.mark.parametrize("order", ORDERS)
def test_critic_rule_against_the_f64_restatement(order):
    case = _case(order)
    F, p = case["F"], case["params"]
    with ctx(order=order, seed=nn.RULE_SEED, gamma=p["gamma"], lr=p["lr"]) as c:
        for i, (w, W) in enumerate(case["init"]):
            c.set_weights(w.reshape(-1, 1), i)
            c.set_policy_weights(W, i)
        phi_s, phi_n, td = [], [], []
        for frm, a, rew, nxt, term in case["rounds"]:
            phi_s.append(c.project(frm))
            phi_n.append(c.project(nxt))
            td.append(c.handle(frm, a, rew, nxt, term))
        assert c.step_count == len(case["rounds"])
        got = np.stack([c.get_weights(i)[:, 0] for i in range(N)]).astype(np.float64)
        for i, (_, W) in enumerate(case["init"]):
            assert c.get_policy_weights(i).tobytes() == W.tobytes(), i                   # critic.handle does not move the actor
    want, deltas, skipped = nn.critic_after(case, nn.RULE_SEED, phi_s, phi_n)
    keep = ~skipped
    print("learners left out (an inner draw within %g of an acceptance boundary): %d" % (nn.MARGIN, skipped.sum()))
    assert skipped.sum() <= 3
    w0 = np.stack([x for x, _ in case["init"]]).astype(np.float64)
    assert np.max(np.abs(want[keep] - w0[keep])) > 1e-3                                  # w moved far more than the bound
    fig_d = max(float(np.max(np.abs(t.astype(np.float64) - d)[keep] / np.maximum(1.0, np.abs(d[keep])))) for t, d in zip(td, deltas))
    fig_w = float(np.max(np.abs(got[keep] - want[keep]) / np.maximum(1.0, np.abs(want[keep]))))
    print("measured (delta, %d): %.4g   measured (w, %d): %.4g" % (order, fig_d, order, fig_w))
    hold(("delta", order), fig_d)
    hold(("w", order), fig_w)


@pytest.mark.parametrize("order", ORDERS)
def test_q_evaluate_f32_against_the_f64_restatement(order):
    case = _case(order)
    frm, a, _, _, _ = case["rounds"][0]
    a = a.copy()
    a[2], a[3], a[4] = -0.5, 1.5, 0.5                                                    # outside [0, 1]: clamped like 0 and 1
    with ctx(order=order) as c:
        for i, (w, W) in enumerate(case["init"]):
            c.set_weights(w.reshape(-1, 1), i)
            c.set_policy_weights(W, i)
        phi = c.project(frm).astype(np.float64)
        q = c.q_evaluate_f32(frm, a)
        before = c.checksum()
        assert np.array_equal(c.q_evaluate_f32(frm, a), q) and c.checksum() == before and c.step_count == 0      # read-only
    want = np.array([nn.q_value(w, W, phi[:, i], float(a[i])) for i, (w, W) in enumerate(case["init"])])
    assert np.isfinite(q).all() and abs(q[2] - nn.q_value(*case["init"][2], phi[:, 2], 0.0)) <= 1e-4 * max(1.0, abs(want[2]))
    hold(("q", order), float(np.max(np.abs(q.astype(np.float64) - want) / np.maximum(1.0, np.abs(want)))))


# ---- 4. the agent contract
P, CAP, K = 5, 7, 48


def _start_near_the_goal(c, off):
    """reset, then every fourth learner (by global id) at x = 0.59, v = 0.06: terminal ends occur as well as cut ones"""
    c.reset()
    s = c.states
    s[:, (np.arange(c.N) + off) % 4 == 0] = np.array([[0.59], [0.06]], dtype=np.float32)
    c.states = s


def _nac_trait(c, k_steps, cap):
    """the loop of nac_beta.rs through the trait calls: domain_step(NULL) (the pending actions through 2a - 1), critic.handle, the restarts, the
    behaviour sample, then NAC::handle(()) for the learners whose step was the P-th of its episode, counted from 0"""
    ep = c.episode_steps.astype(np.int64)
    for _ in range(k_steps):
        update = (ep % P == 0).astype(np.uint8)
        a = c.actions
        frm, nxt, rew, term = c.domain_step()
        c.handle(frm, a, rew, nxt, term)
        ep += 1
        mask = (term.astype(bool) | ((ep >= cap) if cap > 0 else False)).astype(np.uint8)
        c.domain_reset(mask)
        ep[mask == 1] = 0
        c.policy_sample()
        c.nac_update(update)
    c.episode_steps = ep.astype(np.uint32)


@pytest.mark.parametrize("order", ORDERS)
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(order):
    """(66 learners: the harness joins two shards of N / 2.)  The first split, 13, lands between two updates of the learners that started at the start
    state: their second episode is at step 6, past the update at 5 and before the next episode's at 0"""
    n = 66
    kw = dict(order=order, n_envs=n, max_episode_steps=CAP, n_steps=P, lr=0.02, alpha=0.1, gamma=0.97)
    st, ref = check_train_invariance(nac_ctx, kw, K, CAP, depths=(1, 3, 0), first_split=13, kernel="k_train_nac_beta", setup=_start_near_the_goal,
                                     trait=_nac_trait)
    F = (order + 1) ** 2
    # terminals and truncations both occur; a truncated episode ran CAP = 7 > P steps, so it saw the actor's update at i = 0 and at i = 5
    assert st["env_steps"] == n * K and st["episodes"] > st["episodes_truncated"] > 0 and st["sum_abs_td_error"] > 0
    assert st["sum_episode_steps"] >= CAP * st["episodes_truncated"] + (st["episodes"] - st["episodes_truncated"])
    w = ref["weights"]
    assert w.shape == (n, 5 * F, 1) and np.isfinite(w).all() and np.abs(w[:, :3 * F]).max() > 0 and np.abs(w[:, 3 * F:]).max() > 0
    assert ref["actions"].dtype == np.float32 and ref["actions"].min() >= bn.LO and ref["actions"].max() <= bn.HI


def test_checkpoint_resumes_bitwise_and_foreign_files_are_refused(tmp_path):
    kw = dict(n_envs=32, order=3, max_episode_steps=17, n_steps=P, lr=0.02)
    path = os.path.join(str(tmp_path), "nac_beta.ckpt")
    check_checkpoint_resume(nac_ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"))
    with open(path, "rb") as f:
        head = f.read(72)
    F = 16
    assert int.from_bytes(head[12:16], "little") == CMC and int.from_bytes(head[44:48], "little") == NAC and int.from_bytes(head[52:56], "little") == 12
    assert os.path.getsize(path) == 72 + 32 * 4 * 3 * F + 32 * 4 * F * 2
    tdac_beta = dict(domain=CMC, order=3, algo=rsrl_amd.ILSTD_ACTOR_CRITIC, policy=BETA, n_envs=32, n_steps=2, lr=0.02, alpha=0.2)
    ilstd = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=rsrl_amd.ILSTD, policy=rsrl_amd.RANDOM, n_envs=32, n_steps=3, alpha=0.02)
    qlearning = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=rsrl_amd.QLEARNING, policy=rsrl_amd.GREEDY, n_envs=32)
    check_foreign_checkpoints_refused(nac_ctx, kw, path, [tdac_beta, ilstd, qlearning], tmp_path)


def test_example_builds_and_runs(tmp_path):
    out = run_example(tmp_path, "nac_beta", [8, 2, 300])
    lines = out.strip().splitlines()
    assert len(lines) == 3 and lines[0].startswith("Batch 1:") and lines[1].startswith("Batch 2:") and lines[2].startswith("OOS:")
    assert "nan" not in out.lower()


# ---- 5. the refusals
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

    with ctx(max_episode_steps=20) as c:
        h, F = c._h, c.F
        before = c.checksum()
        for call in (lambda: L.rsrl_hip_get_actions(h, p(out_i)), lambda: L.rsrl_hip_set_actions(h, p(ai)),
                     lambda: L.rsrl_hip_domain_step(h, p(ai), p(S.copy()), p(S.copy()), p(r), p(t)),
                     lambda: L.rsrl_hip_handle(h, p(S), p(ai), p(r), p(S), p(t), N, p(out_f)),
                     lambda: L.rsrl_hip_policy_sample(h, p(S), N, p(out_i)), lambda: L.rsrl_hip_policy_sample(h, None, N, p(out_i)),
                     lambda: L.rsrl_hip_policy_mode(h, p(S), N, p(out_i))):
            refused(call)                                                                # the int32 calls
        for call in (lambda: c.q_evaluate(S), lambda: c.q_find_max(S), lambda: c.q_find_min(S),
                     lambda: L.rsrl_hip_q_expected_value(h, p(S), N, p(np.zeros((3, N), dtype=np.float32)), p(out_f)),
                     lambda: c.handle_batch(np.zeros((1, 2, N)), np.zeros((1, N)), np.zeros((1, N)), np.zeros(N)),
                     lambda: c.rollout_trajectory(5), lambda: c.rollout_policy(rsrl_amd.RANDOM, 5),
                     lambda: c.get_traces(0), lambda: L.rsrl_hip_get_td_weights(h, 0, p(out_f)), lambda: c.get_lstd_state(0)):
            refused(call)
        x = af.copy()
        x[5] = np.nan
        refused(lambda: L.rsrl_hip_q_evaluate_f32(h, p(S), p(x), N, p(out_f)), EINVAL)
        assert c.checksum() == before and c.step_count == 0
        assert c.n_weight_rows == 3 * F and c.get_weights(0).shape == (3 * F, 1) and not c.get_weights(0).any()
    with rsrl_amd.Context(domain=CMC, order=3, algo=rsrl_amd.ILSTD_ACTOR_CRITIC, policy=BETA, n_envs=N, n_steps=2) as g:
        assert g.n_weight_rows == g.F
        refused(lambda: L.rsrl_hip_nac_update(g._h, None, p(out_f)))
        refused(lambda: L.rsrl_hip_q_evaluate_f32(g._h, p(S), p(af), N, p(out_f)))
    with rsrl_amd.Context(n_envs=4, order=3) as q:
        assert q.n_weight_rows == q.F == 16
        refused(lambda: L.rsrl_hip_nac_update(q._h, None, None))


# ---- 6. the loop's mapping
def test_pending_actions_step_through_two_a_minus_one_and_the_rollout_is_the_mode_loop():
    rng = np.random.default_rng(21)
    S = rng.uniform([-1.2, -0.07], [0.6, 0.07], size=(N, 2)).T.astype(np.float32)
    S[:, 0], S[:, 1], S[:, 2] = (0.59, 0.06), (-1.2, -0.07), (-0.5, 0.0)
    a = rng.uniform(0.0, 1.0, size=N).astype(np.float32)
    a[0], a[1], a[2] = 1.0, 0.0, 0.5
    limit = 40
    with ctx(order=3, max_episode_steps=limit - 1) as c:
        c.states, c.actions = S, a
        r1 = c.domain_step()
        assert np.array_equal(c.actions, a)                                              # the pending actions stay the agent's
        c.states = S
        r2 = c.domain_step((2.0 * a - 1.0).astype(np.float32))                           # explicit actions: the domain's, literally
        for x, y in zip(r1, r2):
            assert x.tobytes() == y.tobytes()
        assert r1[3][0] == 1 and r1[2][0] == 0.0 and r1[3].sum() < N
        # rollout_greedy = a host loop of policy_mode + domain_step(2 m - 1) from the start state
        for i in range(N):
            c.set_policy_weights((rng.normal(size=(c.F, 2)) * 0.5).astype(np.float32), i)
        for lim in (limit, 0):                                                           # (0: bounded by max_episode_steps, limit - 1 transitions)
            n_states, total = c.rollout_greedy(lim)
            c.reset()
            n_host, tot_host, live = np.ones(N, dtype=np.uint32), np.zeros(N, dtype=np.float32), np.ones(N, dtype=bool)
            for _ in range(limit - 1):
                m = c.policy_mode(c.states)
                _, _, rew, term = c.domain_step((2.0 * m - 1.0).astype(np.float32))
                n_host[live] += 1
                tot_host[live] += rew[live]
                live &= term == 0
            assert np.array_equal(n_states, n_host) and total.tobytes() == tot_host.tobytes(), lim
        assert n_states.max() == limit and len(np.unique(c.policy_mode(c.states))) > N // 2
