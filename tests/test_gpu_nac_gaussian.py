"""NAC with the Gaussian policy and the SCB SARSA critic (RSRL_NAC with RSRL_GAUSSIAN, train_nac.hip) on the device, against
tests/gaussian_numpy.py: the actor's update bit for bit against the float32 restatement (tests/nac_numpy.nac_handle_f32), the critic's rule,
Q(s, a) and the policy side against the f64 one, the agent contract through tests/agent_contract.py (train against the host trait loop / launch
depths / shards, the checkpoint, foreign files, the C++ example), the refusals, and the loop that hands the domain the action itself.

The f32 chain (ln, exp, the division by Sigma^2) has no derivable bound: the bounds of MEASURED below are four times the maxima
profiles/nac_gaussian_rate.md records (scripts/nac_gaussian_rate.py, on these very inputs; the factor covers inputs the measurement did not see);
every test prints its figure before it asserts.  The sampler has no acceptance test, so the rule test leaves no learner out."""
import functools
import os

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import RsrlHipError, _abi
from tests import beta_numpy as bn
from tests import gaussian_numpy as gn
from tests import nac_numpy as nn
from tests.agent_contract import check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, run_example

pytestmark = pytest.mark.gpu

CMC, NAC, GAUSSIAN, BETA = rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, rsrl_amd.NAC, 6, rsrl_amd.BETA
ORDERS = [1, 3, 5]           # F = 4, 16, 36
N = 67                       # one full wave and a partial one
ESTATE, EINVAL = -5, -1

# four times the measured maxima (profiles/nac_gaussian_rate.md), each max |d x| / max(1, |x|) against the f64 restatement
MEASURED = {
    ("w", 1): 4 * 6.279e-8, ("w", 3): 4 * 1.907e-8, ("w", 5): 4 * 9.054e-9,                      # w after three rounds of handle
    ("delta", 1): 4 * 3.081e-7, ("delta", 3): 4 * 1.536e-7, ("delta", 5): 4 * 1.148e-7,          # td_error_out over the three rounds
    ("q", 1): 4 * 1.012e-7, ("q", 3): 4 * 7.731e-8, ("q", 5): 4 * 3.128e-8,                      # q_evaluate_f32
    ("mu", 1): 4 * 6.276e-8, ("mu", 3): 4 * 2.962e-8, ("mu", 5): 4 * 1.990e-8,                   # policy_params, policy_mode_f32
    ("sd", 1): 4 * 1.373e-7, ("sd", 3): 4 * 1.765e-7, ("sd", 5): 4 * 2.142e-7,
    ("pdf", 1): 4 * 5.469e-8, ("pdf", 3): 4 * 4.138e-8, ("pdf", 5): 4 * 3.664e-8,                # policy_pdf
    ("sample", 1): 4 * 1.099e-6, ("sample", 3): 4 * 9.935e-7, ("sample", 5): 4 * 8.648e-7,       # policy_sample_f32, 64 calls
}

BASE = dict(domain=CMC, order=3, algo=NAC, policy=GAUSSIAN, n_envs=N, seed=5, gamma=0.95, lr=0.01, alpha=0.1, n_steps=100)


def ctx(**kw):
    return rsrl_amd.Context(**dict(BASE, **kw))


def hold(name, figure):
    print("measured %s: %.4g (bound %.4g)" % (name, figure, MEASURED[name]))
    assert figure <= MEASURED[name], (name, figure, MEASURED[name])


# ---- 1. the actor's update
@pytest.mark.parametrize("order", ORDERS)
def test_actor_update_is_the_float32_restatement_bit_for_bit(order):
    rng = np.random.default_rng(90 + order)
    with ctx(order=order) as c:
        F = c.F
        assert c.n_weight_rows == 3 * F and c.n_out == 1 and c.n_policy_out == 2 and c.A == 0
        assert not c.get_weights(0).any() and not c.get_policy_weights(0).any()           # both zero at create
        w = (rng.normal(size=(N, 3 * F, 1)) * rng.uniform(0.01, 3.0, size=(N, 1, 1))).astype(np.float32)
        w[0] = 0.0                                                                       # g = 0: norm = 1e-3, no movement
        unit = w[1, :2 * F, 0].astype(np.float64) / np.linalg.norm(w[1, :2 * F, 0].astype(np.float64))
        w[1, :2 * F, 0] = (unit * 0.9999e-3).astype(np.float32)                          # ||g|| just below the floor
        w[2, :2 * F, 0] = (unit * 1.0001e-3).astype(np.float32)                          # ... and just above
        w[3, :2 * F, 0] = (unit * 1e3).astype(np.float32)                                # ||g|| near 1e3
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
            assert c.get_weights(i).tobytes() == w[i].tobytes(), i                       # the critic's weights are untouched
        assert norm[0] == np.float32(1e-3) and norm[4] == np.float32(1e-3) and norm[1] == np.float32(1e-3) and norm[2] > np.float32(1e-3)
        assert np.array_equal(c.get_policy_weights(0), pol[0]) and np.array_equal(c.get_policy_weights(4), pol[4])
        assert abs(norm[3] - 1e3) < 1.0 and c.step_count == 0
        # mask = NULL: every learner
        after = np.stack([c.get_policy_weights(i) for i in range(N)])
        norm2 = c.nac_update()
        for i in range(N):
            want, wn = nn.nac_handle_f32(w[i], after[i], BASE["alpha"])
            assert c.get_policy_weights(i).tobytes() == want.tobytes() and norm2[i].tobytes() == wn.tobytes(), i
        assert np.all(norm2 > 0) and not np.array_equal(c.get_policy_weights(5), pol[5])


# ---- 2., 3., 4. the critic and the policy side against the f64 restatement: one pass over handle_case's inputs per order, shared and left unchanged
@functools.lru_cache(maxsize=None)
def _case(order):
    return gn.handle_case(order)


@functools.lru_cache(maxsize=None)
def _figures(order):
    case = _case(order)
    p = case["params"]
    with ctx(order=order, seed=gn.RULE_SEED, gamma=p["gamma"], lr=p["lr"]) as c:
        fig, arr = gn.figures(c, case, gn.RULE_SEED)
        arr["steps"] = c.step_count
        arr["columns"] = [c.get_policy_weights(i) for i in range(N)]
    for k, v in sorted(fig.items()):
        print("measured (%s, %d): %.4g" % (k, order, v))
    return fig, arr


@pytest.mark.parametrize("order", ORDERS)
def test_critic_rule_against_the_f64_restatement(order):
    case = _case(order)
    fig, arr = _figures(order)
    assert arr["steps"] == len(case["rounds"]) == 3
    for i, (_, W) in enumerate(case["init"]):
        assert arr["columns"][i].tobytes() == W.tobytes(), i                             # critic.handle does not move the actor
    w0 = np.stack([x for x, _ in case["init"]]).astype(np.float64)
    assert arr["want"].shape == (N, 3 * case["F"]) and np.max(np.abs(arr["want"] - w0)) > 1e-3      # every learner; w moved far more than the bound
    assert all(t.shape == (N,) and np.isfinite(t).all() for t in arr["td"])
    hold(("delta", order), fig["delta"])
    hold(("w", order), fig["w"])


@pytest.mark.parametrize("order", ORDERS)
def test_q_evaluate_f32_against_the_f64_restatement(order):
    case = _case(order)
    fig, arr = _figures(order)
    aq = arr["aq"]
    assert aq[2] == -2.5 and aq[3] == 1.5 and np.isfinite(arr["q"]).all()               # outside [-1, 1]: taken as they are
    frm = case["rounds"][0][0]
    with ctx(order=order) as c:
        for i, (w, W) in enumerate(case["init"]):
            c.set_weights(w.reshape(-1, 1), i)
            c.set_policy_weights(W, i)
        q = c.q_evaluate_f32(frm, aq)
        before = c.checksum()
        assert np.array_equal(c.q_evaluate_f32(frm, aq), q) and c.checksum() == before and c.step_count == 0      # read-only
        assert q.tobytes() == arr["q"].tobytes()
        inside = aq.copy()
        inside[2], inside[3] = -1.0, 1.0
        q_in = c.q_evaluate_f32(frm, inside)
        assert q_in[2] != q[2] and q_in[3] != q[3] and np.array_equal(q_in[5:], q[5:])   # not clamped
    hold(("q", order), fig["q"])


@pytest.mark.parametrize("order", ORDERS)
def test_policy_side_against_the_f64_restatement(order):
    case = _case(order)
    fig, arr = _figures(order)
    frm, a, _, _, _ = case["rounds"][0]
    hold(("mu", order), fig["mu"])
    hold(("sd", order), fig["sd"])
    hold(("pdf", order), fig["pdf"])
    hold(("sample", order), fig["sample"])
    mu, sd, smp = arr["dmu"].astype(np.float64), arr["dsd"].astype(np.float64), arr["sample"].astype(np.float64)
    assert arr["sample"].shape == (gn.SAMPLE_CALLS, N) and sd.min() >= 0.32
    # the derived range: |z| <= sqrt(48 ln 2) < 5.77, one f32 fma behind it
    worst = float(np.max(np.abs(smp - mu) / sd))
    print("max |a - mu| / sd: %.4g (bound %.4g)" % (worst, 5.77 * (1 + 2.0 ** -20)))
    assert np.all(np.abs(smp - mu) <= 5.77 * sd * (1 + 2.0 ** -20))
    # the pooled standardised draws, n = 67 learners x 64 calls = 4 288: mean and variance within five standard errors of 0 and 1
    z = ((smp - mu) / sd).ravel()
    n = z.size
    print("n = %d: mean %.4g (bound %.4g), variance - 1 %.4g (bound %.4g)" % (n, z.mean(), 5 / np.sqrt(n), z.var() - 1, 5 * np.sqrt(2.0 / n)))
    assert n == 4288 and abs(z.mean()) <= 5.0 / np.sqrt(n) and abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert len(np.unique(arr["sample"])) > 0.99 * n and (np.abs(smp) > 1.0).any()        # not clamped
    with ctx(order=order, seed=gn.RULE_SEED) as c, ctx(order=order, seed=gn.RULE_SEED) as d, ctx(order=order, seed=gn.RULE_SEED + 1) as e:
        for x in (c, d, e):
            for i, (_, W) in enumerate(case["init"]):
                x.set_policy_weights(W, i)
        m = c.policy_mode(frm)
        assert m.tobytes() == arr["dmu"].tobytes()                                       # the mode is mu
        before = c.checksum()
        assert c.policy_pdf(frm, a).tobytes() == c.policy_pdf(frm, a).tobytes() and c.checksum() == before
        # the same (seed, id, t, purpose): the same bits, in another ctx too; another seed: other draws
        s0, s1 = c.policy_sample(frm), c.policy_sample(frm)
        assert s0.tobytes() == arr["sample"][0].tobytes() and s1.tobytes() == arr["sample"][1].tobytes() and s0.tobytes() != s1.tobytes()
        assert d.policy_sample(frm).tobytes() == s0.tobytes() and e.policy_sample(frm).tobytes() != s0.tobytes()
        assert c.step_count == 0


# ---- 5. the agent contract
P, CAP, K = 5, 7, 48


def _start_near_the_goal(c, off):
    """reset, then every fourth learner (by global id) at x = 0.59, v = 0.06: terminal ends occur as well as cut ones"""
    c.reset()
    s = c.states
    s[:, (np.arange(c.N) + off) % 4 == 0] = np.array([[0.59], [0.06]], dtype=np.float32)
    c.states = s


def _nac_trait(c, k_steps, cap):
    """the loop of nac.rs through the trait calls: domain_step(NULL) -- the pending actions, NO mapping --, critic.handle, the restarts, the behaviour
    sample, then NAC::handle(()) for the learners whose step was the P-th of its episode, counted from 0"""
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
    st, ref = check_train_invariance(ctx, kw, K, CAP, depths=(1, 3, 0), first_split=13, kernel="k_train_nac_gauss", setup=_start_near_the_goal,
                                     trait=_nac_trait)
    F = (order + 1) ** 2
    # terminals and truncations both occur; a truncated episode ran CAP = 7 > P steps, so it saw the actor's update at i = 0 and at i = 5
    assert st["env_steps"] == n * K and st["episodes"] > st["episodes_truncated"] > 0 and st["sum_abs_td_error"] > 0
    assert st["sum_episode_steps"] >= CAP * st["episodes_truncated"] + (st["episodes"] - st["episodes_truncated"])
    w, th = ref["weights"], ref["theta"]
    assert w.shape == (n, 3 * F, 1) and th.shape == (n, F, 2) and np.isfinite(w).all() and np.isfinite(th).all()
    assert np.abs(w).max() > 0 and np.abs(th[:, :, 0]).max() > 0 and np.abs(th[:, :, 1]).max() > 0
    assert ref["actions"].dtype == np.float32 and np.isfinite(ref["actions"]).all()


def test_checkpoint_resumes_bitwise_and_foreign_files_are_refused(tmp_path):
    kw = dict(n_envs=32, order=3, max_episode_steps=17, n_steps=P, lr=0.02)
    path = os.path.join(str(tmp_path), "nac_gauss.ckpt")
    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"))
    with open(path, "rb") as f:
        head = f.read(72)
    F = 16
    assert int.from_bytes(head[8:12], "little") == 10 and int.from_bytes(head[12:16], "little") == CMC
    assert int.from_bytes(head[44:48], "little") == NAC and int.from_bytes(head[52:56], "little") == 14
    assert os.path.getsize(path) == 72 + 32 * 4 * 3 * F + 32 * 4 * F * 2
    nac_beta = dict(domain=CMC, order=3, algo=NAC, policy=BETA, n_envs=32, n_steps=P, lr=0.02)      # the same sections, aux_kind 12: refused both ways
    tdac_beta = dict(domain=CMC, order=3, algo=rsrl_amd.ILSTD_ACTOR_CRITIC, policy=BETA, n_envs=32, n_steps=2, lr=0.02, alpha=0.2)
    qlearning = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=rsrl_amd.QLEARNING, policy=rsrl_amd.GREEDY, n_envs=32)
    check_foreign_checkpoints_refused(ctx, kw, path, [nac_beta, tdac_beta, qlearning], tmp_path)


# ---- 6. the loop hands the domain the action itself
def test_pending_actions_step_literally_and_the_rollout_is_the_mode_loop():
    rng = np.random.default_rng(31)
    S = rng.uniform([-1.2, -0.07], [0.6, 0.07], size=(N, 2)).T.astype(np.float32)
    S[:, 0], S[:, 1], S[:, 2] = (0.59, 0.06), (-1.2, -0.07), (-0.5, 0.0)
    a = rng.uniform(-1.5, 1.5, size=N).astype(np.float32)
    a[0], a[1], a[2], a[3] = 1.0, -1.0, 0.0, 7.25
    limit = 40
    with ctx(order=3, max_episode_steps=limit - 1) as c:
        c.states, c.actions = S, a
        assert c.actions.tobytes() == a.tobytes()                                        # any finite f32, as it is: no clamp
        r1 = c.domain_step()
        assert c.actions.tobytes() == a.tobytes()
        c.states = S
        r2 = c.domain_step(a)
        c.states = S
        r3 = c.domain_step(np.clip(a, -1.0, 1.0))                                        # the domain clips (map_onto)
        for x, y, z in zip(r1, r2, r3):
            assert x.tobytes() == y.tobytes() == z.tobytes()
        c.states = S
        r4 = c.domain_step((2.0 * a - 1.0).astype(np.float32))                           # NOT the Beta loop's mapping
        assert r4[1].tobytes() != r1[1].tobytes()
        assert r1[3][0] == 1 and r1[2][0] == 0.0 and r1[3].sum() < N
        # rollout_greedy = a host loop of policy_mode + domain_step(m) from the start state
        for i in range(N):
            c.set_policy_weights((rng.normal(size=(c.F, 2)) * 0.5).astype(np.float32), i)
        for lim in (limit, 0):                                                           # (0: bounded by max_episode_steps, limit - 1 transitions)
            n_states, total = c.rollout_greedy(lim)
            c.reset()
            n_host, tot_host, live = np.ones(N, dtype=np.uint32), np.zeros(N, dtype=np.float32), np.ones(N, dtype=bool)
            for _ in range(limit - 1):
                m = c.policy_mode(c.states)
                _, _, rew, term = c.domain_step(m)
                n_host[live] += 1
                tot_host[live] += rew[live]
                live &= term == 0
            assert np.array_equal(n_states, n_host) and total.tobytes() == tot_host.tobytes(), lim
        assert n_states.max() == limit and len(np.unique(c.policy_mode(c.states))) > N // 2


# ---- 7. the refusals
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
        c.reset()
        before, acts = c.checksum(), c.actions
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
            refused(call)                                                                # the Beta agent's ESTATE list
        for bad in (np.nan, np.inf, -np.inf):
            x = af.copy()
            x[5] = bad
            refused(lambda: L.rsrl_hip_q_evaluate_f32(h, p(S), p(x), N, p(out_f)), EINVAL)
            refused(lambda: L.rsrl_hip_handle_f32(h, p(S), p(x), p(r), p(S), p(t), N, p(out_f)), EINVAL)
            refused(lambda: L.rsrl_hip_set_actions_f32(h, p(x)), EINVAL)
            refused(lambda: L.rsrl_hip_domain_step_f32(h, p(x), None, None, None, None), EINVAL)
            refused(lambda: L.rsrl_hip_policy_pdf(h, p(S), p(x), N, p(out_f)), EINVAL)
        assert c.checksum() == before and c.step_count == 0 and c.actions.tobytes() == acts.tobytes()
        assert c.n_weight_rows == 3 * F and c.get_weights(0).shape == (3 * F, 1) and not c.get_weights(0).any()
    # RSRL_GAUSSIAN on a ctx that is no NAC: refused at create
    for kw in (dict(algo=rsrl_amd.ILSTD_ACTOR_CRITIC, n_steps=2), dict(algo=rsrl_amd.QLEARNING), dict(domain=rsrl_amd.MOUNTAIN_CAR),
               dict(domain=rsrl_amd.MOUNTAIN_CAR, algo=rsrl_amd.SARSA)):
        with pytest.raises(RsrlHipError) as e:
            ctx(**kw)
        assert e.value.code == EINVAL and "RSRL_GAUSSIAN" in str(e.value), kw
    for kw in (dict(policy=5), dict(policy=7)):
        with pytest.raises(RsrlHipError) as e:
            ctx(**kw)
        assert e.value.code == EINVAL and "unknown policy" in str(e.value), kw


# ---- 8. reset
def test_reset_samples_on_blk_init_and_leaves_the_learner_alone():
    order = 3
    case = _case(order)
    with ctx(order=order, seed=11) as c:
        for i, (w, W) in enumerate(case["init"]):
            c.set_weights(w.reshape(-1, 1), i)
            c.set_policy_weights(W, i)
        c.reset()
        S = c.states
        assert np.all(S[0] == np.float32(-0.5)) and np.all(S[1] == 0.0) and not c.episode_steps.any() and c.step_count == 0
        for i, (w, W) in enumerate(case["init"]):
            assert c.get_weights(i).tobytes() == w.reshape(-1, 1).tobytes() and c.get_policy_weights(i).tobytes() == W.tobytes(), i
        dmu, dsd = c.policy_params(S)
        phi = c.project(S).astype(np.float64)
        Ws = [W.astype(np.float64) for _, W in case["init"]]
        mu, sd = gn.gauss_params(np.array([phi[:, i] @ Ws[i][:, 0] for i in range(N)]), np.array([phi[:, i] @ Ws[i][:, 1] for i in range(N)]))
        want = gn.gauss_sample(11, np.arange(N), 0, bn.BLK_INIT, mu, sd)
        a = c.actions
        hold(("sample", order), float(np.max(np.abs(a.astype(np.float64) - want) / np.maximum(1.0, np.abs(want)))))
        assert not np.array_equal(a, gn.gauss_sample(11, np.arange(N), 0, bn.BLK_STEP, mu, sd).astype(np.float32))
        # policy_sample() before the first handle repeats the initial stream, bit for bit
        assert c.policy_sample().tobytes() == a.tobytes() and c.policy_sample().tobytes() == a.tobytes()
        assert np.all(np.abs(a.astype(np.float64) - dmu) <= 5.77 * dsd.astype(np.float64) * (1 + 2.0 ** -20))


# ---- 9. the example
def test_example_builds_and_runs(tmp_path):
    out = run_example(tmp_path, "nac", [8, 2, 300])
    lines = out.strip().splitlines()
    assert len(lines) == 3 and lines[0].startswith("Batch 1:") and lines[1].startswith("Batch 2:") and lines[2].startswith("OOS:")
    assert "nan" not in out.lower()
