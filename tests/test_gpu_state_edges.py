"""The HIP path on the crafted states of tests/state_edges.py: every learner is one table row.

  transitions   rsrl_hip_domain_step on one ctx per kernel family and domain, the whole table under every action: bit for bit the oracle's device-order
                instantiation (f32d: next state, reward, terminal -- on bit patterns, so that -0.0 counts), and DIRECTLY against f64 at the measured
                bars with the three decision assertions (state_edges.py)
  bases         rsrl_hip_project on every register-family order, generic orders up to the largest admitted and the order-7 wave family: bit for bit
                f32d, within the bar of f64, the constant feature exactly 1.0 last; rsrl_hip_tile_indices exact
  driver loops  the ctx's states set to the table, the same on the oracle's device-order loop of the family, train(1) then train(2) (the second
                call steps from the states the first left: just-reset ones among them, so the fused loop's hoisted Pre of a reset state is
                used): states, actions, episode counters, weights (they carry the in-loop features) identical ON BIT PATTERNS (bit_differences: -0.0 is not
                0.0).  One row per kernel name of tests/test_gpu_counter_edges.py's case table (MountainCar, Acrobot) and CartPole rows of this
                file's own: the wave family's plain Dom::step f32 and bf16 (step_uniform is Acrobot's), the fused register loop, the generic
                loop, the tile coder, the lambda and TD kernels.  Per-learner weights: learner i is row i // A under action i % A -- the Greedy
                policy over weights that are zero but for 1.0 in the bias row of column i % A, and that action pending; shared weights: the table
                eight times under the Random policy, copy k with action k % A pending.  The pending actions are installed on both sides, so the
                first batch-step steps every (row, action) pair by construction (asserted; more than the 90 % asked for); the later steps'
                actions are the policy's
  agent kernels the agents behind driver_loop.hpp and the lane-group frame: tests/agent_contract.check_train_invariance with a setup that installs
                the table -- train(3) equals the host trait loop (whose domain_step the first leg has just held to the oracle), the split
                train(1) + train(1) + train(1) and two joined shards, bit for bit

Domain::rollout has no leg here: rsrl_hip_rollout_* start every learner from the domain's default state (models.hpp k_rollout), so no table row reaches them.
No non-finite state goes in, and state_edges.answers() has refused (on the CPU) any row whose fp32 successor is not finite before its wraps."""
import numpy as np
import pytest

import rsrl_amd as ra
from tests import state_edges as se
from tests.edge_helpers import BF16, EG, LAM, SM, TILE, oracle_kwargs
from tests.test_gpu_counter_edges import BY_NAME, case

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MC, CP, AC, CMC = se.MC, se.CP, se.AC, se.CMC
TDAC = 35

# one ctx per family: what selects the kernel family of rsrl_hip_domain_step's ctx (the trait entry points are instantiated per family)
STEP_CTX = {
    "reg": {MC: dict(order=5), CP: dict(order=1), AC: dict(order=1)},
    "generic": {MC: dict(order=6), CP: dict(order=2), AC: dict(order=3)},
    "tile": {d: dict(basis=ra.TILE_CODING, n_tilings=8, tiles_per_dim=6) for d in (MC, CP, AC)},
    "wave": {CP: dict(order=7), AC: dict(order=7)},
    "beta": {CMC: dict(order=3, algo=ra.ILSTD_ACTOR_CRITIC, policy=ra.BETA, gamma=0.95, lr=0.05, alpha=0.3, n_steps=3)},
    "gaussian": {CMC: dict(order=3, algo=TDAC, policy=ra.GAUSSIAN, gamma=0.95, lr=0.01, alpha=0.01)},
}
STEP_PARAMS = [pytest.param(fam, d, id="%s-d%d" % (fam, d)) for fam, per in STEP_CTX.items() for d in per]


def assert_bits(got, want, what):
    got, want = se.bits(got), se.bits(want)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d differ, first at %s" % (what, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("family,domain", STEP_PARAMS)
def test_domain_step_on_the_table(family, domain):
    S, names = se.table(domain)
    n = S.shape[1]
    ad, a64 = se.answers(domain, "f32d"), se.answers(domain, "f64")
    acts = se.actions(domain)
    nxt, rew, term = np.zeros((n, len(acts), S.shape[0]), dtype=F32), np.zeros((n, len(acts)), dtype=F32), np.zeros((n, len(acts)), dtype=bool)
    with ra.Context(domain=domain, n_envs=n, seed=3, **STEP_CTX[family][domain]) as c:
        for j, a in enumerate(acts):
            c.states = S
            frm, nx, r, t = c.domain_step(np.full(n, a, dtype=F32 if domain == CMC else np.int32))
            assert_bits(frm, S, "from, action %r" % (a,))
            assert_bits(c.states, nx, "the ctx's states after the step, action %r" % (a,))
            nxt[:, j], rew[:, j], term[:, j] = nx.T, r, t.astype(bool)
    # bit for bit the device-order oracle
    assert_bits(nxt, ad["next"], "next state against f32d")
    assert_bits(rew, ad["reward"], "reward against f32d")
    assert np.array_equal(term, ad["term"]), names[np.any(term != ad["term"], axis=1)]
    # directly against f64
    e = se.err(domain, nxt, a64["next"]).max(axis=(1, 2))
    print("domain %d %s: device / f64" % (domain, family), ", ".join("%s %.4g (bar %.4g)" % (w, e[m].max(), se.step_bar(domain, w)) for w, m in se.sets(domain)))
    assert np.all(e <= se.row_bars(domain)), names[e > se.row_bars(domain)]
    assert np.array_equal(term, se.predicate(domain, nxt, "f32d"))
    assert_bits(rew, se.reward_of(domain, term), "reward is the constant of term")
    ok = se.decided(domain)
    assert np.array_equal(term[ok], a64["term"][ok]), names[np.any((term != a64["term"]) & ok, axis=1)]


PROJECT = [(MC, o, "reg") for o in (1, 2, 3, 4, 5)] + [(MC, 6, "generic"), (MC, 7, "generic"), (CP, 1, "reg"), (CP, 2, "generic"), (CP, 7, "wave"),
                                                       (AC, 1, "reg"), (AC, 3, "generic"), (AC, 7, "wave")] + [(CMC, o, "cmc") for o in (1, 2, 3, 4, 5)]


@pytest.mark.parametrize("domain,order,family", PROJECT, ids=["d%d-order%d-%s" % p for p in PROJECT])
def test_project_on_the_table(domain, order, family):
    S, names = se.table(domain)
    n = S.shape[1]
    kw = dict(STEP_CTX["beta"][CMC], order=order) if domain == CMC else dict(order=order)
    with ra.Context(domain=domain, n_envs=n, **kw) as c:
        phi = c.project(S)
    want, p64 = se.phi(domain, order, "f32d"), se.phi(domain, order, "f64")
    assert_bits(phi, want, "features against f32d")
    assert np.all(se.bits(phi[-1]) == se.bits(F32(1.0)))
    e = np.abs(phi.astype(F64) - p64).max(axis=0)
    print("domain %d order %d %s: device / f64" % (domain, order, family),
          ", ".join("%s %.4g (bar %.4g)" % (w, e[m].max(), se.phi_bar(domain, order, w)) for w, m in se.sets(domain)))
    assert np.all(e <= se.phi_row_bars(domain, order)), names[e > se.phi_row_bars(domain, order)]


@pytest.mark.parametrize("domain", (MC, CP, AC))
def test_tile_indices_on_the_tile_rows(orc, domain):
    for T, B in se.tile_configs(domain):
        S = se.tile_table(domain, T, B)
        m = S.shape[1]
        with ra.Context(domain=domain, basis=ra.TILE_CODING, n_tilings=T, tiles_per_dim=B, n_envs=m, weight_mode=ra.W_SHARED) as c:      # (a batch may not exceed n_envs)
            got = c.tile_indices(S)
        want = se.tile_numpy(domain, T, B, S)
        assert got.shape == (T, m) and np.array_equal(got, want), (T, B, np.argwhere(got != want)[:5].tolist())
        ag = orc.make_agent(domain=domain, basis=orc.TILE, n_tilings=T, tiles_per_dim=B)
        assert np.array_equal(got[:, ::7], np.stack([orc.tile_indices(ag, S[:, i]) for i in range(0, m, 7)], axis=1))


# ------------------------------------------------------------------------------------------------------------------------------- the driver loops
# (the code copy the row reaches -- the test's name; tests/test_gpu_counter_edges.py's case; steps_per_launch: None the case's own, -1 the default depth with
# RSRL_REG_PRODUCER=0, the fused loop without its producer wave)
LOOPS = [
    ("kernels_reg_fused_pre_mc3", "reg-qlearning-mc3", 0), ("kernels_reg_fused_pre_mc3_depth1", "reg-qlearning-mc3", 1), ("kernels_reg_fused_pre_mc3_depth2", "reg-qlearning-mc3", 2),
    ("kernels_reg_pw_producer_wave_mc5", "reg-sarsa-mc5", 0), ("kernels_reg_fused_pre_mc5_without_the_producer_wave", "reg-sarsa-mc5", -1), ("kernels_reg_fused_ab1", "reg-esarsa-ab1", 0), ("kernels_reg_fused_ab1_depth2", "reg-esarsa-ab1", 2),
    ("kernels_reg_step_lm_quad0", "regstep-lm-sarsa-mc3", None), ("kernels_reg_q4_step_quad1", "regstep-q4-sarsa-mc3", None), ("kernels_reg_step_fm", "regstep-fm-qlearning-mc4", None),
    ("models_generic_fourier_ab2", "generic-sarsa-ab2", 0), ("models_generic_fourier_mc6", "generic-esarsa-mc6", 0), ("models_tile_ab", "tile-sarsa-ab", 0),
    ("kernels_wave_step_uniform_ab7", "wave-sarsa-ab7", 0), ("kernels_wave_ab7_esarsa", "wave-esarsa-ab7", 0), ("kernels_wave_bf16_ab7", "wave-bf16-sarsa-ab7", 0),
    ("kernels_lambda_mc3", "lambda-reg-sarsa-mc3", 0), ("kernels_lambda_mem_ab2", "lambda-mem-q-ab2", 0), ("kernels_lambda_tile_mc", "lambda-tile-sarsa-mc", 0),
    ("kernels_wave_lambda_ab7", "lambda-wave-sarsa-ab7", 0),
    ("kernels_gq_mc3", "gq-reg-mc3", 0), ("kernels_gq_mem_ab2", "gq-mem-ab2", 0), ("kernels_wave_aux_gq_ab7", "gq-wave-ab7", 0),
    ("kernels_td_mc3", "td-reg-mc3", 0), ("kernels_td_mem_mc6", "td-mem-lambda-mc6", 0), ("kernels_td_tile_mc", "td-tile-mc", 0), ("kernels_wave_aux_td_ab7", "td-wave-ab7", 0),
    ("kernels_qsigma_mc3", "qsigma-reg-mc3", 0), ("kernels_qsigma_tile_mc", "qsigma-tile-mc", 0), ("kernels_wave_qsigma_ab7", "qsigma-wave-ab7", 0),
    ("kernels_persist_shared_step_mc3", "shared-dense-step-sarsa-mc3", None), ("kernels_persist_shared_dense_ab1", "shared-dense-persist-qlearning-ab1", None),
    ("kernels_persist_shared_tile_ab", "shared-tile-sarsa-ab", None), ("kernels_sparse_lambda_mc", "sparse-lambda-sarsa-mc", None),
]
# CartPole has no row in that table (it pays 0 until it falls: inside the counter tests' 5-step cap its weights never move; here the forced weights
# and the table's terminal rows move them).  The wave family's CartPole instantiations take the PLAIN Dom::step (kernels_wave.hpp: step_uniform is
# Acrobot's), f32 and bf16; the others are the CartPole copies of the fused register loop, the generic loop, the tile coder and the lambda kernels
CP_CASES = {c["name"]: c for c in [
    case("wave-sarsa-cp7", "k_train_wave", 65, "train_wave", domain=CP, order=7, algo=ra.SARSA, **SM),
    case("wave-bf16-sarsa-cp7", "k_train_wave_pk", 65, "train_wave", domain=CP, order=7, algo=ra.SARSA, **SM, **BF16),
    case("wave-lambda-sarsa-cp7", "k_wave_lambda", 64, "train_wave", domain=CP, order=7, algo=ra.SARSA_LAMBDA, lam=0.9, **EG),
    case("reg-qlearning-cp1", "k_train_reg", 65, "train_dev", domain=CP, order=1, algo=ra.QLEARNING, **EG),
    case("regstep-lm-sarsa-cp1", "k_step_reg_lm", 130, "train_dev", env={"RSRL_K1_QUAD": "0"}, domain=CP, order=1, algo=ra.SARSA, steps_per_launch=1, **EG),
    case("generic-sarsa-cp2", "k_train_mem", 130, domain=CP, order=2, algo=ra.SARSA, **EG),
    case("tile-sarsa-cp", "k_train_mem", 257, domain=CP, algo=ra.SARSA, **TILE, **EG),
    case("lambda-reg-sarsa-cp1", "k_train_lambda", 130, domain=CP, order=1, algo=ra.SARSA_LAMBDA, lam=0.9, **EG),
    case("lambda-mem-q-cp2", "k_train_lambda_mem", 65, domain=CP, order=2, algo=ra.Q_LAMBDA, lam=0.5, trace=ra.TRACE_SATURATE, **EG),
    case("td-reg-cp1", "k_train_td", 130, domain=CP, order=1, algo=ra.TD, policy=ra.RANDOM),
]}
LOOPS += [
    ("kernels_wave_plain_step_cp7", "wave-sarsa-cp7", 0), ("kernels_wave_pk_bf16_plain_step_cp7", "wave-bf16-sarsa-cp7", 0), ("kernels_wave_lambda_plain_step_cp7", "wave-lambda-sarsa-cp7", 0),
    ("kernels_reg_fused_cp1", "reg-qlearning-cp1", 0), ("kernels_reg_fused_cp1_depth2", "reg-qlearning-cp1", 2), ("kernels_reg_step_lm_cp1", "regstep-lm-sarsa-cp1", None),
    ("models_generic_fourier_cp2", "generic-sarsa-cp2", 0), ("models_tile_cp", "tile-sarsa-cp", 0), ("kernels_lambda_cp1", "lambda-reg-sarsa-cp1", 0),
    ("kernels_lambda_mem_cp2", "lambda-mem-q-cp2", 0), ("kernels_td_cp1", "td-reg-cp1", 0),
]
CALLS = (1, 2)
PRED = (ra.TD, ra.TD_LAMBDA)


def bit_differences(c, run, kw, method):
    """what differs between the ctx and the oracle run ON BIT PATTERNS (-0.0 is not 0.0, a NaN equals only the same NaN): states, actions, episode
    counters, weights, traces / fa_td"""
    bad = []
    n, algo = kw["n_envs"], kw.get("algo", 0)

    def same(a, b):
        return a.shape == b.shape and np.array_equal(se.bits(a), se.bits(b))
    if c.step_count != run.t:
        bad.append("step_count %d != %d" % (c.step_count, run.t))
    if not same(c.states.T, run.state):
        bad.append("states")
    if not np.array_equal(c.actions, run.action):
        bad.append("actions (%d of %d)" % (int((c.actions != run.action).sum()), n))
    if not np.array_equal(c.episode_steps, run.ep_step):
        bad.append("episode_steps")
    ow = run.weights
    if kw.get("weight_mode") == ra.W_SHARED:
        w = c.get_weights()
        if not same(w, ow.reshape(w.shape)):
            bad.append("weights")
    else:
        wrong = [i for i in range(n) if not same(c.get_weights(i), ow[i].reshape(c.F, c.n_out))]
        if wrong:
            bad.append("weights of learners %s (%d of %d)" % (wrong[:8], len(wrong), n))
    if method == "train_sparse_lambda":
        wrong = [i for i in range(n) if not same(c.get_traces(i), run.sparse_trace(i))]
        if wrong:
            bad.append("sparse traces of learners %s" % wrong[:8])
    elif algo in LAM or algo == ra.GREEDY_GQ:
        get = c.get_td_weights if algo == ra.GREEDY_GQ else c.get_traces
        wrong = [i for i in range(n) if not same(get(i), run.traces[i].reshape(c.F, c.n_out))]
        if wrong:
            bad.append("traces / fa_td of learners %s (%d of %d)" % (wrong[:8], len(wrong), n))
    if not (np.all(np.isfinite(ow)) and np.abs(ow).max() > 0):
        bad.append("the oracle's weights did not move or are not finite: the case compares nothing")
    return bad


def _install(c_or_run, S, acts, W, device):
    """states, pending actions and (per-learner) weights on a fresh, reset ctx or oracle run"""
    if device:
        c_or_run.states = S
        c_or_run.actions = acts
        if W is not None:
            for i in range(S.shape[1]):
                c_or_run.set_weights(W[i], i)
    else:
        c_or_run.state[:] = S.T
        c_or_run.action[:] = acts
        if W is not None:
            c_or_run.weights[:] = W
        c_or_run.invalidate_q()


@pytest.mark.parametrize("site,case,spl", LOOPS, ids=[l[0] for l in LOOPS])
def test_driver_loop_steps_the_table(orc, monkeypatch, site, case, spl):      # noqa: F811 (the parameter `case` is a row's name here)
    cs = BY_NAME[case] if case in BY_NAME else CP_CASES[case]
    for k, v in cs["env"].items():                   # (the switches are read when the ctx is created)
        monkeypatch.setenv(k, v)
    if spl == -1:                                    # the default depth on the lone fused loop
        monkeypatch.setenv("RSRL_REG_PRODUCER", "0")
        spl = 0
    kw = dict(cs["kw"], max_episode_steps=1000)
    domain, algo = kw.get("domain", MC), kw.get("algo", 0)
    T, _ = se.table(domain)
    rows, A = T.shape[1], len(se.actions(domain))
    shared, pred = kw.get("weight_mode") == ra.W_SHARED, algo in PRED
    if shared:                                       # the Random policy over the table eight times
        kw.update(policy=ra.RANDOM)
        S = np.ascontiguousarray(np.tile(T, (1, 8)))
        row_of = np.tile(np.arange(rows), 8)
    elif pred:                                       # TD / TDLambda take the Random policy: the table A + 1 times, the pending action cycled
        S = np.ascontiguousarray(np.repeat(T, A + 1, axis=1))
        row_of = np.repeat(np.arange(rows), A + 1)
    else:
        kw.update(policy=ra.GREEDY)
        S = np.ascontiguousarray(np.repeat(T, A, axis=1))
        row_of = np.repeat(np.arange(rows), A)
    n = S.shape[1]
    if shared:                                       # (the shared families' rates are per learner count)
        kw["lr"] = cs["kw"]["lr"] * cs["kw"]["n_envs"] / n
    kw["n_envs"] = n
    if spl is not None:
        kw["steps_per_launch"] = spl
    run = orc.Run(orc.make_agent(**oracle_kwargs(orc, kw)), n, "f32d")
    (run.reset_wave if cs["method"] == "train_wave" else run.reset)()
    # the pending action: i % A next to the row's other copies; shared weights: copy k of the table under action k % A (the Random policy draws the rest)
    acts = ((np.arange(n) // rows) % A if shared else np.arange(n) % A).astype(np.int32)
    W = None
    if not shared and not pred:
        W = np.zeros((n, run.F, run.A), dtype=F32)
        if kw.get("basis") == ra.TILE_CODING:        # no constant feature: every cell of tiling 0 carries the preference instead
            W[np.arange(n), : run.F // kw["n_tilings"], acts] = 1.0
        else:
            W[np.arange(n), run.F - 1, acts] = 1.0
    _install(run, S, acts, W, device=False)
    mkw = {"bf16": True} if kw.get("weight_dtype") == ra.W_BF16 else {}
    with ra.Context(**kw) as c:
        c.reset()
        _install(c, S, acts, W, device=True)
        c.timing_enable(True)
        seen = np.zeros((rows, A), dtype=bool)
        for k in CALLS:
            if k == CALLS[0]:
                seen[row_of, run.action] = True     # the pairs the first batch-step steps: the INSTALLED pending actions, so this holds by construction
            getattr(run, cs["method"])(k, **mkw)
            if k == CALLS[0]:
                assert np.all(seen.sum(axis=1) >= min(2, A)) and seen.mean() >= 0.9, (seen.sum(axis=1).min(), seen.mean())
            c.train(k)
            c.sync()
            assert bit_differences(c, run, kw, cs["method"]) == [], "%s (%s) after train(%d)" % (site, case, k)
        kernel = c.timing_read()[2]
        print("%s: %s, %d learners, kernel %s" % (site, case, n, kernel))
        if spl is None or spl == cs["kw"].get("steps_per_launch", 0):
            assert kernel == cs["kernel"], (site, kernel)
    run.close()


# ------------------------------------------------------------------------------------------------------------------------------- the agent kernels
def _agents():
    from tests import (test_gpu_actor_critic as t_ac, test_gpu_cacla as t_cacla, test_gpu_gmc as t_gmc, test_gpu_gtd as t_gtd, test_gpu_lstd as t_lstd,
                       test_gpu_lstd_batch as t_lb, test_gpu_nac_beta as t_nb, test_gpu_nac_gaussian as t_ng, test_gpu_reinforce as t_rf, test_gpu_tdac as t_tdac,
                       test_gpu_tdac_beta as t_tb, test_gpu_tdac_cont as t_tc, test_gpu_tdac_lstd as t_tl)
    from tests.agent_contract import gmc_trait_loop, lstd_batch_trait_loop
    soft = dict(tau=0.7, lr=0.02, alpha=0.2, gamma=0.97)

    def rec(mod):
        def make(**kw):
            mod.Recording.log = []
            return mod.Recording(**dict(mod.BASE, **kw))
        return make
    # name of the code copy: (ctx factory, Context arguments, the step cap, the host trait loop or None for agent_contract's)
    return {
        "kernels_ac_mc3": (t_ac.ctx, dict(domain=MC, order=3, algo=t_ac.AC, **soft), 1000, None),
        "kernels_ac_qac_ab1": (t_ac.ctx, dict(domain=AC, order=1, algo=t_ac.QAC, **soft), 1000, None),
        "kernels_ac_cp1": (t_ac.ctx, dict(domain=CP, order=1, algo=t_ac.AC, **soft), 1000, None),
        "kernels_tdac_mc5": (t_tdac.ctx, dict(domain=MC, order=5, **soft), 1000, None),
        "kernels_tdac_ab1": (t_tdac.ctx, dict(domain=AC, order=1, **soft), 1000, None),
        "kernels_reinforce_cp1": (t_rf.ctx, dict(domain=CP, order=1, algo=ra.REINFORCE, tau=0.7, alpha=0.02, gamma=0.97), 1000, t_rf._host_trait_loop),
        "kernels_reinforce_mc3": (t_rf.ctx, dict(domain=MC, order=3, algo=ra.REINFORCE, tau=0.7, alpha=0.02, gamma=0.97), 1000, t_rf._host_trait_loop),
        "kernels_gtd_gtd2_mc5": (t_gtd.ctx, dict(domain=MC, order=5, algo=ra.GTD2, lr=0.01, lr_td=0.02, gamma=0.97), 1000, None),
        "kernels_gtd_tdc_ab1": (t_gtd.ctx, dict(domain=AC, order=1, algo=ra.TDC, lr=0.01, lr_td=0.02, gamma=0.97), 1000, None),
        "kernels_lstd_recursive_mc3": (t_lstd.ctx, dict(domain=MC, order=3, algo=t_lstd.RLSTD, gamma=0.97, alpha=0.02, n_steps=2), 1000, None),
        "kernels_lstd_ilstd_cp1": (t_lstd.ctx, dict(domain=CP, order=1, algo=t_lstd.ILSTD, gamma=0.97, alpha=0.02, n_steps=2), 1000, None),
        "kernels_tdac_lstd_ab1": (t_tl.ctx, dict(domain=AC, order=1, n_steps=2, **soft), 1000, None),
        "kernels_gmc_cp1": (rec(t_gmc), dict(t_gmc.CASE_B), t_gmc.CASE_B["max_episode_steps"], gmc_trait_loop),
        "kernels_lstd_batch_mc3": (rec(t_lb), dict(domain=MC, order=3, max_episode_steps=7, algo=ra.LSTD), 7, lstd_batch_trait_loop),
        "kernels_lstd_batch_lambda_cp1": (rec(t_lb), dict(domain=CP, order=1, max_episode_steps=40, algo=ra.LSTD_LAMBDA), 40, lstd_batch_trait_loop),
        "kernels_cacla_cmc3": (t_cacla.ctx, dict(order=3, lr=0.02, alpha=0.01, gamma=0.97), 1000, None),
        "kernels_tdac_cont_gaussian_cmc3": (t_tc.ctx, dict(order=3, policy=ra.GAUSSIAN, lr=0.02, alpha=0.01, gamma=0.97), 1000, t_tc.trait_loop),
        "kernels_tdac_cont_beta_cmc5": (t_tc.ctx, dict(order=5, policy=ra.BETA, lr=0.02, alpha=0.01, gamma=0.97), 1000, t_tc.trait_loop),
        "kernels_tdac_beta_cmc3": (t_tb.ctx, dict(order=3, lr=0.02, alpha=0.2, gamma=0.97, n_steps=2), 1000, None),
        "kernels_nac_beta_cmc3": (t_nb.nac_ctx, dict(order=3, n_steps=t_nb.P, lr=0.02, alpha=0.1, gamma=0.97), 1000, t_nb._nac_trait),
        "kernels_nac_gauss_cmc3": (t_ng.ctx, dict(order=3, n_steps=t_ng.P, lr=0.02, alpha=0.1, gamma=0.97), 1000, t_ng._nac_trait),
    }


AGENT_IDS = ["kernels_ac_mc3", "kernels_ac_qac_ab1", "kernels_ac_cp1", "kernels_tdac_mc5", "kernels_tdac_ab1", "kernels_reinforce_cp1", "kernels_reinforce_mc3",
             "kernels_gtd_gtd2_mc5", "kernels_gtd_tdc_ab1", "kernels_lstd_recursive_mc3", "kernels_lstd_ilstd_cp1", "kernels_tdac_lstd_ab1", "kernels_gmc_cp1",
             "kernels_lstd_batch_mc3", "kernels_lstd_batch_lambda_cp1", "kernels_cacla_cmc3", "kernels_tdac_cont_gaussian_cmc3", "kernels_tdac_cont_beta_cmc5",
             "kernels_tdac_beta_cmc3", "kernels_nac_beta_cmc3", "kernels_nac_gauss_cmc3"]


@pytest.mark.parametrize("site", AGENT_IDS)
def test_agent_kernel_steps_the_table(site):
    from tests.agent_contract import check_train_invariance, trait_loop
    make, kw, cap, trait = _agents()[site]
    domain = kw.get("domain", CMC)
    S, _ = se.table(domain)
    n = S.shape[1] - S.shape[1] % 2                  # (the harness joins two shards of n / 2)
    assert n % 64 != 0
    kw = dict(kw, n_envs=n, max_episode_steps=cap)

    def setup(c, off):
        c.reset()
        c.states = S[:, off:off + c.N]

    st, ref = check_train_invariance(make, kw, 3, cap, depths=(1,), first_split=1, setup=setup, trait=trait or trait_loop)
    assert st["env_steps"] == 3 * n
