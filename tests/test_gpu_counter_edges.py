"""The 32-bit edges of the two integers that address every random draw: the batch-step counter t (Philox counter words (uint32_t)t and
(uint32_t)(t >> 32); the per-step streams use t >> 1; graph replays add a device-side counter) and the global learner id env_offset + i
(uint32_t gid, Philox counter word 2).  Every other test starts at t = 0 with ids below 2^21.

The counter: a checkpoint header stores step_count as a little-endian u64 at byte 64 and carries no digest, so a fresh ctx's checkpoint with those
8 bytes rewritten installs any counter (load_weights: c->t = step_count; reset() keeps it and draws the first action at it).  Nothing else is
carried by a fresh ctx, so the oracle needs only Run.t = T0 (pinned on the CPU by tests/test_oracle_counter_cpu.py).  Runs start 5 or 4 steps
below 2^32 and 2^33 (odd and even: the fused loops peel an odd first step and share one Philox block per pair of steps) and cross the edge inside a
fused launch, with one and five steps per launch, between launches (train(3); train(1); train(K - 4)) and -- the launch-bound families -- inside a
replayed step graph (32 steps per graph: train(3); train(33) without statistics; train(2); train(33) for the shared families).  One row per kernel name of kFamily (ctx.hpp) and its
refinements in train_kernel_name() (abi_ctx.hip); the kernel that ran is read back through timing_read().

The learner id: 130 learners whose ids straddle the sign bit inside one wave (env_offset = 2^31 - 65) and end at the largest id check_config admits
(2^32 - 1 - 130), against the oracle built with the same env_offset.

Comparison: bit for bit against the oracle loop that restates the family (states, actions, episode steps, weights, traces / fa_td / epsilons).
Reference-free companion: the same configuration started at T0 + 2^32 (resp. + 2^33) -- every LOW counter word equal -- must not walk the same
actions: that is what a counter truncated to its low word would do.  (T0 - 2^32 is negative for the first edge.)"""
import numpy as np
import pytest

import rsrl_amd as ra
from tests.agent_contract import trait_loop
from tests.edge_helpers import (AB, BF16, E32, E33, EG, LAM, MC, OFFSETS, SHARED, SM, T_ALL, T_TWO, TILE, feats as _feats, install_counter,
                                oracle_kwargs)

pytestmark = pytest.mark.gpu

K = 24
def case(name, kernel, n, method="train", env=None, t0s=T_TWO, fixed_spl=False, graph=False, spls=(0, 1, 5), **kw):
    """one row: Context arguments (lr / alpha scaled like the campaigns: lr |phi|^2 well below 1), the oracle loop that restates the kernel, the
    kernel timing_read() must name; fixed_spl: steps_per_launch is part of what selects the kernel (or the family has one step per launch)"""
    step = 0.2 / _feats(kw)
    shared = kw.get("weight_mode") == ra.W_SHARED
    kw.setdefault("lr", step / n if shared else step)
    if kw.get("algo", 0) in (ra.EXPECTED_SARSA, ra.PAL):
        kw.setdefault("alpha", 0.5)
    elif kw.get("algo", 0) == ra.Q_SIGMA:
        kw.setdefault("alpha", 0.06)
    else:
        kw.setdefault("alpha", step / n if shared else step)
    kw.setdefault("gamma", 0.97)
    return dict(name=name, kernel=kernel, env=env or {}, kw=dict(kw, n_envs=n, seed=1234 + len(name)), method=method, t0s=t0s, fixed_spl=fixed_spl, graph=graph, spls=spls)


CASES = [
    # ---- the one-step agents on the register family's fused loop
    case("reg-qlearning-mc3", "k_train_reg", 257, "train_dev", t0s=T_ALL, domain=MC, order=3, algo=ra.QLEARNING, **EG),
    case("reg-sarsa-mc5", "k_train_reg", 130, "train_dev", t0s=T_ALL, domain=MC, order=5, algo=ra.SARSA, **SM),
    case("reg-sarsa-own-policy-mc1", "k_train_reg", 64, "train_dev", t0s=T_ALL, domain=MC, order=1, algo=ra.SARSA, agent_policy=ra.EPSILON_GREEDY,
         agent_epsilon=0.4, **EG),
    case("reg-esarsa-ab1", "k_train_reg", 65, "train_dev", t0s=T_ALL, domain=AB, order=1, algo=ra.EXPECTED_SARSA, **SM),
    case("reg-pal-mc2", "k_train_reg", 129, "train_dev", t0s=T_ALL, domain=MC, order=2, algo=ra.PAL, **SM),
    case("reg-qlearning-mc4-eps-schedule", "k_train_reg", 100, "train_dev", t0s=T_ALL, domain=MC, order=4, algo=ra.QLEARNING, epsilon_decay=0.9, epsilon_min=0.05,
         spls=(0, 7, 5), **EG),           # (depth 7 for 1: check_config refuses epsilon_decay with steps_per_launch = 1 -- the schedule exists only in the fused loops)
    # ---- the three single-step kernels
    case("regstep-lm-sarsa-mc3", "k_step_reg_lm", 130, "train_dev", env={"RSRL_K1_QUAD": "0"}, fixed_spl=True, graph=True, domain=MC, order=3, algo=ra.SARSA,
         steps_per_launch=1, **EG),
    case("regstep-q4-sarsa-mc3", "k_step_reg_q4", 130, "train_dev", env={"RSRL_K1_QUAD": "1"}, fixed_spl=True, graph=True, domain=MC, order=3, algo=ra.SARSA,
         steps_per_launch=1, **SM),
    case("regstep-fm-qlearning-mc4", "k_step_reg", 257, "train_dev", fixed_spl=True, graph=True, domain=MC, order=4, algo=ra.QLEARNING, steps_per_launch=1, **EG),
    # ---- the generic loop (weights in memory): Fourier orders beyond the register family, tile coding
    case("generic-sarsa-ab2", "k_train_mem", 130, domain=AB, order=2, algo=ra.SARSA, **EG),
    case("generic-esarsa-mc6", "k_train_mem", 65, domain=MC, order=6, algo=ra.EXPECTED_SARSA, **SM),
    case("tile-sarsa-ab", "k_train_mem", 257, domain=AB, algo=ra.SARSA, **TILE, **EG),
    # ---- the wave family (order 7 on a 4-D domain), f32 and bf16: the stochastic-rounding blocks take the whole t
    case("wave-sarsa-ab7", "k_train_wave", 65, "train_wave", t0s=T_ALL, domain=AB, order=7, algo=ra.SARSA, **SM),
    case("wave-esarsa-ab7", "k_train_wave", 64, "train_wave", t0s=T_ALL, domain=AB, order=7, algo=ra.EXPECTED_SARSA, **EG),
    case("wave-bf16-sarsa-ab7", "k_train_wave_pk", 65, "train_wave", t0s=T_ALL, domain=AB, order=7, algo=ra.SARSA, **SM, **BF16),
    case("wave-bf16-esarsa-ab7", "k_train_wave_pk", 64, "train_wave", t0s=T_ALL, domain=AB, order=7, algo=ra.EXPECTED_SARSA, **SM, **BF16),
    # ---- SARSA(lambda) / Q(lambda) on every family they run on
    case("lambda-reg-sarsa-mc3", "k_train_lambda", 130, domain=MC, order=3, algo=ra.SARSA_LAMBDA, lam=0.9, **EG),
    case("lambda-mem-q-ab2", "k_train_lambda_mem", 65, domain=AB, order=2, algo=ra.Q_LAMBDA, lam=0.5, trace=ra.TRACE_SATURATE, **EG),
    case("lambda-tile-sarsa-mc", "k_lambda_tile", 257, domain=MC, algo=ra.SARSA_LAMBDA, lam=0.9, **TILE, **SM),
    case("lambda-wave-sarsa-ab7", "k_wave_lambda", 64, "train_wave", domain=AB, order=7, algo=ra.SARSA_LAMBDA, lam=0.9, **EG),
    case("lambda-wave-bf16-sarsa-ab7", "k_wave_lambda", 65, "train_wave", domain=AB, order=7, algo=ra.SARSA_LAMBDA, lam=0.5, **SM, **BF16),
    # ---- GreedyGQ
    case("gq-reg-mc3", "k_train_gq", 130, domain=MC, order=3, algo=ra.GREEDY_GQ, lr_td=0.002, **EG),
    case("gq-mem-ab2", "k_train_gq_mem", 65, domain=AB, order=2, algo=ra.GREEDY_GQ, lr_td=0.002, **SM),
    case("gq-wave-ab7", "k_wave_aux", 64, "train_wave", domain=AB, order=7, algo=ra.GREEDY_GQ, lr_td=2e-5, **EG),
    case("gq-wave-bf16-ab7", "k_wave_aux", 65, "train_wave", domain=AB, order=7, algo=ra.GREEDY_GQ, lr_td=2e-5, **EG, **BF16),
    # ---- TD / TD(lambda): the Random policy takes a draw every step (TDLambda as in the reference has no step size: low orders, where it stays finite)
    case("td-reg-mc3", "k_train_td", 130, domain=MC, order=3, algo=ra.TD, policy=ra.RANDOM),
    case("td-reg-lambda-mc2", "k_train_td", 65, domain=MC, order=2, algo=ra.TD_LAMBDA, lam=0.5, policy=ra.RANDOM),
    case("td-mem-lambda-mc6", "k_td_mem", 65, domain=MC, order=6, algo=ra.TD_LAMBDA, lam=0.5, policy=ra.RANDOM),
    case("td-tile-mc", "k_td_tile", 257, domain=MC, algo=ra.TD, policy=ra.RANDOM, **TILE),
    case("td-wave-ab7", "k_wave_aux", 64, "train_wave", domain=AB, order=7, algo=ra.TD, policy=ra.RANDOM),
    # ---- QSigma
    case("qsigma-reg-mc3", "k_train_qsigma", 130, domain=MC, order=3, algo=ra.Q_SIGMA, sigma=0.5, n_steps=2, **EG),
    case("qsigma-tile-mc", "k_train_qsigma", 65, domain=MC, algo=ra.Q_SIGMA, sigma=0.5, n_steps=2, **TILE, **EG),
    case("qsigma-wave-ab7", "k_wave_qsigma", 64, "train_wave", domain=AB, order=7, algo=ra.Q_SIGMA, sigma=0.5, n_steps=2, **EG),
    # ---- one shared approximator: dense per step, dense persistent, tile coding (per step only), the sparse-trace lambda agents
    case("shared-dense-step-sarsa-mc3", "k_shared_step", 600, "train_shared_dev", env={"RSRL_NO_PERSIST": "1"}, fixed_spl=True, graph=True, domain=MC, order=3,
         algo=ra.SARSA, **EG, **SHARED),
    case("shared-dense-persist-qlearning-ab1", "k_shared_persist", 130, "train_shared_dev", fixed_spl=True, domain=AB, order=1, algo=ra.QLEARNING, **SM, **SHARED),
    case("shared-tile-sarsa-ab", "k_shared_ca", 257, fixed_spl=True, graph=True, domain=AB, algo=ra.SARSA, **TILE, **EG, **SHARED),
    case("shared-tile-esarsa-mc", "k_shared_ca", 130, fixed_spl=True, graph=True, domain=MC, algo=ra.EXPECTED_SARSA, **TILE, **SM, **SHARED),
    case("sparse-lambda-sarsa-mc", "k_sparse_trace_scatter", 65, "train_sparse_lambda", fixed_spl=True, domain=MC, algo=ra.SARSA_LAMBDA, lam=0.9, **TILE, **EG,
         **SHARED),
    case("sparse-lambda-q-ab", "k_sparse_trace_scatter", 130, "train_sparse_lambda", fixed_spl=True, domain=AB, algo=ra.Q_LAMBDA, lam=0.5, trace=ra.TRACE_SATURATE,
         **TILE, **SM, **SHARED),
]
BY_NAME = {c["name"]: c for c in CASES}
CAP = 5            # the step cap: every learner's episode ends several times inside the window


def oracle_run(orc, cs, kw, t0, calls):
    run = orc.Run(orc.make_agent(**oracle_kwargs(orc, kw)), kw["n_envs"], "f32d")
    run.t = t0
    (run.reset_wave if cs["method"] == "train_wave" else run.reset)()
    mkw = {"bf16": True} if kw.get("weight_dtype") == ra.W_BF16 else {}
    stats = [getattr(run, cs["method"])(k, **mkw) for k in calls]
    assert run.t == t0 + sum(calls)
    return run, stats


def differences(c, run, kw, method):
    """what differs between the ctx and the oracle run, bit for bit"""
    bad = []
    n, algo = kw["n_envs"], kw.get("algo", 0)
    if c.step_count != run.t:
        bad.append(f"step_count {c.step_count} != {run.t}")
    if not np.array_equal(c.states.T, run.state, equal_nan=True):
        bad.append("states")
    if not np.array_equal(c.actions, run.action):
        bad.append(f"actions ({int((c.actions != run.action).sum())} of {n})")
    if not np.array_equal(c.episode_steps, run.ep_step):
        bad.append("episode_steps")
    ow = run.weights
    if kw.get("weight_mode") == ra.W_SHARED:
        w = c.get_weights()
        if not np.array_equal(w, ow.reshape(w.shape), equal_nan=True):
            bad.append("weights")
    else:
        wrong = [i for i in range(n) if not np.array_equal(c.get_weights(i), ow[i].reshape(c.F, c.n_out), equal_nan=True)]
        if wrong:
            bad.append(f"weights of learners {wrong[:8]} ({len(wrong)} of {n})")
    if method == "train_sparse_lambda":
        wrong = [i for i in range(n) if not np.array_equal(c.get_traces(i), run.sparse_trace(i))]
        if wrong:
            bad.append(f"sparse traces of learners {wrong[:8]}")
    elif algo in LAM or algo == ra.GREEDY_GQ:
        get = c.get_td_weights if algo == ra.GREEDY_GQ else c.get_traces
        wrong = [i for i in range(n) if not np.array_equal(get(i), run.traces[i].reshape(c.F, c.n_out), equal_nan=True)]
        if wrong:
            bad.append(f"traces / fa_td of learners {wrong[:8]} ({len(wrong)} of {n})")
    if "epsilon_decay" in kw and not np.array_equal(c.epsilons, run.eps):
        bad.append("epsilons")
    if not (np.all(np.isfinite(ow)) and np.abs(ow).max() > 0):
        bad.append("the oracle's weights did not move or are not finite: the case compares nothing")
    return bad


def _variants(cs):
    own = cs["kw"].get("steps_per_launch", 0)
    if cs["fixed_spl"]:
        v = [(own, [K], True), (own, [3, 1, K - 4], False)]
        if cs["graph"]:
            # one replayed 32-step graph with the edge INSIDE it for every T0 (at step 4 or 5 of the run).  train_now replays a graph when no
            # statistics are asked for and 32 steps or more remain -- the single-step kernels once Q(s,.) is carried (here: from the second call's
            # first step on), the shared families from an odd step of the call on (here: after its first step).  The ABI has no count of replays
            # to assert (timing_read counts a graph as its 32 steps): the cuts are shaped after those conditions instead.
            v.append((own, [2, 33], False) if cs["kw"].get("weight_mode") == ra.W_SHARED else (own, [3, 33], False))
        return v
    a, b, c = cs["spls"]
    return [(a, [K], True), (b, [K], False), (c, [K], False), (a, [3, 1, K - 4], False)]


def _label(t0):
    return ("2p32" if t0 < E33 - 8 else "2p33") + f"m{(E32 if t0 < E33 - 8 else E33) - t0}"


COUNTER_PARAMS = [pytest.param(cs["name"], t0, id=f"{cs['name']}-{cs['kernel']}-t{_label(t0)}") for cs in CASES for t0 in cs["t0s"]]


def _stats_equal(dst, ost):
    return [k for k in ("env_steps", "episodes", "episodes_truncated", "sum_episode_steps") if int(dst[k]) != int(ost[k])]


@pytest.mark.parametrize("name,t0", COUNTER_PARAMS)
def test_counter_crosses_the_edge_bitwise_vs_oracle(orc, monkeypatch, tmp_path, name, t0):
    cs = BY_NAME[name]
    for k, v in cs["env"].items():                   # (the switches are read when the ctx is created)
        monkeypatch.setenv(k, v)
    base = dict(cs["kw"], max_episode_steps=CAP)
    ref_actions = None
    for spl, calls, stats in _variants(cs):
        kw = dict(base, steps_per_launch=spl) if not cs["fixed_spl"] or "steps_per_launch" in base else dict(base)
        what = f"{name} T0 = {t0} steps_per_launch {spl} calls {calls}"
        assert t0 < (E32 if t0 < E33 - 8 else E33) < t0 + sum(calls)
        run, ost = oracle_run(orc, cs, kw, t0, calls)
        with ra.Context(**kw) as c:
            install_counter(c, t0, tmp_path)
            assert np.array_equal(c.actions, _first_actions(orc, cs, kw, t0)), f"{what}: the first action is not drawn at T0"
            c.timing_enable(True)
            dst = [c.train(k, want_stats=stats) for k in calls]
            c.sync()
            kernel = c.timing_read()[2]
            print(f"{what}: kernel {kernel}")
            if spl == cs["kw"].get("steps_per_launch", 0):
                assert kernel == cs["kernel"], what
            bad = differences(c, run, kw, cs["method"])
            if stats:
                bad += [f"stats.{k}" for d, o in zip(dst, ost) for k in _stats_equal(d, o)]
                assert sum(o["episodes"] for o in ost) >= kw["n_envs"], "every learner's episode ends inside the window"
            assert bad == [], what
            if ref_actions is None:
                ref_actions = c.actions.copy()
    # reference-free: the same low counter words under another high word must not give the same actions
    other = t0 + (E32 if t0 < E33 - 8 else E33)
    kw = dict(base)
    with ra.Context(**kw) as c:
        install_counter(c, other, tmp_path)
        first = c.actions.copy()
        c.train(K, want_stats=False)
        assert c.step_count == other + K
        assert not np.array_equal(c.actions, ref_actions), f"{name}: started at {other} the run walks the actions of {t0}: the counter's high word is not used"
        run0 = _first_actions(orc, cs, kw, t0)
        assert not np.array_equal(first, run0), f"{name}: the first action at {other} is the one at {t0}"


def _first_actions(orc, cs, kw, t0):
    run = orc.Run(orc.make_agent(**oracle_kwargs(orc, kw)), kw["n_envs"], "f32d")
    run.t = t0
    (run.reset_wave if cs["method"] == "train_wave" else run.reset)()
    return run.action.copy()


ID_PARAMS = [pytest.param(cs["name"], off, id=f"{cs['name']}-{cs['kernel']}-off{'2p31m65' if off < E32 // 2 else '2p32m131'}") for cs in CASES for off in OFFSETS]


@pytest.mark.parametrize("name,off", ID_PARAMS)
def test_learner_ids_at_the_top_of_the_id_space_bitwise_vs_oracle(orc, monkeypatch, name, off):
    cs = BY_NAME[name]
    for k, v in cs["env"].items():
        monkeypatch.setenv(k, v)
    n = 130
    kw = dict(cs["kw"], n_envs=n, env_offset=off, max_episode_steps=CAP)
    if kw.get("weight_mode") == ra.W_SHARED:          # (the shared families' rates are per learner count)
        kw["lr"] = cs["kw"]["lr"] * cs["kw"]["n_envs"] / n
        kw["alpha"] = cs["kw"]["alpha"] * cs["kw"]["n_envs"] / n if kw.get("algo", 0) in LAM else kw["alpha"]
    assert off < (1 << 31) < off + n or off + n == (1 << 32) - 1
    calls = [3, 1, K - 4]
    run, _ = oracle_run(orc, cs, kw, 0, calls)
    with ra.Context(**kw) as c:
        c.reset()
        c.timing_enable(True)
        for k in calls:
            c.train(k, want_stats=False)
        c.sync()
        assert c.timing_read()[2] == cs["kernel"]
        assert differences(c, run, kw, cs["method"]) == [], f"{name} env_offset {off}"
        mine = c.actions.copy()
    # reference-free: the learners whose ids have bit 31 set are not the learners of the 31-bit images of those ids
    j0 = max(0, (1 << 31) - off)
    with ra.Context(**dict(kw, n_envs=n - j0, env_offset=(off + j0) & 0x7fffffff)) as c:
        c.reset()
        for k in calls:
            c.train(k, want_stats=False)
        assert not np.array_equal(c.actions, mine[j0:])


def test_ids_past_32_bits_are_refused():
    for n, off in ((130, (1 << 32) - 130), (1, (1 << 32) - 1), (64, 1 << 32)):
        with pytest.raises(ra.RsrlHipError, match="global env ids must fit 32 bits") as e:
            ra.Context(n_envs=n, env_offset=off)
        assert e.value.code == -1, (n, off)
    with ra.Context(n_envs=130, env_offset=(1 << 32) - 1 - 130) as c:      # the largest shard check_config admits
        c.reset()
        assert c.train(2)["env_steps"] == 260


# ---- the trait-granular loop: policy_sample() addresses batch-step step_count - 1, handle's inner draw step_count
@pytest.mark.parametrize("t0", T_TWO, ids=_label)
@pytest.mark.parametrize("name,spl", [("regstep-lm-sarsa-mc3", 1), ("tile-sarsa-ab", 0), ("generic-sarsa-ab2", 0)])
def test_trait_loop_crosses_the_edge_bitwise_vs_reference_order_oracle(orc, tmp_path, name, spl, t0):
    # the reference-order loop (orc_run_train: every Q evaluated afresh, as the trait calls do) restates the trait loop of every family
    cs = BY_NAME[name]
    kw = dict(cs["kw"], steps_per_launch=spl, max_episode_steps=CAP)
    run, _ = oracle_run(orc, dict(cs, method="train"), kw, t0, [12])
    with ra.Context(**kw) as c:
        install_counter(c, t0, tmp_path)
        trait_loop(c, 12, CAP)
        assert differences(c, run, kw, "train") == [], f"{name} T0 = {t0}"
        mine = c.actions.copy()
    with ra.Context(**kw) as c:                      # reference-free: the same low counter words under another high word
        install_counter(c, t0 + (E32 if t0 < E33 - 8 else E33), tmp_path)
        trait_loop(c, 12, CAP)
        assert not np.array_equal(c.actions, mine), f"{name}: the trait loop's draws do not use the counter's high word"


# ---- the newer agents: no f32d loop restates them; their own files' f64 numpy loops and bars, at a high counter / at the top of the id space ---------
# (actions exact for the learners outside the near_boundary band, weights at those files' tolerances; launch depths and cuts bit for bit)
WHERE = [pytest.param(t0, 0, id=f"t{_label(t0)}") for t0 in T_TWO] + [pytest.param(0, off, id=f"off{'2p31m65' if off < E32 // 2 else '2p32m131'}") for off in OFFSETS]
ACTORS = {
    # name: (algo, kernel, what the numpy loop returns besides the actions -> the ctx's getters)
    "ac": (ra.ACTOR_CRITIC, "k_train_ac"), "qac": (ra.Q_ACTOR_CRITIC, "k_train_ac"), "tdac": (ra.TD_ACTOR_CRITIC, "k_train_tdac"),
    "reinforce": (ra.REINFORCE, "k_train_reinforce"), "baseline-reinforce": (ra.BASELINE_REINFORCE, "k_train_reinforce"),
}


def _start(c, t0, tmp_path):
    if t0:
        install_counter(c, t0, tmp_path)
    else:
        c.reset()


def _bits(arrays):
    return [np.asarray(a).tobytes() for a in arrays]


@pytest.mark.parametrize("t0,off", WHERE)
@pytest.mark.parametrize("agent", list(ACTORS))
def test_actor_agents_bars_of_their_own_files(orc, tmp_path, agent, t0, off):
    from tests.ac_numpy import ac_restated_loop, near_boundary
    from tests.reinforce_numpy import reinforce_restated_loop
    from tests.tdac_numpy import tdac_restated_loop
    algo, kernel = ACTORS[agent]
    N, cap, seed, gamma, lr, alpha, tau, domain, order = (130 if off else 65), 7, 31, 0.95, 0.05, 0.002, 0.5, MC, 3
    kw = dict(domain=domain, order=order, algo=algo, policy=ra.SOFTMAX, n_envs=N, env_offset=off, seed=seed, gamma=gamma, lr=lr, alpha=alpha, tau=tau,
              max_episode_steps=cap)
    rng = np.random.default_rng(8)
    B = [rng.normal(0.0, 0.5, size=(16, 3)).astype(np.float32) for _ in range(N)] if algo == ra.BASELINE_REINFORCE else None

    def prepare(c):
        _start(c, t0, tmp_path)
        if B is not None:                                              # the baseline never moves: REINFORCE's second approximator is an input
            for i in range(N):
                c.set_weights(B[i], i)

    def snapshot(c):
        out = [c.actions, c.states, c.episode_steps, np.stack([c.get_policy_weights(i) for i in range(N)])]
        if algo != ra.REINFORCE:                                       # (REINFORCE has no value function)
            out.append(np.stack([c.get_weights(i) for i in range(N)]))
        if algo in (ra.REINFORCE, ra.BASELINE_REINFORCE):
            out.append(np.stack([c.get_behaviour_weights(i) for i in range(N)]))
        return out

    with ra.Context(**kw) as c:
        prepare(c)
        S0, A0 = c.states, c.actions
        for i in range(N):                                             # the first action: theta = 0, drawn from BLK_INIT at the installed counter
            x = orc.draw(seed, off + i, t0, orc.BLK_INIT)
            if not near_boundary(np.full(3, 1.0 / 3.0), x):
                assert A0[i] == orc.policy_sample(orc.SOFTMAX, np.zeros(3), x, tau=tau), i
        c.timing_enable(True)
        dev_acts, episodes = [], 0
        for _ in range(K):                                             # one batch-step per call: the same bits as train(K), every action seen
            episodes += c.train(1)["episodes"]
            dev_acts.append(c.actions)
        assert c.timing_read()[2] == kernel and c.step_count == t0 + K
        stepwise = snapshot(c)
        if algo in (ra.ACTOR_CRITIC, ra.Q_ACTOR_CRITIC):
            acts, Ws, Ts, near = ac_restated_loop(orc, algo == ra.Q_ACTOR_CRITIC, domain, order, N, K, cap, seed, gamma, lr, alpha, tau, S0, A0, t0=t0, env_offset=off)
            pairs = lambda i: ((c.get_weights(i), Ws[i]), (c.get_policy_weights(i), Ts[i]))                     # noqa: E731
        elif algo == ra.TD_ACTOR_CRITIC:
            acts, ws, Ts, near = tdac_restated_loop(orc, domain, order, N, K, cap, seed, gamma, lr, alpha, tau, S0, A0, t0=t0, env_offset=off)
            pairs = lambda i: ((c.get_weights(i)[:, 0], ws[i]), (c.get_policy_weights(i), Ts[i]))               # noqa: E731
        else:
            acts, Ts, Tbs, near = reinforce_restated_loop(orc, domain, order, N, K, cap, seed, gamma, alpha, tau, S0, A0,
                                                          None if B is None else [b.astype(np.float64) for b in B], t0=t0, env_offset=off)
            pairs = lambda i: ((c.get_policy_weights(i), Ts[i]), (c.get_behaviour_weights(i), Tbs[i]))          # noqa: E731
        same = (np.array(dev_acts) == acts).all(axis=0)                # an fp32 rounding may flip a softmax draw: that learner leaves the comparison
        print(f"{agent} t0 {t0} off {off}: same {same.mean():.3f} compared {(same & ~near).mean():.3f}")
        assert same.mean() >= 0.9, same
        assert (same & ~near).mean() >= 0.75                           # (at least 3/4 of the learners compared)
        for i in np.flatnonzero(same & ~near):
            for got, want in pairs(i):
                assert np.max(np.abs(got - want)) <= 3e-6 * (1 + np.max(np.abs(want))) * K * 16, i
        assert episodes >= N
    # the edge inside a fused launch, with five steps per launch and between launches: bit for bit the stepwise run
    for spl, calls in ((0, [K]), (5, [K]), (0, [3, 1, K - 4])):
        with ra.Context(steps_per_launch=spl, **kw) as c:
            prepare(c)
            for k in calls:
                c.train(k, want_stats=False)
            assert _bits(snapshot(c)) == _bits(stepwise), (spl, calls)
    if t0:
        with ra.Context(**kw) as c:
            install_counter(c, t0 + (E32 if t0 < E33 - 8 else E33), tmp_path)
            if B is not None:
                for i in range(N):
                    c.set_weights(B[i], i)
            c.train(K, want_stats=False)
            assert not np.array_equal(c.actions, stepwise[0])


@pytest.mark.parametrize("t0,off", WHERE)
def test_hiv_bars_of_its_own_file(orc, tmp_path, t0, off):
    from tests import hiv_numpy as hv
    N, cap, seed, lr, gamma = (130 if off else 65), 7, 21, 0.01, 0.9
    lo, hi = [-5.0] * 6, [8.0] * 6
    kw = dict(domain=ra.HIV_TREATMENT, order=1, algo=ra.QLEARNING, policy=ra.RANDOM, n_envs=N, env_offset=off, max_episode_steps=cap, seed=seed, lr=lr, gamma=gamma)
    snaps = []
    for spl, calls in ((0, [K]), (1, [K]), (5, [3, 1, K - 4])):
        with ra.Context(steps_per_launch=spl, **kw) as c:
            _start(c, t0, tmp_path)
            first = c.actions
            c.timing_enable(True)
            st = [c.train(k) for k in calls]
            assert c.timing_read()[2] == "k_hiv_train"
            if not snaps:
                _, a, y, obs32, ep, W, n_trunc = ref = hv.q_learning_random_loop(orc, lo, hi, 1, c.F, N, K, cap, seed, lr, gamma, t0=t0, env_offset=off)
                assert np.array_equal(first, ref[0])
                assert np.array_equal(c.actions, a)
                assert hv.bits_equal(c.get_hidden_states(), y)
                u = np.abs(c.states.view(np.int32).astype(np.int64) - obs32.view(np.int32).astype(np.int64))
                assert np.all(u <= 1)
                assert np.array_equal(c.episode_steps, ep)
                for i in range(N):
                    assert np.allclose(c.get_weights(i), W[i], atol=2e-5, rtol=1e-4), i
                assert sum(s["episodes"] for s in st) == n_trunc >= N
            snaps.append(_bits([np.stack([c.get_weights(i) for i in range(N)]), c.states, c.get_hidden_states(), c.actions, c.episode_steps]))
            acts = c.actions
    assert snaps[1] == snaps[0] and snaps[2] == snaps[0]
    if t0:
        with ra.Context(**kw) as c:
            install_counter(c, t0 + (E32 if t0 < E33 - 8 else E33), tmp_path)
            c.train(K, want_stats=False)
            assert not np.array_equal(c.actions, acts)


@pytest.mark.parametrize("t0,off", WHERE)
@pytest.mark.parametrize("algo", [ra.RECURSIVE_LSTD, ra.ILSTD], ids=["rlstd", "ilstd"])
def test_lstd_trait_loop_and_train(orc, tmp_path, algo, t0, off):
    # the Random policy's action IS the draw: every step's actions exact; the f64 state against the numpy replay of the recorded transitions at the
    # bound of test_gpu_lstd.py's replay (1e4 F K eps, relative); train() at every launch depth bit for bit the trait loop
    from tests.lstd_numpy import random_policy_actions, replay_trait_loop
    N, cap, seed, gamma, alpha, n_upd, domain, order = (130 if off else 65), 7, 9, 0.97, 0.02, 2, MC, 3
    kw = dict(domain=domain, order=order, algo=algo, policy=ra.RANDOM, n_envs=N, env_offset=off, seed=seed, gamma=gamma, alpha=alpha, n_steps=n_upd, max_episode_steps=cap)

    def state_of(c):
        out = [c.states, c.actions, c.episode_steps]
        for i in range(N):
            out += [x for x in c.get_lstd_state(i) if x is not None]
        return _bits(out)

    with ra.Context(**kw) as c:
        _start(c, t0, tmp_path)
        assert np.array_equal(c.actions, random_policy_actions(orc, seed, 3, N, t0, orc.BLK_INIT, off))
        ep, rec = np.zeros(N, dtype=np.int64), []
        for k in range(K):
            a = c.actions
            frm, nxt, rew, term = c.domain_step(a)
            c.handle(frm, a, rew, nxt, term)
            rec.append((frm.copy(), nxt.copy(), rew.copy(), term.copy()))
            ep += 1
            mask = (term.astype(bool) | (ep >= cap)).astype(np.uint8)
            c.domain_reset(mask)
            ep[mask == 1] = 0
            got = c.policy_sample()
            assert c.step_count == t0 + k + 1
            assert np.array_equal(got, random_policy_actions(orc, seed, 3, N, t0 + k, orc.BLK_STEP, off)), k      # (RESET is an alias of STEP)
        c.episode_steps = ep.astype(np.uint32)
        F = c.F
        tol = 1e4 * F * K * np.finfo(np.float64).eps
        for i in range(0, N, 8):
            want = replay_trait_loop(orc, algo == ra.RECURSIVE_LSTD, domain, order, F, [(f[:, i], n[:, i], r[i], t[i]) for f, n, r, t in rec], gamma, alpha, n_upd)
            got = c.get_lstd_state(i)
            for g, w in list(zip(got, want))[: 2 if algo == ra.RECURSIVE_LSTD else 3]:
                assert np.max(np.abs(g - w)) <= tol * (1.0 + np.max(np.abs(w))), i
            assert np.abs(want[0]).max() > 0
        trait = state_of(c)
    for spl, calls in ((0, [K]), (1, [K]), (5, [3, 1, K - 4])):
        with ra.Context(steps_per_launch=spl, **kw) as c:
            _start(c, t0, tmp_path)
            c.timing_enable(True)
            for k in calls:
                c.train(k, want_stats=False)
            assert c.timing_read()[2] == "k_train_lstd"
            assert state_of(c) == trait, (spl, calls)
