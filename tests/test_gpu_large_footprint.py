"""Per-learner arrays past 2^31 bytes, 2^32 bytes and (two rows) 2^31 elements: the device runs the full size, the oracle replays slices of 8
learners through env_offset, bit for bit -- states, actions, episode steps, the sampled learners' weights and traces / fa_td.  Per-learner weights
make the learners independent and the draws are keyed by the global learner id, so a slice is a complete reference (the style of
test_c2_full_size_sampled_learners_bitwise_vs_oracle; every other test stays below 1.6 GB).

K = 6 batch-steps cut as train(4); train(2) with max_episode_steps = 3 (every learner restarts inside the run).  The sampled learners start from
DISTINCT random weights (set_weights before reset; the oracle slice starts from the same): a store that lands on another learner, or a load that
reads zeros from an out-of-range descriptor, changes a compared bit.

Which learners: learner-major layouts with b bytes per learner -- learner 0, N - 1 and, for each edge E in {2^31 B, 2^32 B, 2^31 elements where the
array reaches it}, floor(E / b) - 1, floor(E / b), floor(E / b) + 1.  SoA layouts (f32[A][F][N]: every learner touches the high rows) -- learner 0,
N - 1, one interior 256-learner block boundary, and an assert that some row starts beyond each edge.  N lies 3 % past the edge plus 3: the last
wave / lane group is ragged.  The kernel that ran is read back through timing_read() and is part of the test id.

Also at these sizes: checksum() equal between steps_per_launch 0 and 1; the all-learners form of set_weights read back at the sampled learners;
rollout_greedy's n_states of the sampled slices; a save_weights / load_weights round trip (wave f32 row, 4.4 GB through tmp_path).

One large ctx is alive at a time (the largest, BaselineREINFORCE's three f32[A][F][N] arrays, holds 13.3 GB: inside the 14 GB this module allows itself).  A case whose Context(...) fails with RSRL_HIP_ENOMEM skips with its size in the message, and the
module's last test asserts that at most one case skipped that way.

The newer agents (AC / TDAC / REINFORCE, LSTD, HIV) have no oracle loop and their numpy loops start from zero weights: their rows compare 64-learner
slices of the full-size run are compared with the f64 numpy loops of their own test files, started from the slices' pre-set state, at those files' bars
-- and, as an addition, bit for bit with 64-learner ctxs at the same env_offset.  The trait-granular fast path runs the trait loop with device pointers
at 3.2 and 4.4 GB against the oracle's reference-order loop; the sparse-trace lambda agents' value lists pass 2^32 bytes at 2 160 069 learners, all of
which the oracle replays."""
import os
import shutil

import numpy as np
import pytest

import rsrl_amd as ra
from tests.edge_helpers import AB, BF16, CP, EG, MC, SM, TILE, feats, oracle_kwargs

pytestmark = pytest.mark.gpu

ENOMEM = -3
E31, E32 = 1 << 31, 1 << 32
M = 8                      # learners per oracle slice
CUT = (4, 2)
CAP = 3
SKIPPED_FOR_MEMORY = []


def row(name, kernel, n, method, learner_major, env=None, spl=(0,), extras=(), **kw):
    step = 0.2 / feats(kw)
    kw.setdefault("lr", step)
    kw.setdefault("alpha", 0.5 if kw["algo"] in (ra.EXPECTED_SARSA, ra.PAL) else (0.06 if kw["algo"] == ra.Q_SIGMA else step))
    kw.setdefault("gamma", 0.97)
    return dict(name=name, kernel=kernel, n=n, method=method, learner_major=learner_major, env=env or {}, spl=spl, extras=extras,
                kw=dict(kw, seed=77 + len(name), max_episode_steps=CAP))


ROWS = [
    # ---- the wave family: learner-major, 49 152 B (f32) / 24 576 B (bf16) per Acrobot learner, 32 768 B per CartPole learner
    row("wave-f32-esarsa-ab7", "k_train_wave", 90005, "train_wave", True, spl=(0, 1), extras=("set_all",), domain=AB, order=7, algo=ra.EXPECTED_SARSA, **SM),
    row("wave-bf16-esarsa-ab7", "k_train_wave_pk", 180008, "train_wave", True, spl=(0, 1), domain=AB, order=7, algo=ra.EXPECTED_SARSA, **SM, **BF16),
    row("wave-lambda-sarsa-ab7", "k_wave_lambda", 90005, "train_wave", True, domain=AB, order=7, algo=ra.SARSA_LAMBDA, lam=0.9, **EG),
    row("wave-aux-gq-cp7", "k_wave_aux", 135007, "train_wave", True, domain=CP, order=7, algo=ra.GREEDY_GQ, lr_td=2e-5, **EG),
    row("wave-qsigma-ab7", "k_wave_qsigma", 90005, "train_wave", True, domain=AB, order=7, algo=ra.Q_SIGMA, sigma=0.5, n_steps=2, **EG),
    # ---- tile coding with per-learner tables: 8 tilings x 6^4 tiles x 2 actions = 82 944 B per CartPole learner (TD: one column, 41 472 B)
    row("tile-sarsa-cp", "k_train_mem", 53337, "train", True, spl=(0, 1), domain=CP, algo=ra.SARSA, **TILE, **EG),
    row("tile-lambda-sarsa-cp", "k_lambda_tile", 53337, "train", True, domain=CP, algo=ra.SARSA_LAMBDA, lam=0.9, **TILE, **EG),
    row("tile-td-cp", "k_td_tile", 106673, "train", True, domain=CP, algo=ra.TD, policy=ra.RANDOM, **TILE),
    # ---- the generic Fourier orders: SoA, CartPole Fourier(4), 5 000 B per learner (TD: 2 500 B)
    row("generic-sarsa-cp4", "k_train_mem", 884766, "train", False, spl=(0, 1), extras=("rollout",), domain=CP, order=4, algo=ra.SARSA, **EG),
    row("generic-lambda-q-cp4", "k_train_lambda_mem", 884766, "train", False, domain=CP, order=4, algo=ra.Q_LAMBDA, lam=0.5, **EG),
    row("generic-gq-cp4", "k_train_gq_mem", 884766, "train", False, domain=CP, order=4, algo=ra.GREEDY_GQ, lr_td=1e-4, **SM),
    row("generic-td-cp4", "k_td_mem", 1769532, "train", False, domain=CP, order=4, algo=ra.TD, policy=ra.RANDOM),
    row("generic-qsigma-cp4", "k_train_qsigma", 884766, "train", False, domain=CP, order=4, algo=ra.Q_SIGMA, sigma=0.5, n_steps=2, **EG),
    # ---- the register family: MountainCar Fourier(5), 432 B per learner; fused, and one step per launch on a W too large for the single-step kernels
    row("reg-fused-sarsa-mc5", "k_train_reg", 10240318, "train_dev", False, spl=(0, 1), extras=("set_all", "rollout"), domain=MC, order=5, algo=ra.SARSA, **EG),
    # ---- the single-step kernels between 2^31 and 2^32 bytes: learner-major W (four lanes per learner / one), and k_step_reg's one descriptor (F = 25)
    row("regstep-q4-sarsa-mc5", "k_step_reg_q4", 7500003, "train_dev", True, env={"RSRL_K1_QUAD": "1"}, domain=MC, order=5, algo=ra.SARSA, steps_per_launch=1, **EG),
    row("regstep-lm-qlearning-mc5", "k_step_reg_lm", 7500003, "train_dev", True, env={"RSRL_K1_QUAD": "0"}, domain=MC, order=5, algo=ra.QLEARNING, steps_per_launch=1, **SM),
    row("regstep-fm-esarsa-mc4", "k_step_reg", 10000003, "train_dev", False, domain=MC, order=4, algo=ra.EXPECTED_SARSA, steps_per_launch=1, **EG),
    # ---- past 2^31 ELEMENTS (8.6 GB of f32)
    row("wave-f32-sarsa-ab7-2p31-elements", "k_train_wave", 180008, "train_wave", True, domain=AB, order=7, algo=ra.SARSA, **SM),
    row("reg-fused-qlearning-mc5-2p31-elements", "k_train_reg", 20480003, "train_dev", False, domain=MC, order=5, algo=ra.QLEARNING, **EG),
]


def sampled_slices(r, F, n_out):
    """-> (offsets of the M-learner slices, the picked learners, what the choice rests on)"""
    n = r["n"]
    esz = 2 if r["kw"].get("weight_dtype") == ra.W_BF16 else 4
    b = F * n_out * esz                                   # bytes per learner of W (the auxiliary matrix has the same shape, f32)
    total = b * n
    edges = [e for e in (E31, E32, E31 * esz) if e < total]
    assert edges and total > E31, (r["name"], total)
    if r["learner_major"]:
        picks = [0, n - 1] + [e // b + d for e in edges for d in (-1, 0, 1)]
        assert all(0 <= p < n for p in picks) and n - 1 > max(picks[2:]) + 64, picks
    else:
        rows_ = F * n_out
        for e in edges:                                   # SoA: row k of f32[A][F][N] starts at byte k * N * 4
            assert (rows_ - 1) * n * 4 > e, (r["name"], e)
        picks = [0, n - 1, (n // 2) // 256 * 256]
    centres = [0, n - 1] + ([e // b for e in edges] if r["learner_major"] else picks[2:])           # one slice around each edge's three learners
    offs = sorted({min(max(p - 4, 0), n - M) for p in centres})
    assert all(b_ - a_ >= M for a_, b_ in zip(offs, offs[1:])) and all(any(o <= p < o + M for o in offs) for p in picks), (offs, picks)
    return offs, sorted(set(picks)), dict(bytes_per_learner=b, total_bytes=total, edges=edges)


def _weights_for(rng, shape, bf16):
    w = (rng.normal(size=shape) * (0.5 / np.sqrt(shape[0]))).astype(np.float32)
    if bf16:
        w = (w.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)      # bf16-representable: stored exactly
    return w


def _open(r, kw):
    try:
        return ra.Context(**kw)
    except ra.RsrlHipError as e:
        if e.code == ENOMEM:
            SKIPPED_FOR_MEMORY.append(r["name"])
            pytest.skip(f"{r['name']}: no device memory for {r['n']} learners ({e})")
        raise


def _oracle_slice(orc, r, kw, off, W0):
    okw = oracle_kwargs(orc, dict(kw, n_envs=M))
    okw["env_offset"] = off
    run = orc.Run(orc.make_agent(**okw), M, "f32d")
    run.weights[:] = W0.reshape(run.weights.shape)
    (run.reset_wave if r["method"] == "train_wave" else run.reset)()
    mkw = {"bf16": True} if kw.get("weight_dtype") == ra.W_BF16 else {}
    for k in CUT:
        getattr(run, r["method"])(k, **mkw)
    return run


PARAMS = [pytest.param(r, id=f"{r['name']}-N{r['n']}-{r['kernel']}") for r in ROWS]


@pytest.mark.parametrize("r", PARAMS)
def test_large_footprint_sampled_learners_bitwise_vs_oracle(orc, monkeypatch, tmp_path, r):
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    n, algo = r["n"], r["kw"]["algo"]
    bf16 = r["kw"].get("weight_dtype") == ra.W_BF16
    rng = np.random.default_rng(len(r["name"]))
    sums = []
    for spl in r["spl"]:
        kw = dict(r["kw"], n_envs=n)
        if "steps_per_launch" not in kw:
            kw["steps_per_launch"] = spl
        with _open(r, kw) as c:
            F, n_out = c.F, c.n_out
            offs, picks, info = sampled_slices(r, F, n_out)
            if spl == r["spl"][0]:
                print(f"{r['name']}: N {n} F {F} x {n_out}, {info['bytes_per_learner']} B / learner, {info['total_bytes'] / 1e9:.2f} GB, edges {info['edges']}, "
                      f"slices at {offs}")
                W0 = {off: np.stack([_weights_for(rng, (F, n_out), bf16) for _ in range(M)]) for off in offs}
            if "set_all" in r["extras"] and spl == r["spl"][0]:
                # the all-learners form of set_weights: one matrix to every learner, read back where the indices are large
                w_all = _weights_for(rng, (F, n_out), bf16)
                c.set_weights_all(w_all)
                for p in picks:
                    assert np.array_equal(c.get_weights(p), w_all), p
            for off in offs:
                for j in range(M):
                    c.set_weights(W0[off][j], off + j)
            for off in offs:                               # (read back before anything runs: the accessors' own index arithmetic)
                for j in (0, M - 1):
                    assert np.array_equal(c.get_weights(off + j), W0[off][j]), (off, j)
            if "set_all" in r["extras"] and spl == r["spl"][0]:
                c.set_weights_all(np.zeros((F, n_out), dtype=np.float32))          # the unsampled learners start from zero, like the oracle's
                for off in offs:
                    for j in range(M):
                        c.set_weights(W0[off][j], off + j)
            c.reset()
            c.timing_enable(True)
            st = c.train(CUT[0])
            c.train(CUT[1], want_stats=False)
            kernel = c.timing_read()[2]
            assert kernel == r["kernel"], (r["name"], spl, kernel)
            assert st["env_steps"] == n * CUT[0] and st["episodes"] >= n
            sums.append(c.checksum())
            if spl != r["spl"][0]:
                continue                                   # (the second launch depth: its checksum is the comparison)
            S, A_, EP = c.states, c.actions, c.episode_steps
            n_dev = c.rollout_greedy(40)[0] if "rollout" in r["extras"] else None
            for off in offs:
                run = _oracle_slice(orc, r, kw, off, W0[off])
                what = f"{r['name']} learners {off}..{off + M - 1}"
                assert np.array_equal(S[:, off:off + M].T, run.state, equal_nan=True), what + ": states"
                assert np.array_equal(A_[off:off + M], run.action), what + ": actions"
                assert np.array_equal(EP[off:off + M], run.ep_step), what + ": episode steps"
                ow = run.weights
                assert np.all(np.isfinite(ow)) and not np.array_equal(ow.reshape(W0[off].shape), W0[off]), what + ": the oracle's weights did not move"
                for j in range(M):
                    assert np.array_equal(c.get_weights(off + j), ow[j].reshape(F, n_out)), f"{what}: weights of learner {off + j}"
                    if algo in (ra.SARSA_LAMBDA, ra.Q_LAMBDA, ra.TD_LAMBDA):
                        assert np.array_equal(c.get_traces(off + j), run.traces[j].reshape(F, n_out)), f"{what}: traces of learner {off + j}"
                    elif algo == ra.GREEDY_GQ:
                        assert np.array_equal(c.get_td_weights(off + j), run.traces[j].reshape(F, n_out)), f"{what}: fa_td of learner {off + j}"
                if n_dev is not None:
                    assert np.array_equal(n_dev[off:off + M], run.rollout_greedy(40)[0]), what + ": rollout_greedy"
    assert all(s == sums[0] for s in sums), (r["name"], "checksum differs between launch depths", sums)


def test_large_checkpoint_round_trip_wave_f32(tmp_path):
    # save_weights / load_weights walk the arrays with their own index arithmetic: 4.4 GB through a file
    r = ROWS[0]
    if shutil.disk_usage(str(tmp_path)).free < (6 << 30):
        pytest.skip(f"the temp directory has less than 6 GB free: no {r['n']}-learner checkpoint round trip")
    rng = np.random.default_rng(5)
    path = os.path.join(str(tmp_path), "large.ckpt")
    try:
        with _open(r, dict(r["kw"], n_envs=r["n"])) as c:
            offs, picks, _ = sampled_slices(r, c.F, c.n_out)
            W0 = {p: _weights_for(rng, (c.F, c.n_out), False) for p in picks}
            for p, w in W0.items():
                c.set_weights(w, p)
            c.reset()
            c.train(3, want_stats=False)
            keep = {p: c.get_weights(p) for p in picks}
            assert all(not np.array_equal(keep[p], W0[p]) for p in picks)
            before, t = c.checksum(), c.step_count
            c.save_weights(path)
            assert os.path.getsize(path) > E32
            c.set_weights_all(np.zeros((c.F, c.n_out), dtype=np.float32))
            assert c.checksum()[0] != before[0]
            c.load_weights(path)
            assert c.step_count == t and c.checksum()[0] == before[0]
            for p in picks:
                assert np.array_equal(c.get_weights(p), keep[p]), p
    finally:
        if os.path.exists(path):
            os.remove(path)


# ---- the newer agents at these sizes: no oracle loop restates them and their numpy loops start from zero weights, so the reference is the DEVICE
# itself at a size where every offset is small -- a 64-learner ctx at env_offset = off, given the same distinct random state, must be the slice
# off .. off + 63 of the full-size run bit for bit (sharding invariance, which their own files assert at 64 learners and compare with numpy there).
MS = 64
AGENT_ROWS = [
    # name, kernel, N, bytes per learner of the largest array, learner-major, Context arguments
    ("ac-mc5", "k_train_ac", 10240318, 432, False, dict(domain=MC, order=5, algo=ra.ACTOR_CRITIC, policy=ra.SOFTMAX, lr=0.05, alpha=0.002, tau=0.5)),
    ("tdac-mc5", "k_train_tdac", 10240318, 432, False, dict(domain=MC, order=5, algo=ra.TD_ACTOR_CRITIC, policy=ra.SOFTMAX, lr=0.05, alpha=0.002, tau=0.5)),
    ("reinforce-mc5", "k_train_reinforce", 10240318, 432, False, dict(domain=MC, order=5, algo=ra.REINFORCE, policy=ra.SOFTMAX, alpha=0.002, tau=0.5)),
    ("baseline-reinforce-mc5", "k_train_reinforce", 10240318, 432, False, dict(domain=MC, order=5, algo=ra.BASELINE_REINFORCE, policy=ra.SOFTMAX, alpha=0.002, tau=0.5)),
    ("rlstd-mc5", "k_train_lstd", 426682, 10368, True, dict(domain=MC, order=5, algo=ra.RECURSIVE_LSTD, policy=ra.RANDOM, alpha=0.02, n_steps=2)),
    ("ilstd-mc5", "k_train_lstd", 426682, 10368, True, dict(domain=MC, order=5, algo=ra.ILSTD, policy=ra.RANDOM, alpha=0.02, n_steps=2)),
    ("hiv-qlearning-o2", "k_hiv_train", 379273, 11664, True, dict(domain=ra.HIV_TREATMENT, order=2, algo=ra.QLEARNING, policy=ra.RANDOM, lr=1e-3)),
]


def _agent_state(c, i):
    """every per-learner array the agent has, through its getters"""
    algo, out = c.cfg.algo, []
    if algo in (ra.RECURSIVE_LSTD, ra.ILSTD):
        return [x for x in c.get_lstd_state(i) if x is not None]
    if algo != ra.REINFORCE:
        out.append(c.get_weights(i))
    if algo in (ra.ACTOR_CRITIC, ra.TD_ACTOR_CRITIC, ra.REINFORCE, ra.BASELINE_REINFORCE):
        out.append(c.get_policy_weights(i))
    if algo in (ra.REINFORCE, ra.BASELINE_REINFORCE):
        out.append(c.get_behaviour_weights(i))
    return out


def _install(c, i, st):
    algo = c.cfg.algo
    if algo in (ra.RECURSIVE_LSTD, ra.ILSTD):
        c.set_lstd_state(st["theta"], st["mat"], st["mu"] if algo == ra.ILSTD else None, i)
        return
    if algo != ra.REINFORCE:
        c.set_weights(st["W"][:, :c.n_out], i)
    if algo in (ra.ACTOR_CRITIC, ra.TD_ACTOR_CRITIC, ra.REINFORCE, ra.BASELINE_REINFORCE):
        c.set_policy_weights(st["Th"], i)
    if algo in (ra.REINFORCE, ra.BASELINE_REINFORCE):
        c.set_behaviour_weights(st["Th"], i)                 # the open episode is sampled from the theta it began with


def _random_state(rng, F, A, rlstd):
    Mx = rng.normal(0.0, 1.0, size=(F, F))
    mat = 1e-3 * (np.eye(F) + (Mx + Mx.T) / (4.0 * F)) if rlstd else np.eye(F) + 0.1 * Mx / np.sqrt(F)      # (well conditioned: test_gpu_lstd.py's randomise)
    return dict(W=(rng.normal(size=(F, A)) * 0.5 / np.sqrt(F)).astype(np.float32), Th=(rng.normal(size=(F, A)) * 0.5 / np.sqrt(F)).astype(np.float32),
                theta=rng.normal(0.0, 0.5, size=F), mat=mat, mu=rng.normal(0.0, 1.0, size=F))


@pytest.mark.parametrize("name,kernel,n,b,learner_major,kw", [pytest.param(*r, id=f"{r[0]}-N{r[2]}-{r[1]}") for r in AGENT_ROWS])
def test_large_footprint_newer_agents_slices_equal_small_shards(name, kernel, n, b, learner_major, kw):
    kw = dict(kw, seed=91, gamma=0.95, max_episode_steps=CAP)
    total = b * n
    assert total > E32
    offs = _slices_of(n, b, learner_major)
    if not learner_major:
        rows_ = total // (n * 4)
        assert (rows_ - 1) * n * 4 > E32                      # SoA: the last rows of f32[A][F][N] start beyond 2^32 bytes
    rng = np.random.default_rng(len(name))
    r = dict(name=name, n=n)
    with _open(r, dict(kw, n_envs=n)) as c:
        F, A = c.F, c.A
        states = {off: [_random_state(rng, F, A, kw["algo"] == ra.RECURSIVE_LSTD) for _ in range(MS)] for off in offs}
        print(f"{name}: N {n} F {F}, {b} B / learner in the largest array ({total / 1e9:.2f} GB), slices at {offs}")
        for off in offs:
            for j in range(MS):
                _install(c, off + j, states[off][j])
        c.reset()
        c.timing_enable(True)
        st = c.train(CUT[0])
        c.train(CUT[1], want_stats=False)
        assert c.timing_read()[2] == kernel
        assert st["env_steps"] == n * CUT[0] and st["episodes"] >= n
        S, A_, EP = c.states, c.actions, c.episode_steps
        Y = c.get_hidden_states() if kw["domain"] == ra.HIV_TREATMENT else None
        full = {off: [_agent_state(c, off + j) for j in range(MS)] for off in offs}
        before = {off: _agent_state(c, off) for off in offs}
    for off in offs:
        with ra.Context(**dict(kw, n_envs=MS, env_offset=off)) as s:
            for j in range(MS):
                _install(s, j, states[off][j])
            start = _agent_state(s, 0)
            s.reset()
            s.train(CUT[0])
            s.train(CUT[1], want_stats=False)
            what = f"{name} learners {off}..{off + MS - 1}"
            assert S[:, off:off + MS].tobytes() == s.states.tobytes(), what + ": states"
            assert np.array_equal(A_[off:off + MS], s.actions), what + ": actions"
            assert np.array_equal(EP[off:off + MS], s.episode_steps), what + ": episode steps"
            if Y is not None:
                assert np.ascontiguousarray(Y[:, off:off + MS]).tobytes() == s.get_hidden_states().tobytes(), what + ": hidden states"
            for j in range(MS):
                got, want = full[off][j], _agent_state(s, j)
                assert [x.tobytes() for x in got] == [x.tobytes() for x in want], f"{what}: learner {off + j}"
            assert any(x.tobytes() != y.tobytes() for x, y in zip(before[off], start)), what + ": nothing learned"


def _slices_of(n, b, learner_major):
    centres = [0, n - 1] + ([E31 // b, E32 // b] if learner_major else [(n // 2) // 256 * 256])
    return sorted({min(max(p - MS // 2, 0), n - MS) for p in centres})


@pytest.mark.parametrize("name,kernel,n,b,learner_major,kw", [pytest.param(*r, id=f"{r[0]}-N{r[2]}-{r[1]}") for r in AGENT_ROWS])
def test_large_footprint_newer_agents_against_their_numpy_loops(orc, name, kernel, n, b, learner_major, kw):
    """the f64 numpy loops of the agents' own test files (tests/*_numpy.py), started from the slices' pre-set state, at those files' bars: actions
    exact for the learners outside the near_boundary band (at least 3/4 of a slice compared), weights at the driver-loop tests' tolerance; HIV and
    LSTD (Random policy: the action IS the draw) every action exact, HIV's weights and hidden states and LSTD's f64 state at their files' bounds.
    One batch-step per call, so that every action is seen: the same bits as any other cut (the shard test above runs 4 + 2)."""
    from tests import hiv_numpy as hv
    from tests.ac_numpy import ac_restated_loop
    from tests.lstd_numpy import random_policy_actions, replay_trait_loop
    from tests.reinforce_numpy import reinforce_restated_loop
    from tests.tdac_numpy import tdac_restated_loop
    kw = dict(kw, seed=91, gamma=0.95, max_episode_steps=CAP)
    algo, domain, order, seed, gamma = kw["algo"], kw["domain"], kw["order"], 91, 0.95
    lstd, hiv = algo in (ra.RECURSIVE_LSTD, ra.ILSTD), kw["domain"] == ra.HIV_TREATMENT
    Ksteps = sum(CUT)
    offs = _slices_of(n, b, learner_major)
    rng = np.random.default_rng(1000 + len(name))
    r = dict(name=name, n=n)
    with _open(r, dict(kw, n_envs=n)) as c:
        F, A = c.F, c.A
        states = {off: [_random_state(rng, F, A, algo == ra.RECURSIVE_LSTD) for _ in range(MS)] for off in offs}
        for off in offs:
            for j in range(MS):
                _install(c, off + j, states[off][j])
        c.reset()
        S0, A0 = c.states, c.actions
        c.timing_enable(True)
        acts = {off: [] for off in offs}
        rec = {off: [] for off in offs}
        ep = np.zeros(n, dtype=np.int64)
        for k in range(Ksteps):
            if lstd:                                        # the trait loop with host arrays: the transitions are what the numpy rule replays
                a = c.actions
                frm, nxt, rew, term = c.domain_step(a)
                c.handle(frm, a, rew, nxt, term)
                ep += 1
                mask = (term.astype(bool) | (ep >= CAP)).astype(np.uint8)
                c.domain_reset(mask)
                ep[mask == 1] = 0
                now = c.policy_sample()
                for off in offs:
                    rec[off].append((frm[:, off:off + MS].copy(), nxt[:, off:off + MS].copy(), rew[off:off + MS].copy(), term[off:off + MS].copy()))
            else:
                c.train(1, want_stats=False)
                now = c.actions
            for off in offs:
                acts[off].append(now[off:off + MS].copy())
        if lstd:
            c.episode_steps = ep.astype(np.uint32)
        else:
            assert c.timing_read()[2] == kernel
        assert c.step_count == Ksteps
        S, EP = c.states, c.episode_steps
        Y = c.get_hidden_states() if hiv else None
        final = {off: [_agent_state(c, off + j) for j in range(MS)] for off in offs}
    if lstd:                                                # ... and k_train_lstd at the full size is that trait loop, bit for bit (test_gpu_lstd.py's bar)
        with _open(r, dict(kw, n_envs=n)) as c:
            for off in offs:
                for j in range(MS):
                    _install(c, off + j, states[off][j])
            c.reset()
            c.timing_enable(True)
            for k in CUT:
                c.train(k, want_stats=False)
            assert c.timing_read()[2] == kernel
            assert c.states.tobytes() == S.tobytes() and np.array_equal(c.episode_steps, EP)
            for off in offs:
                assert np.array_equal(c.actions[off:off + MS], acts[off][-1])
                for j in range(MS):
                    assert [x.tobytes() for x in _agent_state(c, off + j)] == [x.tobytes() for x in final[off][j]], (off, j)
    for off in offs:
        what = f"{name} learners {off}..{off + MS - 1}"
        st = states[off]
        s0, a0, dev = S0[:, off:off + MS], A0[off:off + MS], np.array(acts[off])
        if lstd:
            for k in range(Ksteps):                         # (RESET is an alias of STEP)
                assert np.array_equal(dev[k], random_policy_actions(orc, seed, 3, MS, k, orc.BLK_STEP, off)), (what, k)
            tol = 1e4 * F * Ksteps * np.finfo(np.float64).eps
            for j in range(0, MS, 4):
                init = (st[j]["theta"], st[j]["mat"], st[j]["mu"] if algo == ra.ILSTD else None)
                want = replay_trait_loop(orc, algo == ra.RECURSIVE_LSTD, domain, order, F, [(f[:, j], nx[:, j], rw[j], tm[j]) for f, nx, rw, tm in rec[off]],
                                         gamma, kw["alpha"], kw["n_steps"], init=init)
                for g, w in zip(final[off][j], want):
                    assert np.max(np.abs(g - w)) <= tol * (1.0 + np.max(np.abs(w))), (what, j)
                assert not np.array_equal(want[0], st[j]["theta"])
            continue
        if hiv:
            lo, hi = [-5.0] * 6, [8.0] * 6
            W0 = np.stack([x["W"] for x in st]).astype(np.float64)
            first, a, y, obs32, ep_, W, _ = hv.q_learning_random_loop(orc, lo, hi, order, F, MS, Ksteps, CAP, seed, kw["lr"], gamma, env_offset=off, W0=W0)
            assert np.array_equal(a0, first) and np.array_equal(dev[-1], a), what
            assert hv.bits_equal(np.ascontiguousarray(Y[:, off:off + MS]), y), what + ": hidden states"
            u = np.abs(np.ascontiguousarray(S[:, off:off + MS]).view(np.int32).astype(np.int64) - obs32.view(np.int32).astype(np.int64))
            assert np.all(u <= 1) and np.array_equal(EP[off:off + MS], ep_), what
            for j in range(MS):
                assert np.allclose(final[off][j][0], W[j], atol=2e-5, rtol=1e-4), (what, j)
                assert not np.allclose(W[j], W0[j], atol=2e-5, rtol=1e-4), (what, j, "nothing learned")
            continue
        W0, Th0 = [x["W"] for x in st], [x["Th"] for x in st]
        args = (domain, order, MS, Ksteps, CAP, seed, gamma)
        if algo == ra.ACTOR_CRITIC:
            ref, Ws, Ts, near = ac_restated_loop(orc, False, *args, kw["lr"], kw["alpha"], kw["tau"], s0, a0, env_offset=off, W0=W0, Th0=Th0)
            pairs = lambda j: ((final[off][j][0], Ws[j]), (final[off][j][1], Ts[j]))                  # noqa: E731
        elif algo == ra.TD_ACTOR_CRITIC:
            ref, ws, Ts, near = tdac_restated_loop(orc, *args, kw["lr"], kw["alpha"], kw["tau"], s0, a0, env_offset=off, w0=[w[:, 0] for w in W0], Th0=Th0)
            pairs = lambda j: ((final[off][j][0][:, 0], ws[j]), (final[off][j][1], Ts[j]))            # noqa: E731
        else:
            base = algo == ra.BASELINE_REINFORCE
            ref, Ts, Tbs, near = reinforce_restated_loop(orc, *args, kw["alpha"], kw["tau"], s0, a0, [w.astype(np.float64) for w in W0] if base else None,
                                                         env_offset=off, Th0=Th0)
            pairs = lambda j: ((final[off][j][-2], Ts[j]), (final[off][j][-1], Tbs[j]))               # noqa: E731
        same = (dev == ref).all(axis=0)
        print(f"{what}: same {same.mean():.3f} compared {(same & ~near).mean():.3f}")
        assert same.mean() >= 0.9, (what, same)
        assert (same & ~near).mean() >= 0.75, what
        for j in np.flatnonzero(same & ~near):
            for got, want in pairs(j):
                assert np.max(np.abs(got - want)) <= 3e-6 * (1 + np.max(np.abs(want))) * Ksteps * 16, (what, j)
            assert not np.array_equal(Ts[j], Th0[j]), (what, j, "nothing learned")


# ---- the trait-granular fast path (kernels_trait.hpp: per-wave buffer descriptors over a learner-major W) with device pointers -------------------
def _device_ptr_loop(c, k):
    """env.transition -> agent.handle -> [terminal: new episode] -> policy.sample, one C-ABI call each on device arrays (tests/test_gpu_trait_loop.py)"""
    import ctypes as C
    from rsrl_amd import _abi
    from rsrl_amd._devmem import DeviceBuffer
    L, h, n, D = c._L, c._h, c.N, c.D
    frm, to = DeviceBuffer(D * n, "float32"), DeviceBuffer(D * n, "float32")
    rew, act, term, td = DeviceBuffer(n, "float32"), DeviceBuffer(n, "int32"), DeviceBuffer(n, "uint8"), DeviceBuffer(n, "float32")
    p = lambda b: C.c_void_p(b.ptr)      # noqa: E731
    try:
        _abi.check(L.rsrl_hip_get_actions(h, p(act)))
        for _ in range(k):
            _abi.check(L.rsrl_hip_domain_step(h, p(act), p(frm), p(to), p(rew), p(term)))
            _abi.check(L.rsrl_hip_handle(h, p(frm), p(act), p(rew), p(to), p(term), n, p(td)))
            _abi.check(L.rsrl_hip_domain_reset(h, p(term)))
            _abi.check(L.rsrl_hip_policy_sample(h, None, n, p(act)))
        c.sync()
        return act.to_host(), term.to_host()
    finally:
        for buf in (frm, to, rew, act, term, td):
            buf.free()


# (learners, how the calls are served, the kernel timing_read() names last: the fast kernels name themselves; past 2^32 bytes W is feature-major and the
#  calls go to the generic kernels, which are not timed)
TRAIT_ROWS = [(7500003, "fused", "k_trait_lm<step>"), (7500003, "separate", "k_trait_lm<handle>"), (10240318, "fused", ""), (10240318, "separate", "")]


@pytest.mark.parametrize("n,mode,kernel", [pytest.param(*t, id=f"N{t[0]}-{t[1]}-{t[2] or 'generic-kernels'}") for t in TRAIT_ROWS])
def test_large_footprint_trait_loop_device_pointers_bitwise_vs_oracle(orc, monkeypatch, n, mode, kernel):
    # MountainCar Fourier(5), steps_per_launch = 1, 432 B per learner: 3.2 GB (learner-major W, the fast kernels' per-wave descriptors reach past
    # 2^31 bytes) and 4.4 GB (past what one descriptor addresses).  The loop restarts episodes on terminal transitions only, so half of every sampled
    # slice starts next to the goal; reference: the oracle's reference-order loop (orc_run_train, every Q evaluated afresh as the trait calls do)
    if mode == "separate":
        monkeypatch.setenv("RSRL_NO_TRAIT_DEFER", "1")
    Ksteps, b = sum(CUT), 432
    kw = dict(domain=MC, order=5, algo=ra.SARSA, steps_per_launch=1, seed=123, gamma=0.97, lr=0.2 / 36, alpha=0.2 / 36, max_episode_steps=0, **EG)
    centres = [0, n - 1, (n // 2) // 256 * 256] + [e // b for e in (E31, E32) if e < b * n]
    offs = sorted({min(max(p - 4, 0), n - M) for p in centres})
    rng = np.random.default_rng(n % 1000)
    r = dict(name=f"trait-{mode}", n=n)
    with _open(r, dict(kw, n_envs=n)) as c:
        W0 = {off: np.stack([_weights_for(rng, (c.F, c.n_out), False) for _ in range(M)]) for off in offs}
        for off in offs:
            for j in range(M):
                c.set_weights(W0[off][j], off + j)
        c.reset()
        S = c.states
        near_goal = np.stack([rng.uniform(0.44, 0.49, size=M // 2), rng.uniform(0.04, 0.065, size=M // 2)]).astype(np.float32)
        for off in offs:
            S[:, off:off + M // 2] = near_goal
        c.states = S
        c.timing_enable(True)
        act, term = _device_ptr_loop(c, Ksteps)
        named = c.timing_read()[2]
        print(f"trait loop N {n} {mode}: timing_read names {named!r}, slices at {offs}")
        assert named == kernel
        assert c.step_count == Ksteps
        Sf, Af = c.states, c.actions
        assert np.array_equal(act, Af)
        episodes = 0
        for off in offs:
            okw = oracle_kwargs(orc, dict(kw, n_envs=M))
            okw["env_offset"] = off
            run = orc.Run(orc.make_agent(**okw), M, "f32d")
            run.weights[:] = W0[off]
            run.reset()
            run.state[: M // 2] = near_goal.T
            episodes += run.train(Ksteps)["episodes"]
            what = f"trait loop {mode} N {n} learners {off}..{off + M - 1}"
            assert np.array_equal(Sf[:, off:off + M].T, run.state), what + ": states"
            assert np.array_equal(Af[off:off + M], run.action), what + ": actions"
            for j in range(M):
                assert np.array_equal(c.get_weights(off + j), run.weights[j]), f"{what}: weights of learner {off + j}"
            assert not np.array_equal(run.weights, W0[off])
        assert episodes >= len(offs), "the slices' learners next to the goal reach it inside the run"


# ---- SARSA(lambda) over ONE shared tile table with a sparse trace per learner: the value lists (512 x 4 B per learner) past 2^32 bytes ---------------
def test_large_footprint_sparse_trace_lists_bitwise_vs_oracle(orc):
    # the learners are coupled through the table, so the oracle replays ALL of them (train_sparse_lambda; about 20 s of one core for 2 160 069
    # learners x 6 steps, inside this module's budget): the table and every state / action bit for bit, the sparse traces of the learners around the
    # 2^31- and 2^32-byte offsets of the value lists (2 KiB per learner) and of the key lists (1 KiB per learner)
    n, Ksteps = 2160069, sum(CUT)
    kw = dict(domain=MC, algo=ra.SARSA_LAMBDA, lam=0.9, seed=17, gamma=0.97, lr=0.2 / 8 / n, alpha=0.2 / 8 / n, max_episode_steps=CAP, weight_mode=ra.W_SHARED, **TILE, **EG)
    assert n * 2048 > E32 and n * 1024 > E31
    picks = sorted({0, n - 1} | {e // bb + d for e in (E31, E32) for bb in (2048, 1024) if e // bb + 1 < n for d in (-1, 0, 1)})
    rng = np.random.default_rng(3)
    r = dict(name="sparse-trace-lambda", n=n)
    with _open(r, dict(kw, n_envs=n)) as c:
        w0 = (rng.normal(size=c.get_weights().shape) * 0.1).astype(np.float32)
        c.set_weights(w0)
        c.reset()
        c.timing_enable(True)
        st = c.train(CUT[0])
        c.train(CUT[1], want_stats=False)
        assert c.timing_read()[2] == "k_sparse_trace_scatter"
        assert st["env_steps"] == n * CUT[0] and st["episodes"] >= n
        okw = oracle_kwargs(orc, dict(kw, n_envs=n))
        run = orc.Run(orc.make_agent(**okw), n, "f32d")
        run.weights[:] = w0.reshape(run.weights.shape)
        run.reset()
        for k in CUT:
            run.train_sparse_lambda(k)
        print(f"sparse-trace lambda: N {n}, value lists {n * 2048 / 1e9:.2f} GB, traces compared at learners {picks}")
        assert np.array_equal(c.states.T, run.state) and np.array_equal(c.actions, run.action) and np.array_equal(c.episode_steps, run.ep_step)
        w = c.get_weights()
        assert np.array_equal(w, run.weights.reshape(w.shape)) and not np.array_equal(w, w0)
        for i in picks:
            z = run.sparse_trace(i)
            assert np.array_equal(c.get_traces(i), z), i
        assert any(np.abs(run.sparse_trace(i)).max() > 0 for i in picks)


def test_at_most_one_case_skipped_for_memory():
    assert len(SKIPPED_FOR_MEMORY) <= 1, SKIPPED_FOR_MEMORY
