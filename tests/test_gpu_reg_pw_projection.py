"""The producer-wave loop's own projection (rsrl_amd/csrc/fourier_reg_pw.hpp: one packed register move per pair of dimension-1 harmonics,
the statements in issue order) on crafted states: MountainCar, Fourier order 5, QLearning + epsilon-greedy, 1 000 learners, weights zero.

The states are set from outside: both bounds of each dimension, the normalised positions 0, 1/4, 1/2, 3/4, 1 (where sincospi's quadrant select
flips) and their float neighbours, velocity 0 and +- its maximum, every combination of these, and a seeded random remainder.  One batch-step,
then three more.  With W = 0 the first update writes fl(scale * phi(s)[f]) into the taken column and nothing else, and phi's last feature is
the constant 1, so the column's last row IS scale: a harmonic that landed in the wrong half of a pair, or in the wrong pair, shows in the weights.
Compared bit for bit: the default loop (pw::k_train_reg, with and without statistics -- the two instantiations) against RSRL_REG_PRODUCER=0
(k_train_reg) on weights, states, actions, episode steps and the carried Q; and both against the oracle's device-order run ("f32d")."""
import numpy as np
import pytest

import rsrl_amd as ra

pytestmark = pytest.mark.gpu

N = 1000
KW = dict(gamma=0.97, lr=0.05, epsilon=0.2, seed=31, max_episode_steps=1000)
CALLS = (1, 3)


def _crafted(orc):
    lo, hi = (b.astype(np.float32) for b in orc.domain_bounds(0))
    per_dim = []
    for d in range(2):
        v = [np.float32(lo[d] + np.float32(p) * (hi[d] - lo[d])) for p in (0.0, 0.25, 0.5, 0.75, 1.0)] + [lo[d], hi[d]]
        if d == 1:
            v.append(np.float32(0.0))
        v = np.array(v, dtype=np.float32)
        v = np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))])
        per_dim.append(np.unique(np.clip(v, lo[d], hi[d])))
    grid = np.array([(x, y) for x in per_dim[0] for y in per_dim[1]], dtype=np.float32).T          # (2, combinations)
    assert grid.shape[1] <= N // 2
    rng = np.random.default_rng(20)
    rest = (lo[:, None] + (hi - lo)[:, None] * rng.random((2, N - grid.shape[1]), dtype=np.float32)).astype(np.float32)
    s = np.ascontiguousarray(np.concatenate([grid, np.clip(rest, lo[:, None], hi[:, None])], axis=1))
    # spread the crafted learners over the blocks and waves instead of leaving them in the first four waves
    return np.ascontiguousarray(s[:, np.random.default_rng(21).permutation(N)])


def _device_run(knob, want_stats, states):
    with pytest.MonkeyPatch.context() as mp:
        if knob is None:
            mp.delenv("RSRL_REG_PRODUCER", raising=False)
        else:
            mp.setenv("RSRL_REG_PRODUCER", knob)                 # (read when the ctx is created)
        with ra.Context(domain=ra.MOUNTAIN_CAR, order=5, n_envs=N, algo=ra.QLEARNING, policy=ra.EPSILON_GREEDY, **KW) as c:
            c.reset()
            c.states = states
            snaps = []
            for k in CALLS:
                c.train(k, want_stats=want_stats)
                c.sync()
                q = c.q_carry
                assert q is not None
                snaps.append(dict(weights=np.stack([c.get_weights(i) for i in range(N)]), states=c.states, actions=c.actions,
                                  episode_steps=c.episode_steps, q_carry=q))
            return snaps


@pytest.fixture(scope="module")
def runs(orc):
    states = _crafted(orc)
    ag = orc.make_agent(policy=orc.EGREEDY, **KW)
    run = orc.Run(ag, N, "f32d")
    run.reset()
    run.state[:] = states.T
    run.invalidate_q()
    oracle = []
    for k in CALLS:
        run.train_dev(k)
        oracle.append(dict(weights=run.weights.copy(), states=run.state.T.copy(), actions=run.action.copy(), episode_steps=run.ep_step.copy()))
    run.close()
    return dict(s0=states, oracle=oracle, off=_device_run("0", True, states), on=_device_run(None, True, states),
                quiet=_device_run(None, False, states))


@pytest.mark.parametrize("arm", ["on", "quiet"])
def test_producer_loop_projects_the_lone_loops_bits(runs, arm):
    for j, (off, on) in enumerate(zip(runs["off"], runs[arm])):
        for k in off:
            assert off[k].tobytes() == on[k].tobytes(), f"{k} after call {j} ({CALLS[j]} batch-steps)"
    assert np.count_nonzero(runs["off"][0]["weights"]) > 0


@pytest.mark.parametrize("arm", ["off", "on", "quiet"])
def test_crafted_states_against_the_device_order_oracle(runs, arm):
    for j, (want, got) in enumerate(zip(runs["oracle"], runs[arm])):
        assert np.array_equal(got["weights"], want["weights"]), f"weights after call {j}"
        assert np.array_equal(got["states"], want["states"]) and np.array_equal(got["actions"], want["actions"]), f"call {j}"
        assert np.array_equal(got["episode_steps"].astype(np.int64), want["episode_steps"].astype(np.int64)), f"call {j}"


@pytest.mark.parametrize("arm", ["on", "quiet"])
def test_first_update_is_scale_times_phi_of_the_set_state(runs, orc, arm):
    w = runs[arm][0]["weights"]                                  # (N, F, A) after ONE batch-step from W = 0
    s0 = runs["s0"]
    unmoved = 0
    for i in range(N):
        taken = np.flatnonzero(w[i][-1])                         # phi's last feature is the constant 1: the last row holds scale in the taken column
        if len(taken) == 0:                                      # a zero TD error (the goal's reward is 0, Q is 0): nothing was written
            assert np.count_nonzero(w[i]) == 0, f"learner {i}"
            unmoved += 1
            continue
        assert len(taken) == 1, f"learner {i}: {w[i][-1]}"
        col, scale = w[i][:, taken[0]], w[i][-1, taken[0]]
        phi = orc.fourier_project(0, 5, s0[:, i], prec="f32d").astype(np.float32)
        assert phi[-1] == 1
        assert np.array_equal(col, (np.float32(scale) * phi).astype(np.float32)), f"learner {i}, state {s0[:, i]}"
        assert np.count_nonzero(np.delete(w[i], taken[0], axis=1)) == 0, f"learner {i}: a column of an action not taken was written"
    assert unmoved <= N // 10, unmoved                          # (only learners that reached the goal in this step)
