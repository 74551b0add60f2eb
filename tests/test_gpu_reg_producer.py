"""The fused loop whose Philox draws come from a partner wave per SIMD (kernels_reg_pw.hpp, pw::k_train_reg) against the loop that draws
for itself (k_train_reg): the same library, two ctxs -- RSRL_REG_PRODUCER=0 and the default -- compared BIT FOR BIT: weights, states, actions,
episode steps, the carried Q(s,.) and every call's statistics; and once more without statistics, where the producer loop runs its instantiation without
the per-step accumulators.  (Against the oracle the existing bitwise suites run the new loop by default.)

The ring holds 2 x H pairs of batch-steps per consumer wave, H = 8 (kRingPairs): one workgroup barrier per 16 batch-steps.  The run is cut into
calls of 1, 2, 2H-1, 2H, 2H+1, 0, 4H+3 and 5 batch-steps (every call asks for statistics, so every call is launched on its own): launches start
at odd and at even batch-steps, are shorter than a ring half, exactly one half and several halves long.  steps_per_launch = 5 cuts the same calls
into launches that never reach a barrier past the first; the default depth runs each call as one launch.  max_episode_steps = 7 puts the step-cap
slow path (a divergent branch, no barrier inside) between barriers; 1000 never truncates inside the run.
n_envs: 1, 63, 64, 65 (partial waves; consumer waves wholly beyond the end, which must still walk every barrier), 255, 257 (a last block with
three such waves), 1000 (several blocks)."""
import ctypes as C

import numpy as np
import pytest

import rsrl_amd as ra
from rsrl_amd import _devmem

pytestmark = pytest.mark.gpu

H = 8                                                    # kRingPairs of kernels_reg_pw.hpp
CALLS = [1, 2, 2 * H - 1, 2 * H, 2 * H + 1, 0, 4 * H + 3, 5]
CONFIGS = {
    "qlearning-egreedy": dict(algo=ra.QLEARNING, policy=ra.EPSILON_GREEDY, epsilon=0.2),
    "sarsa-egreedy": dict(algo=ra.SARSA, policy=ra.EPSILON_GREEDY, epsilon=0.2),          # the agent's own draw: the inner stream
    "esarsa-softmax": dict(algo=ra.EXPECTED_SARSA, policy=ra.SOFTMAX, tau=0.5, alpha=0.5),
    "pal-greedy": dict(algo=ra.PAL, policy=ra.GREEDY, alpha=0.5),
}
N_ENVS = [1, 63, 64, 65, 255, 257, 1000]


def _run(monkeypatch, knob, kw, calls, learners=None, want_stats=True):
    """the run under RSRL_REG_PRODUCER = knob (None: unset) -> everything the two loops must agree on, as bytes / plain values.  Without statistics
    a call only enqueues (and calls that find the stream busy are coalesced): sync() after each keeps one launch per call there too."""
    if knob is None:
        monkeypatch.delenv("RSRL_REG_PRODUCER", raising=False)
    else:
        monkeypatch.setenv("RSRL_REG_PRODUCER", knob)          # (read when the ctx is created)
    with ra.Context(**kw) as c:
        c.reset()
        c.timing_enable(True)
        stats = []
        for k in calls:
            stats.append(c.train(k, want_stats=want_stats))
            c.sync()
        assert c.timing_read()[2] == "k_train_reg"              # one family, one reported name, whichever loop ran
        assert c.step_count == sum(calls)
        q = c.q_carry
        learners = range(c.N) if learners is None else learners
        return dict(stats=stats, states=c.states.tobytes(), actions=c.actions.tobytes(), episode_steps=c.episode_steps.tobytes(),
                    q_carry=None if q is None else q.tobytes(), checksum=c.checksum(),
                    weights=b"".join(c.get_weights(i).tobytes() for i in learners))


def _differences(a, b):
    bad = [k for k in a if k != "stats" and a[k] != b[k]]
    bad += [f"stats of call {j}: {k}" for j, (x, y) in enumerate(zip(a["stats"], b["stats"])) for k in (x or {}) if x[k] != y[k]]      # (the f64 sums too: same order)
    return bad


@pytest.mark.parametrize("n_envs", N_ENVS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_producer_loop_is_the_lone_loop_bit_for_bit(monkeypatch, config, n_envs):
    for cap in (7, 1000):
        for spl in (0, 5):
            kw = dict(domain=ra.MOUNTAIN_CAR, order=5, n_envs=n_envs, seed=77 + n_envs, gamma=0.97, lr=0.005, max_episode_steps=cap, steps_per_launch=spl,
                      **CONFIGS[config])
            off = _run(monkeypatch, "0", kw, CALLS)
            on = _run(monkeypatch, None, kw, CALLS)
            what = f"{config} n_envs {n_envs} max_episode_steps {cap} steps_per_launch {spl}"
            assert _differences(off, on) == [], what
            assert off["q_carry"] is not None, what
            episodes = sum(s["episodes"] for s in off["stats"])
            assert episodes >= n_envs * (sum(CALLS) // cap) if cap == 7 else episodes == 0, what      # the step cap was (was not) met
            assert sum(s["sum_abs_td_error"] for s in off["stats"]) > 0, what
            # launches that return no statistics run the producer loop's instantiation without the per-step accumulators: the same bits again
            quiet = _run(monkeypatch, None, kw, CALLS, want_stats=False)
            assert _differences(dict(off, stats=[None] * len(CALLS)), quiet) == [], what + " (no statistics)"


def test_beyond_one_block_per_cu_the_lone_loop_stays(monkeypatch):
    """n_envs = 256 x CUs + 256: one block more than the device has CUs -- there k_train_reg runs two learner waves per SIMD already and is kept
    (the selection is made at create); knob on and knob off are then the same kernel, and the same bits."""
    cus = C.c_int(0)
    assert _devmem.hip().hipDeviceGetAttribute(C.byref(cus), 63, 0) == 0            # 63 = hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)
    assert 1 <= cus.value <= 1024, cus.value
    n = 256 * cus.value + 256
    kw = dict(domain=ra.MOUNTAIN_CAR, order=5, n_envs=n, seed=5, gamma=0.97, lr=0.005, max_episode_steps=4, **CONFIGS["sarsa-egreedy"])
    learners = list(range(0, n, 997)) + list(range(n - 300, n))
    off = _run(monkeypatch, "0", kw, [6], learners)
    on = _run(monkeypatch, None, kw, [6], learners)
    assert _differences(off, on) == []
    assert off["stats"][0]["episodes"] == n and off["stats"][0]["env_steps"] == 6 * n
