"""tests/agent_contract.py without a GPU: `diff` sees what np.array_equal or the bytes alone would let through, `join_shards` puts every entry on
the axis its name says, and `check_train_invariance` fails on a ctx whose result depends on how the steps were split or whose shard ignores
env_offset -- on a fake Context over numpy arrays (a one-step value agent: weights, states, actions, episode steps)."""
import types

import numpy as np
import pytest

import rsrl_amd as ra
from tests.agent_contract import check_train_invariance, diff, join_shards, snapshot

D, F, A = 2, 3, 2


class FakeCtx:
    """train(k) is k rounds of its own domain_step / handle / domain_reset / policy_sample: honest by construction.  Every number is a function of
    (global learner id, step count), as the Philox streams are.  flaw "split": a train call that continues an earlier one nudges the weights;
    flaw "offset": the ids are local"""

    def __init__(self, n_envs, env_offset=0, max_episode_steps=0, steps_per_launch=0, algo=ra.SARSA, domain=ra.MOUNTAIN_CAR, flaw=None):
        self.cfg = types.SimpleNamespace(algo=algo, domain=domain)
        self.N, self.cap, self.flaw, self.t = n_envs, max_episode_steps, flaw, 0
        self.ids = np.arange(n_envs, dtype=np.int64) + (0 if flaw == "offset" else env_offset)
        self.W = np.zeros((n_envs, F, A), np.float32)
        self.states, self.actions, self.episode_steps = np.zeros((D, n_envs), np.float32), np.zeros(n_envs, np.int32), np.zeros(n_envs, np.uint32)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def _draw(self, salt):
        return ((self.ids * 2654435761 + self.t * 40503 + salt * 97) % 1013).astype(np.float32) / np.float32(1013.0)

    def get_weights(self, i):
        return self.W[i].copy()

    def reset(self):
        self.domain_reset(np.ones(self.N, np.uint8))
        self.policy_sample()

    def domain_step(self, actions):
        frm = self.states.copy()
        self.states = (frm * np.float32(0.5) + self._draw(1) + actions.astype(np.float32)).astype(np.float32)
        return frm, self.states.copy(), self._draw(2), (self._draw(3) < 0.1).astype(np.uint8)

    def handle(self, frm, actions, rew, nxt, term):
        self.W[np.arange(self.N), :, actions] += np.float32(0.01) * (rew * (1 - term))[:, None] * frm.T.sum(axis=1, keepdims=True)
        self.t += 1

    def domain_reset(self, mask):
        self.states[:, mask == 1] = np.float32(-0.5)

    def policy_sample(self):
        self.actions = (self._draw(4) + np.float32(0.1) * np.tanh(self.W[:, 0, 0]) > 0.5).astype(np.int32)

    def train(self, k):
        if self.flaw == "split" and self.t > 0:          # a call that continues an earlier one
            self.W += np.float32(2.0 ** -20)
        ep = self.episode_steps.astype(np.int64)
        for _ in range(k):
            frm, nxt, rew, term = self.domain_step(self.actions)
            self.handle(frm, self.actions, rew, nxt, term)
            ep += 1
            mask = (term.astype(bool) | ((ep >= self.cap) if self.cap > 0 else False)).astype(np.uint8)
            self.domain_reset(mask)
            ep[mask == 1] = 0
            self.policy_sample()
        self.episode_steps = ep.astype(np.uint32)
        return dict(env_steps=self.N * k)


def _snap(rng, n=4):
    return {"weights": rng.normal(size=(n, F, A)).astype(np.float32), "lstd_matrix": rng.normal(size=(n, F, F)),
            "states": rng.normal(size=(D, n)).astype(np.float32), "actions": rng.integers(0, A, size=n).astype(np.int32)}


def test_diff_is_empty_on_a_copy_and_names_what_differs():
    a = _snap(np.random.default_rng(0))
    b = {n: x.copy() for n, x in a.items()}
    assert diff(a, b) == []
    b["actions"][2] ^= 1
    assert diff(a, b) == ["actions"]
    del b["states"]
    assert diff(a, b) == ["states", "actions"] and diff(b, a) == ["actions", "states"]


def test_diff_reports_a_negative_zero_against_zero():
    a = _snap(np.random.default_rng(1))
    a["weights"][1, 2, 0] = 0.0
    b = {n: x.copy() for n, x in a.items()}
    b["weights"][1, 2, 0] = -0.0
    assert np.array_equal(a["weights"], b["weights"])          # what array_equal alone lets through
    assert diff(a, b) == ["weights"]


def test_diff_reports_two_nans_with_different_payloads():
    a = _snap(np.random.default_rng(2))
    b = {n: x.copy() for n, x in a.items()}
    a["lstd_matrix"].view(np.uint64)[0, 1, 1] = 0x7FF8000000000001
    b["lstd_matrix"].view(np.uint64)[0, 1, 1] = 0x7FF8000000000002
    assert np.isnan(a["lstd_matrix"][0, 1, 1]) and np.isnan(b["lstd_matrix"][0, 1, 1])
    assert diff(a, b) == ["lstd_matrix"]


def test_diff_reports_a_shape_mismatch():
    a = _snap(np.random.default_rng(3))
    b = {n: x.copy() for n, x in a.items()}
    b["states"] = b["states"].reshape(a["states"].shape[::-1])          # the same bytes
    assert diff(a, b) == ["states"]


def test_diff_reports_one_flipped_mantissa_bit_of_an_f64_entry():
    a = _snap(np.random.default_rng(4))
    b = {n: x.copy() for n, x in a.items()}
    b["lstd_matrix"].view(np.uint64)[3, 0, 2] ^= 1
    assert np.allclose(a["lstd_matrix"], b["lstd_matrix"], rtol=1e-15, atol=0)
    assert diff(a, b) == ["lstd_matrix"]


@pytest.mark.parametrize("dim", [2, 4])
def test_join_shards_puts_every_entry_on_its_axis(dim):
    rng = np.random.default_rng(dim)
    n1, n2 = 3, 5
    whole = {"weights": rng.normal(size=(n1 + n2, F, A)), "lstd_theta": rng.normal(size=(n1 + n2, F)), "theta": rng.normal(size=(n1 + n2, F, A)),
             "states": rng.normal(size=(dim, n1 + n2)), "hidden": rng.normal(size=(6, n1 + n2)), "actions": rng.integers(0, A, size=n1 + n2),
             "episode_steps": rng.integers(0, 9, size=n1 + n2), "return_carry": rng.normal(size=n1 + n2)}
    per_learner = ("weights", "lstd_theta", "theta")
    parts = [{n: (x[sl] if n in per_learner else x[..., sl]) for n, x in whole.items()} for sl in (slice(0, n1), slice(n1, None))]
    joined = join_shards(*parts)
    assert list(joined) == list(whole) and diff(joined, whole) == []
    assert joined["states"].shape == (dim, n1 + n2) and joined["weights"].shape == (n1 + n2, F, A)


def test_check_train_invariance_passes_an_honest_ctx_and_fails_the_two_flawed_ones():
    kw = dict(n_envs=8, max_episode_steps=5)
    st, ref = check_train_invariance(FakeCtx, kw, K=30, cap=5, depths=(1, 7), first_split=10)
    assert st["env_steps"] == 8 * 30 and list(ref) == ["weights", "states", "actions", "episode_steps"]
    assert np.abs(ref["weights"]).max() > 0 and len(set(ref["actions"])) == 2 and 0 < ref["episode_steps"].max() < 5
    with FakeCtx(**kw) as c:
        assert diff(snapshot(c, learners=[0, 7]), {n: (x[[0, 7]] if n == "weights" else x) for n, x in snapshot(c).items()}) == []
    for flaw, where in (("split", "steps_per_launch 1 .*: weights differ"), ("offset", "shards .*: weights, states, actions")):
        with pytest.raises(AssertionError, match=where):
            check_train_invariance(lambda **k: FakeCtx(flaw=flaw, **k), kw, K=30, cap=5, depths=(1, 7), first_split=10)
