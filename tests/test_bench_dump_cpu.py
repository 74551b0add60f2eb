"""bench.py --dump-outputs: what the timed steps left for a caller (weights, states, actions, episode step counts) as .npy files -- float32 / float64 only,
within the size limit (a fixed, seeded sample of the learners above it), the same files for the same inputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class FakeContext:
    """the parts of rsrl_amd.Context that bench.dump_outputs reads, filled from a seed"""

    def __init__(self, n, F=36, A=3, D=2, seed=3):
        rng = np.random.default_rng(seed)
        self.N, self.F, self.n_out, self.D = n, F, A, D
        self.W = rng.standard_normal((n, F, A)).astype(np.float32)
        self.states = rng.standard_normal((D, n)).astype(np.float32)
        self.actions = rng.integers(0, A, n).astype(np.int32)
        self.episode_steps = rng.integers(0, 1000, n).astype(np.uint32)

    def get_weights(self, i):
        return self.W[i].copy()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_every_learner_below_the_limit(tmp_path):
    import bench
    c = FakeContext(300)
    rec = bench.dump_outputs(c, str(tmp_path / "out"))
    got = _load(tmp_path / "out")
    assert set(got) == {"weights", "states", "actions", "episode_steps", "learner_index"} and rec["learners"] == 300
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["weights"], c.W) and np.array_equal(got["states"], c.states)
    assert np.array_equal(got["actions"], c.actions.astype(np.float32)) and np.array_equal(got["episode_steps"], c.episode_steps.astype(np.float32))
    assert np.array_equal(got["learner_index"], np.arange(300))
    assert rec["bytes"] == sum(a.nbytes for a in got.values())


def test_a_seeded_sample_above_the_limit(tmp_path):
    import bench
    c = FakeContext(5000)
    limit = 200 * 1024
    rec = [bench.dump_outputs(c, str(tmp_path / d), limit_bytes=limit) for d in ("a", "b")]
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert 0 < rec[0]["learners"] < 5000 and rec[0]["bytes"] <= limit and sum(x.nbytes for x in a.values()) <= limit
    idx = a["learner_index"].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and np.array_equal(a["weights"], c.W[idx]) and np.array_equal(a["states"], c.states[:, idx])
    for k in a:                                                           # the same inputs give the same files
        assert np.array_equal(a[k], b[k]), k


def test_rank_suffix(tmp_path):
    import bench
    rec = bench.dump_outputs(FakeContext(10), str(tmp_path), suffix="_rank1")
    assert sorted(os.listdir(tmp_path)) == rec["files"] and all(f.endswith("_rank1.npy") for f in rec["files"])
