"""Checkpoint files, pinned byte for byte: one small ctx per payload layout (aux_kind 0..8, the epsilon schedule's version 4, and the weight
layouts k_weights_get walks), reset, trained a fixed number of batch-steps from a fixed seed, saved -- sha256 and size of every file go into
tests/golden/checkpoint_digests.json.  tests/test_gpu_checkpoint_format.py runs digests() again and compares: a change of the writer that moves
one byte of one file fails there.  Training is bit-reproducible (the suite asserts it), so the files are.

    python tests/golden/make_checkpoint_digests.py            (on the GPU; rewrites the JSON)
"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "checkpoint_digests.json")

# name -> (Context keywords, batch-steps trained before the save, file version, aux_kind).  Constants are spelt as the ABI's numbers
# (rsrl_amd/context.py): domain 0 MountainCar / 1 CartPole; basis 1 tile coding; policy 1 epsilon-greedy / 2 softmax / 3 random;
# weight_mode 1 shared; weight_dtype 1 bf16.
CASES = {
    # aux_kind 0: weights only
    "q_per_learner": (dict(domain=0, order=3, algo=0, policy=1, epsilon=0.1, n_envs=32, seed=11, max_episode_steps=20), 40, 2, 0),
    "q_shared": (dict(domain=0, order=3, algo=0, policy=1, epsilon=0.1, n_envs=32, seed=11, max_episode_steps=20, weight_mode=1, lr=0.001 / 32), 40, 2, 0),
    "q_wave_order7": (dict(domain=1, order=7, algo=0, policy=1, epsilon=0.1, n_envs=8, seed=11, max_episode_steps=20), 40, 2, 0),
    "q_wave_bf16": (dict(domain=1, order=7, algo=0, policy=1, epsilon=0.1, n_envs=8, seed=11, max_episode_steps=20, weight_dtype=1), 40, 2, 0),
    "q_tile": (dict(domain=0, basis=1, n_tilings=4, tiles_per_dim=4, algo=0, policy=1, epsilon=0.1, n_envs=32, seed=11, max_episode_steps=20, lr=0.01), 40, 2, 0),
    "q_single_step": (dict(domain=0, order=3, algo=0, policy=1, epsilon=0.1, n_envs=32, seed=11, max_episode_steps=20, steps_per_launch=1), 40, 2, 0),
    # aux_kind 1: eligibility traces
    "sarsa_lambda": (dict(domain=0, order=3, algo=3, policy=1, epsilon=0.2, gamma=0.99, alpha=0.01, lam=0.7, n_envs=32, seed=12, max_episode_steps=20), 40, 2, 1),
    "td_lambda": (dict(domain=0, order=3, algo=8, policy=3, gamma=0.9, alpha=0.05, lam=0.3, n_envs=32, seed=12, max_episode_steps=20), 40, 2, 1),
    # aux_kind 2: fa_td's weights
    "greedy_gq": (dict(domain=0, order=3, algo=6, policy=1, epsilon=0.2, gamma=0.9, lr=0.01, lr_td=0.005, n_envs=32, seed=13, max_episode_steps=20), 40, 2, 2),
    # aux_kind 3: the n-step backups
    "q_sigma": (dict(domain=0, order=3, algo=9, policy=1, epsilon=0.2, gamma=0.9, lr=0.01, alpha=0.5, sigma=0.5, n_steps=3, n_envs=16, seed=1, max_episode_steps=30), 50, 3, 3),
    # aux_kind 4: sparse traces over the shared tile table (non-empty lists after 100 batch-steps)
    "sparse_lambda": (dict(domain=0, basis=1, n_tilings=8, tiles_per_dim=8, algo=3, policy=1, epsilon=0.3, gamma=0.99, lam=0.97, trace=2, weight_mode=1, seed=7,
                           alpha=0.1 / 8 / 32, n_envs=32), 100, 6, 4),
    # aux_kind 5: ActorCritic's theta (both SARSA critics)
    "actor_critic": (dict(domain=0, order=3, algo=10, policy=2, n_envs=32, seed=5, gamma=0.95, lr=0.02, alpha=0.2, tau=0.5, max_episode_steps=17), 25, 7, 5),
    "q_actor_critic": (dict(domain=0, order=3, algo=11, policy=2, n_envs=32, seed=5, gamma=0.95, lr=0.02, alpha=0.2, tau=0.5, max_episode_steps=17), 25, 7, 5),
    # aux_kind 6: the TD ActorCritic's theta
    "td_actor_critic": (dict(domain=0, order=3, algo=13, policy=2, n_envs=32, seed=5, gamma=0.95, lr=0.02, alpha=0.2, tau=0.5, max_episode_steps=17), 25, 8, 6),
    # aux_kind 7: theta, theta_b, g (REINFORCE has no weights section)
    "reinforce": (dict(domain=0, order=3, algo=15, policy=2, n_envs=32, seed=5, gamma=0.95, alpha=0.2, tau=0.5, max_episode_steps=17), 25, 9, 7),
    "baseline_reinforce": (dict(domain=0, order=3, algo=16, policy=2, n_envs=32, seed=5, gamma=0.95, alpha=0.2, tau=0.5, max_episode_steps=17), 25, 9, 7),
    # aux_kind 8: the f64 least-squares state (iLSTD's has mu)
    "recursive_lstd": (dict(domain=0, order=3, algo=18, policy=3, n_envs=32, seed=5, gamma=0.95, alpha=0.05, n_steps=3, max_episode_steps=17), 25, 10, 8),
    "ilstd": (dict(domain=0, order=3, algo=19, policy=3, n_envs=32, seed=5, gamma=0.95, alpha=0.05, n_steps=3, max_episode_steps=17), 25, 10, 8),
    # the per-learner epsilon schedule: version 4 whatever the aux_kind (here 1), eps[N] at the end
    "eps_schedule": (dict(domain=0, order=3, algo=3, policy=1, trace=1, gamma=0.99, alpha=0.01, lam=0.7, epsilon=0.2, epsilon_decay=0.99, n_envs=32, seed=2,
                          max_episode_steps=20), 60, 4, 1),
}


def write_case(name, path):
    """create the case's ctx, reset, train, save to `path`; -> (the writer's checksum, the Context keywords)"""
    import rsrl_amd
    kw, steps, _, _ = CASES[name]
    with rsrl_amd.Context(**kw) as c:
        c.reset()
        c.train(steps, want_stats=False)
        c.save_weights(path)
        return c.checksum(), kw


def digests(tmpdir, names=None):
    """-> {case: {"sha256", "bytes", "version", "aux_kind"}}, the files left in tmpdir as <case>.ckpt, and {case: the writer's checksum}"""
    import struct
    out, sums = {}, {}
    for name in (names or CASES):
        path = os.path.join(tmpdir, name + ".ckpt")
        sums[name], _ = write_case(name, path)
        raw = open(path, "rb").read()
        out[name] = {"sha256": hashlib.sha256(raw).hexdigest(), "bytes": len(raw),
                     "version": struct.unpack_from("<I", raw, 8)[0], "aux_kind": struct.unpack_from("<i", raw, 12 + 10 * 4)[0]}
    return out, sums


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        got, _ = digests(tmp)
        again, _ = digests(tmp)
    assert got == again, "a case's file differs between two runs: " + ", ".join(k for k in got if got[k] != again[k])
    for name, (_, _, version, aux_kind) in CASES.items():
        assert (got[name]["version"], got[name]["aux_kind"]) == (version, aux_kind), (name, got[name])
    with open(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(got, indent=1, sort_keys=True))
