"""The iLSTD ActorCritic's checkpoint file (file version 10, aux_kind 9), pinned byte for byte as tests/golden/make_checkpoint_digests.py pins the
other payload layouts: a small ctx, reset, trained a fixed number of batch-steps from a fixed seed, saved -- sha256 and size go into
tests/golden/checkpoint_digest_tdac_lstd.json, and tests/test_gpu_tdac_lstd.py writes the file again and compares.

    python tests/golden/make_checkpoint_digest_tdac_lstd.py            (on the GPU; rewrites the JSON)
"""
import hashlib
import json
import os
import struct
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "checkpoint_digest_tdac_lstd.json")
NAME = "ilstd_actor_critic"
# Context keywords (the ABI's numbers: MountainCar, algo 21, Softmax), batch-steps trained before the save, file version, aux_kind
CASE = (dict(domain=0, order=3, algo=21, policy=2, n_envs=32, seed=5, gamma=0.95, lr=0.05, alpha=0.2, tau=0.5, n_steps=3, max_episode_steps=17), 25, 10, 9)


def write_case(path):
    """create the ctx, reset, train, save to `path`; -> the writer's checksum"""
    import rsrl_amd
    kw, steps, _, _ = CASE
    with rsrl_amd.Context(**kw) as c:
        c.reset()
        c.train(steps, want_stats=False)
        c.save_weights(path)
        return c.checksum()


def digest(tmpdir):
    """-> ({"sha256", "bytes", "version", "aux_kind"}, the writer's checksum); the file is left in tmpdir as <NAME>.ckpt"""
    path = os.path.join(tmpdir, NAME + ".ckpt")
    checksum = write_case(path)
    raw = open(path, "rb").read()
    return {"sha256": hashlib.sha256(raw).hexdigest(), "bytes": len(raw), "version": struct.unpack_from("<I", raw, 8)[0],
            "aux_kind": struct.unpack_from("<i", raw, 12 + 10 * 4)[0]}, checksum


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        got, _ = digest(tmp)
        again, _ = digest(tmp)
    assert got == again, "the file differs between two runs"
    assert (got["version"], got["aux_kind"]) == CASE[2:], got
    with open(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, "w") as f:
        json.dump({NAME: got}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({NAME: got}, indent=1, sort_keys=True))
