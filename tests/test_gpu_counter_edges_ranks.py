"""Rank groups started 5 batch-steps below 2^32 (tests/test_gpu_counter_edges.py has the single-ctx cases and how the counter gets there): G ranks on
one device over ONE shared approximator, every rank loaded at T0 = 2^32 - 5, 12 batch-steps (cut 5 + 7: the edge lies inside the first call).  The
exchanges' tags follow the number of exchanges (peer_seq / px_seq, 0 here), not t: what runs is Common::xdelta = peer_seq - t near -2^32 added to
the host's t (and, peer kind, a third call of 45 steps whose 32-step graphs add the device-side counter), and every rank's draw streams at a high t.

  rccl   the single-thread group (rsrl_hip_group_train) over the test double of RCCL (tests/stubs/rccl_stub.cpp; plain launches: the double does
         not support stream capture)
  peer   one host thread per rank, peer-write exchange through same-process pointers; with the persistent kernel and with per-step exchanges

Every replica of W must be identical, and the group must reproduce the unsharded run AT THE SAME T0: bit for bit for the dense basis (shards of
whole 512-learner blocks, exact 64-bit sums across ranks; the per-step peer exchange sums float deltas in rank order and keeps that only for
G = 2); tile coding to the bound of test_gpu_rccl_stub.py / fuzz_ranks.py (the G-term float sum
over ranks regroups: err_w <= 2e-6 max(1, |W|), >= 99 % of the states identical).  The waits are bounded (peer_timeout_ms, thread joins, the
subprocess's own time limit): a time-out is a failure that reports the library's error, never retried."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = (1 << 32) - 5

SCRIPT = r'''
import json, os, struct, sys, threading
import numpy as np
sys.path.insert(0, os.environ["RSRL_ROOT"])
import rsrl_amd as ra
from rsrl_amd.distributed import shard_range
G, kind, basis, T0, tmp = int(os.environ["G"]), os.environ["KIND"], os.environ["BASIS"], int(os.environ["T0"]), os.environ["TMP"]
N = G * 512
exchange = ra.EXCHANGE_RCCL if kind == "rccl" else ra.EXCHANGE_PEER
if basis == "dense":
    kw = dict(domain=0, order=3, algo=1, policy=1, epsilon=0.3, gamma=0.9, weight_mode=1, seed=7, max_episode_steps=5, lr=0.01 / N)
else:
    kw = dict(domain=2, basis=1, n_tilings=8, tiles_per_dim=6, algo=1, policy=1, epsilon=0.3, gamma=0.99, weight_mode=1, seed=7, max_episode_steps=5, lr=0.1 / 8 / N)
CALLS = (5, 7) if kind == "rccl" else (5, 7, 45)

def at_t0(c, name):
    a, b = os.path.join(tmp, name + ".fresh"), os.path.join(tmp, name + ".t0")
    c.save_weights(a)
    raw = bytearray(open(a, "rb").read())
    assert struct.unpack_from("<Q", raw, 64)[0] == 0
    struct.pack_into("<Q", raw, 64, T0)
    open(b, "wb").write(raw)
    c.load_weights(b)
    c.reset()
    assert c.step_count == T0

ctxs = [ra.Context(n_envs=cnt, env_offset=off, exchange=exchange, peer_timeout_ms=3000, **kw) for off, cnt in (shard_range(N, G, r) for r in range(G))]
errs = []
if kind == "rccl":
    for r, c in enumerate(ctxs): at_t0(c, f"rank{r}")
    ra.Context.group_create(ctxs)
    for c in ctxs: c.reset()
    for k in CALLS: ra.Context.group_train(ctxs, k)
    for c in ctxs: c.sync()
else:
    handles = [c.peer_export(G) for c in ctxs]
    for r, c in enumerate(ctxs): c.peer_connect(handles, r)
    def work(r):
        try:
            at_t0(ctxs[r], f"rank{r}")
            for k in CALLS: ctxs[r].train(k, want_stats=False)
            ctxs[r].sync()
        except Exception as e:
            errs.append(f"rank {r}: {e!r}"[:400])
    th = [threading.Thread(target=work, args=(r,)) for r in range(G)]
    [t.start() for t in th]; [t.join(120) for t in th]
    if any(t.is_alive() for t in th): errs.append("a rank did not return within 120 s")
out = {"errs": errs}
if not errs:
    W = [c.get_weights() for c in ctxs]
    out["t"] = [c.step_count for c in ctxs]
    out["replicas_equal"] = bool(all(np.array_equal(W[0], w) for w in W[1:]))
    with ra.Context(n_envs=N, **kw) as full:
        at_t0(full, "full")
        for k in CALLS: full.train(k, want_stats=False)
        Wf, Sf, Af = full.get_weights(), full.states, full.actions
    out["absw"] = float(np.abs(Wf).max())
    out["err_w"] = float(np.abs(W[0] - Wf).max())
    S = np.concatenate([c.states for c in ctxs], axis=1)
    A = np.concatenate([c.actions for c in ctxs])
    out["states_same"] = float(np.all(S == Sf, axis=0).mean())
    out["actions_same"] = float((A == Af).mean())
print("RESULT " + json.dumps(out), flush=True)
os._exit(0)
'''


def _run(tmp_path, G, kind, basis, no_persist=False):
    from rsrl_amd import _build
    script = tmp_path / "edge_ranks_run.py"
    script.write_text(SCRIPT)
    env = dict(os.environ, RSRL_ROOT=ROOT, G=str(G), KIND=kind, BASIS=basis, T0=str(T0), TMP=str(tmp_path), GPU_MAX_HW_QUEUES=str(2 * G))
    if kind == "rccl":
        stub = _build.build_rccl_stub()
        env.update(RCCL_STUB=stub, LD_PRELOAD=":".join(filter(None, (stub, os.environ.get("LD_PRELOAD")))), RSRL_NO_GRAPH="1")
    if no_persist:
        env["RSRL_NO_PERSIST"] = "1"
    p = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=420)
    assert p.returncode == 0 and "RESULT " in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    print(G, kind, basis, "no_persist" if no_persist else "", d)
    return d


@pytest.mark.parametrize("basis", ["dense", "tile"])
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("kind,no_persist", [("rccl", False), ("peer", False), ("peer", True)], ids=["rccl-double", "peer", "peer-per-step"])
def test_group_loaded_below_2p32_is_the_unsharded_run(tmp_path, kind, no_persist, G, basis):
    d = _run(tmp_path, G, kind, basis, no_persist)
    assert d["errs"] == [], d["errs"]
    steps = 12 if kind == "rccl" else 57
    assert d["t"] == [T0 + steps] * G
    assert d["replicas_equal"] and d["absw"] > 0, d
    if basis == "dense" and no_persist:
        # the per-step peer exchange sums the ranks' float deltas in rank order: G = 4 regroups them (the bound test_gpu_multirank.py uses for
        # regrouped sums; measured 3e-8 at |W| = 0.18, the same at T0 = 0, 1000 and 2^32 - 5, every state and action identical)
        assert d["err_w"] <= 1e-6 * max(1.0, d["absw"]) and d["states_same"] >= 0.99 and d["actions_same"] >= 0.99, d
        assert G > 2 or d["err_w"] == 0.0, d
    elif basis == "dense":
        assert d["err_w"] == 0.0 and d["states_same"] == 1.0 and d["actions_same"] == 1.0, d
    else:
        assert d["err_w"] <= 2e-6 * max(1.0, d["absw"]) and d["states_same"] >= 0.99, d
