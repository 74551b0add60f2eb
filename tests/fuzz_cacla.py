#!/usr/bin/env python3
"""Random campaign over CACLA (33) on ContinuousMountainCar with the Gaussian policy, on tests/fuzz_beta.py's pattern: the Fourier orders 1-5 at
random learner counts (partial blocks), seeds, env offsets (ids that straddle 2^31, the top of the id range), discounts, rates, episode caps
(0: none; 1: every step ends an episode), launch depths and shards; horizons up to 24 batch-steps.  Legs:

    train    train(K), cut into one to three calls, against the host trait loop (domain_step -> handle -> domain_reset(ended) -> policy_sample) --
             w, both columns, states, actions and episode steps bit for bit; every third case also against two env_offset shards joined
    ckpt     every third case: save after train(K1), load into a fresh ctx, carry the env side over, train(K2) on both -- the same bits
    handle   learners given random w and columns and a partial batch of M <= N transitions, two calls in a row: td and w bit for bit against
             tests/cacla_numpy.td_gate_f32 (the oracle's device-order projection), the gate of every learner the restatement's, closed-gate
             learners' columns and every learner past M byte for byte as they were, open-gate learners' columns moved

    python tests/fuzz_cacla.py [n_cases=200] [seed=0]      (GPU box; test infrastructure: imports oracle/)

One line per case and a SUMMARY {json} line; exit code 1 on any mismatch."""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rsrl_amd as ra  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import cacla_numpy as cn  # noqa: E402
from tests.agent_contract import diff, join_shards, snapshot, trait_loop  # noqa: E402

TOP_OF_IDS = -1
MAX_K = 24
SUITE_SEED, SUITE_CASES = 20261020, 150                              # the slice tests/test_gpu_cacla.py runs


def case_rng(seed, idx):
    return np.random.default_rng([seed, idx, cn.CACLA])


def sample(rng):
    kw = dict(domain=ra.CONTINUOUS_MOUNTAIN_CAR, order=int(rng.integers(1, 6)), algo=ra.CACLA, policy=ra.GAUSSIAN, seed=int(rng.integers(0, 1 << 20)),
              gamma=float(rng.choice([0.0, 0.9, 0.99, 1.0])), lr=float(rng.choice([0.0, 0.001, 0.02, 0.05])), alpha=float(rng.choice([0.0, 0.001, 0.01])),
              n_envs=int(rng.choice([1, 2, 5, 63, 64, 66, 130])), env_offset=int(rng.choice([0, 64, 1000003, (1 << 31) - 33, TOP_OF_IDS])),
              max_episode_steps=int(rng.choice([0, 1, 2, 7, 25])), steps_per_launch=int(rng.choice([0, 1, 5, 64])))
    if kw["env_offset"] == TOP_OF_IDS:
        kw["env_offset"] = (1 << 32) - 1 - kw["n_envs"]
    return kw


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def full(c):
    """tests/agent_contract.snapshot and the policy's columns"""
    out = snapshot(c)
    out["theta"] = np.stack([c.get_policy_weights(i) for i in range(c.N)])
    return out


def start(c):
    """reset, then every third learner (by global id) near the goal, so that terminal ends occur as well as cut ones, and every second one with
    V = -40 everywhere (the constant feature is the last one): from w = 0 and rewards of -1 no gate opens within such short horizons"""
    c.reset()
    ids = np.arange(c.N) + c.cfg.env_offset
    s = c.states
    s[:, ids % 3 == 0] = np.array([[0.59], [0.06]], dtype=np.float32)
    c.states = s
    w = np.zeros((c.F, 1), dtype=np.float32)
    w[c.F - 1] = -40.0
    for i in np.nonzero(ids % 2 == 0)[0]:
        c.set_weights(w, int(i))


def project(order, S):
    return np.stack([orc.fourier_project(orc.MOUNTAIN_CAR, order, S[:, i], "f32d") for i in range(S.shape[1])]).astype(np.float32)


def handle_leg(c, kw, rng, legs):
    bad = []
    N, F, order = c.N, c.F, kw["order"]
    w = rng.uniform(-0.5, 0.5, size=(N, F)).astype(np.float32)
    W = (rng.normal(size=(N, F, 2)) * 0.3 / np.sqrt(F)).astype(np.float32)
    for i in range(N):
        c.set_weights(w[i].reshape(F, 1), i)
        c.set_policy_weights(W[i], i)
    M = int(rng.integers(1, N + 1))
    lo, hi = orc.domain_bounds(orc.MOUNTAIN_CAR)
    for call in range(2):
        c.states = rng.uniform(lo, hi, size=(N, 2)).T.astype(np.float32)
        a = rng.uniform(-1.5, 1.5, size=N).astype(np.float32)
        frm, nxt, rew, term = c.domain_step(a)
        term = (term | (rng.random(N) < 0.25)).astype(np.uint8)
        rew = (rew + rng.uniform(-1.0, 2.0, size=N)).astype(np.float32)          # handle takes any reward: both gate outcomes occur
        t0 = c.step_count
        td = c.handle(frm[:, :M], a[:M], rew[:M], nxt[:, :M], term[:M])
        if c.step_count != t0 + 1:
            bad.append("handle is not one batch-step")
        want_td, w[:M], _, _, gate = cn.td_gate_f32(w[:M], project(order, frm[:, :M]), project(order, nxt[:, :M]), rew[:M], term[:M] != 0, kw["gamma"], kw["lr"])
        g_w = np.stack([c.get_weights(i)[:, 0] for i in range(N)])
        g_W = np.stack([c.get_policy_weights(i) for i in range(N)])
        if not np.array_equal(bits(td), bits(want_td)):
            bad.append(f"td of call {call} (M {M})")
        if not np.array_equal(bits(g_w), bits(w)):
            bad.append(f"w of call {call} (M {M})")
        same = np.array([g_W[i].tobytes() == W[i].tobytes() for i in range(N)])
        if not same[M:].all():
            bad.append(f"a learner past M = {M} moved in call {call}")
        if not same[:M][~gate].all():
            bad.append(f"a closed gate moved its columns in call {call}")
        if kw["alpha"] > 0 and same[:M][gate].any():
            bad.append(f"an open gate left its columns in call {call}")
        if kw["alpha"] == 0 and not np.array_equal(g_W, W):                      # (e = 0: fma(0, phi, w) is w as a value)
            bad.append(f"alpha = 0 moved a column in call {call}")
        W = g_W
    legs["handle"] = legs.get("handle", 0) + 1
    return bad


def train_leg(kw, rng, legs, shard):
    bad = []
    N, cap = kw["n_envs"], kw["max_episode_steps"]
    K = int(rng.integers(2, MAX_K + 1))
    cuts = sorted(set(int(x) for x in rng.integers(1, K, size=int(rng.integers(0, 3)))))
    calls = [b - a for a, b in zip([0] + cuts, cuts + [K])]
    with ra.Context(**kw) as c:
        start(c)
        for k in calls:
            c.train(k, want_stats=bool(rng.integers(0, 2)))
        ref, ck = full(c), c.checksum()
    with ra.Context(**dict(kw, steps_per_launch=0)) as c:
        start(c)
        trait_loop(c, K, cap)
        names = diff(full(c), ref)
        if names or c.checksum() != ck:
            bad.append(f"the trait loop != train {calls}: {names or 'checksum'}")
    legs["trait"] = legs.get("trait", 0) + 1
    if shard and N % 2 == 0:
        parts = []
        for off in (0, N // 2):
            with ra.Context(**dict(kw, n_envs=N // 2, env_offset=kw["env_offset"] + off)) as cs:
                start(cs)
                cs.train(K, want_stats=False)
                parts.append(full(cs))
        names = diff(join_shards(*parts), ref)
        if names:
            bad.append(f"two shards of {N // 2} joined != train({K}): {names}")
        legs["shard"] = legs.get("shard", 0) + 1
    return bad


def ckpt_leg(kw, rng, legs):
    bad = []
    k1, k2 = int(rng.integers(1, MAX_K)), int(rng.integers(1, MAX_K))
    with ra.Context(**kw) as a, ra.Context(**kw) as b, tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "cacla.ckpt")
        start(a)
        a.train(k1, want_stats=False)
        a.save_weights(path)
        b.load_weights(path)
        b.states, b.actions, b.episode_steps = a.states, a.actions, a.episode_steps
        if b.step_count != a.step_count or diff(full(b), full(a)) or a.checksum() != b.checksum():
            bad.append(f"the loaded ctx differs after train({k1})")
        a.train(k2, want_stats=False)
        b.train(k2, want_stats=False)
        names = diff(full(b), full(a))
        if names or a.checksum() != b.checksum():
            bad.append(f"{k2} steps after the load: {names or 'checksum'}")
    legs["ckpt"] = legs.get("ckpt", 0) + 1
    return bad


def run_case(seed, idx, legs):
    rng = case_rng(seed, idx)
    kw = sample(rng)
    tag = f"{idx:4d} ord {kw['order']} N {kw['n_envs']:3d} off {kw['env_offset']:10d} cap {kw['max_episode_steps']:3d} spl {kw['steps_per_launch']:2d} " \
          f"gamma {kw['gamma']} lr {kw['lr']} alpha {kw['alpha']}"
    try:
        c = ra.Context(**kw)
    except ra.RsrlHipError as e:
        return "refused", tag + f"  REFUSED: {str(e)[:90]}", kw
    with c:
        c.reset()
        bad = [f"handle: {b}" for b in handle_leg(c, kw, rng, legs)]
    bad += [f"train: {b}" for b in train_leg(kw, rng, legs, idx % 3 == 0)]
    if idx % 3 == 1:
        bad += [f"ckpt: {b}" for b in ckpt_leg(kw, rng, legs)]
    if bad:
        return "MISMATCH", tag + f"  MISMATCH {bad[:4]}", kw
    return "ok", tag + "  ok", kw


def main():
    pos = [a for a in sys.argv[1:] if "=" not in a]
    n_cases = int(pos[0]) if len(pos) > 0 else 200
    seed = int(pos[1]) if len(pos) > 1 else 0
    counts, failures, legs = {}, [], {}
    for idx in range(n_cases):
        try:
            status, line, kw = run_case(seed, idx, legs)
        except Exception as e:      # noqa: BLE001
            status, line, kw = "ERROR", f"{idx:4d} ERROR {type(e).__name__}: {str(e)[:200]}", None
        counts[status] = counts.get(status, 0) + 1
        print(line, flush=True)
        if status in ("MISMATCH", "ERROR"):
            failures.append({"case": idx, "line": line, "config": kw})
    print("SUMMARY " + json.dumps({"cases": n_cases, "seed": seed, "counts": counts, "legs": legs, "failures": failures}, default=str), flush=True)
    sys.exit(1 if failures else 0)


if __name__ == "__main__":
    main()
