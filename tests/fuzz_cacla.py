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

One line per case and a SUMMARY {json} line (tests/campaign.run); exit code 1 on any mismatch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rsrl_amd as ra  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import cacla_numpy as cn  # noqa: E402
from tests import campaign as cg  # noqa: E402
from tests.agent_contract import diff, join_shards, snapshot, trait_loop  # noqa: E402
from tests.campaign import TOP_OF_IDS, bits, count  # noqa: E402

MAX_K = 24
SUITE_SEED, SUITE_CASES = 20261020, 150                              # the slice tests/test_gpu_cacla.py runs


def case_rng(seed, idx):
    return cg.case_rng(seed, idx, cn.CACLA)


def sample(rng):
    kw = dict(domain=ra.CONTINUOUS_MOUNTAIN_CAR, order=int(rng.integers(1, 6)), algo=ra.CACLA, policy=ra.GAUSSIAN, seed=int(rng.integers(0, 1 << 20)),
              gamma=float(rng.choice([0.0, 0.9, 0.99, 1.0])), lr=float(rng.choice([0.0, 0.001, 0.02, 0.05])), alpha=float(rng.choice([0.0, 0.001, 0.01])),
              n_envs=int(rng.choice([1, 2, 5, 63, 64, 66, 130])), env_offset=int(rng.choice([0, 64, 1000003, (1 << 31) - 33, TOP_OF_IDS])),
              max_episode_steps=int(rng.choice([0, 1, 2, 7, 25])), steps_per_launch=int(rng.choice([0, 1, 5, 64])))
    return cg.top_of_ids(kw)


def full(c):
    """tests/agent_contract.snapshot and the policy's columns"""
    out = snapshot(c)
    out["theta"] = np.stack([c.get_policy_weights(i) for i in range(c.N)])
    return out


def start(c, off=0):
    """reset, then every third learner (by global id, so a shard needs no `off`) near the goal, so that terminal ends occur as well as cut ones,
    and every second one with V = -40 everywhere (the constant feature is the last one): from w = 0 and rewards of -1 no gate opens within
    such short horizons"""
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
    count(legs, "handle")
    return bad


def train_leg(kw, rng, legs, shard):
    bad = []
    N, cap = kw["n_envs"], kw["max_episode_steps"]
    K = int(rng.integers(2, MAX_K + 1))
    ref, calls = cg.split_run(kw, rng, K, cg.draw_calls(rng, K, 0, 3), full, start)
    names = cg.differs(cg.trait_run(dict(kw, steps_per_launch=0), K, cap, trait_loop, full, start), ref)
    if names:
        bad.append(f"the trait loop != train {calls}: {names}")
    count(legs, "trait")
    if shard and N % 2 == 0:
        names = diff(join_shards(*cg.shard_run(kw, K, (N // 2, N // 2), full, start)), ref[0])
        if names:
            bad.append(f"two shards of {N // 2} joined != train({K}): {names}")
        count(legs, "shard")
    return bad


def ckpt_leg(kw, rng, legs):
    k1, k2 = int(rng.integers(1, MAX_K)), int(rng.integers(1, MAX_K))
    bad = cg.twin_resume(kw, k1, k2, full, start)
    count(legs, "ckpt")
    return bad


def run_case(seed, idx, legs):
    rng = case_rng(seed, idx)
    kw = sample(rng)
    tag = f"{idx:4d} ord {kw['order']} N {kw['n_envs']:3d} off {kw['env_offset']:10d} cap {kw['max_episode_steps']:3d} spl {kw['steps_per_launch']:2d} " \
          f"gamma {kw['gamma']} lr {kw['lr']} alpha {kw['alpha']}"
    c, refused = cg.create(tag, kw)
    if refused:
        return refused
    with c:
        c.reset()
        bad = [f"handle: {b}" for b in handle_leg(c, kw, rng, legs)]
    bad += [f"train: {b}" for b in train_leg(kw, rng, legs, idx % 3 == 0)]
    if idx % 3 == 1:
        bad += [f"ckpt: {b}" for b in ckpt_leg(kw, rng, legs)]
    return cg.verdict(tag, kw, bad)


def main():
    n_cases, seed = cg.parse_cases(sys.argv[1:])
    legs = {}
    cg.run(lambda idx: run_case(seed, idx, legs), n_cases, seed, extras=lambda failures: {"legs": legs})


if __name__ == "__main__":
    main()
