#!/usr/bin/env python3
"""Random campaign over the continuous TD ActorCritic (35) on ContinuousMountainCar with the Gaussian and the Beta policy, on tests/fuzz_cacla.py's
pattern: the Fourier orders 1-5 at random learner counts 1..257 (partial blocks), seeds, env offsets (ids that straddle 2^31, the top of the id
range), discounts, rates, episode caps (0: none; 1: every step ends an episode), launch depths and shards; horizons up to 24 batch-steps.  Legs:

    f64      learners given random w and columns as tests/tdac_cont_numpy.handle_case builds them (a target preference on the constant feature, up
             to 12, plus a small random part) and a partial batch of M <= N transitions, two calls in a row: td and w bit for bit against
             tests/cacla_numpy.td_gate_f32 (the oracle's device-order projection), every learner past M byte for byte as it was, the first M
             learners' columns against tests/tdac_cont_numpy.handle in f64 on the device's own projection within F64_BOUND; alpha = 0 leaves every
             column's value alone
    self     train(K), cut into one to three calls, against the host trait loop (domain_step(NULL) -> handle -> domain_reset(ended) ->
             policy_sample(NULL)) -- w, both columns, states, actions and episode steps bit for bit; every third case also against two env_offset
             shards joined, every third a checkpoint resumed in a fresh ctx

    python tests/fuzz_tdac_cont.py [n_cases=200] [seed=0]      (GPU box; test infrastructure: imports oracle/)

One line per case and a SUMMARY {json} line (tests/campaign.run; with the largest f64 figure met); exit code 1 on any mismatch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rsrl_amd as ra  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import cacla_numpy as cn  # noqa: E402
from tests import tdac_cont_numpy as tn  # noqa: E402
from tests import campaign as cg  # noqa: E402
from tests.agent_contract import diff, join_shards, snapshot  # noqa: E402
from tests.campaign import TOP_OF_IDS, bits, count  # noqa: E402

MAX_K = 24
SUITE_SEED, SUITE_CASES = 20261020, 24                               # the slice tests/test_gpu_tdac_cont.py runs
# max |d column| / max(1, |column|) of one handle call against f64: four times the largest figure profiles/tdac_cont_rate.md records for the rule
# test's inputs (three calls in a row, the same construction of columns and actions) over both policies and the orders 1-5
F64_BOUND = 4 * 1.443e-7


def case_rng(seed, idx):
    return cg.case_rng(seed, idx, tn.TDAC_CONT)


def sample(rng):
    kw = dict(domain=ra.CONTINUOUS_MOUNTAIN_CAR, order=int(rng.integers(1, 6)), algo=ra.CONTINUOUS_TD_ACTOR_CRITIC, policy=int(rng.choice([ra.GAUSSIAN, ra.BETA])),
              seed=int(rng.integers(0, 1 << 20)), gamma=float(rng.choice([0.0, 0.9, 0.99, 1.0])), lr=float(rng.choice([0.0, 0.001, 0.02, 0.05])),
              alpha=float(rng.choice([0.0, 0.001, 0.01])), n_envs=int(rng.choice([1, 2, 5, 63, 64, 66, 130, 257])),
              env_offset=int(rng.choice([0, 64, 1000003, (1 << 31) - 33, TOP_OF_IDS])), max_episode_steps=int(rng.choice([0, 1, 7, 23, 200])),
              steps_per_launch=int(rng.choice([0, 1, 5, 64])))
    return cg.top_of_ids(kw)


def full(c):
    """tests/agent_contract.snapshot and the policy's columns"""
    out = snapshot(c)
    out["theta"] = np.stack([c.get_policy_weights(i) for i in range(c.N)])
    return out


def start(c, off=0):
    """reset, then every third learner (by global id, so a shard needs no `off`) near the goal, so that terminal ends occur as well as cut ones"""
    c.reset()
    ids = np.arange(c.N) + c.cfg.env_offset
    s = c.states
    s[:, ids % 3 == 0] = np.array([[0.59], [0.06]], dtype=np.float32)
    c.states = s


def trait_loop(c, K, cap):
    """tests/agent_contract.trait_loop with the PENDING actions stepped on (domain_step(NULL): each policy's loop convention, 2a - 1 under Beta)"""
    ep = c.episode_steps.astype(np.int64)
    for _ in range(K):
        a = c.actions
        frm, nxt, rew, term = c.domain_step()
        c.handle(frm, a, rew, nxt, term)
        ep += 1
        mask = (term.astype(bool) | ((ep >= cap) if cap > 0 else False)).astype(np.uint8)
        c.domain_reset(mask)
        ep[mask == 1] = 0
        c.policy_sample()
    c.episode_steps = ep.astype(np.uint32)


def project(order, S):
    return np.stack([orc.fourier_project(orc.MOUNTAIN_CAR, order, S[:, i], "f32d") for i in range(S.shape[1])]).astype(np.float32)


def f64_leg(c, kw, rng, legs):
    bad = []
    N, F, order, policy = c.N, c.F, kw["order"], kw["policy"]
    w = rng.normal(size=(N, F))
    w = (w * rng.uniform(0.5, 3.0, size=(N, 1)) / np.abs(w).sum(axis=1, keepdims=True)).astype(np.float32)      # sum |w| <= 3, as handle_case's
    W = rng.normal(size=(N, F, 2))
    W[:, F - 1] = 0.0
    W *= rng.uniform(0.1, 0.4, size=(N, 1, 2)) / np.abs(W).sum(axis=1, keepdims=True)
    if policy == ra.GAUSSIAN:
        W[:, F - 1, 0], W[:, F - 1, 1] = rng.uniform(-1.0, 1.0, size=N), np.where(rng.random(N) < 0.15, rng.uniform(10.5, 12.0, size=N), rng.uniform(-2.0, 8.0, size=N))
    else:
        W[:, F - 1] = np.where(rng.random((N, 2)) < 0.15, rng.uniform(10.5, 12.0, size=(N, 2)), rng.uniform(-8.0, 8.0, size=(N, 2)))
    W = W.astype(np.float32)
    for i in range(N):
        c.set_weights(w[i].reshape(F, 1), i)
        c.set_policy_weights(W[i], i)
    M = int(rng.integers(1, N + 1))
    lo, hi = orc.domain_bounds(orc.MOUNTAIN_CAR)
    worst = 0.0
    for call in range(2):
        S = rng.uniform(lo, hi, size=(N, 2)).T.astype(np.float32)
        c.states = S
        if policy == ra.GAUSSIAN:                                                # on both sides of the mean, |a - mu| <= 2 sd
            mu, sd = c.policy_params(S)
            z = rng.uniform(0.3, 2.0, size=N) * np.where(rng.random(N) < 0.5, -1.0, 1.0)
            a = (mu.astype(np.float64) + sd.astype(np.float64) * z).astype(np.float32)
        else:
            a = rng.uniform(tn.A_LO, tn.A_HI, size=N).astype(np.float32)
        frm, nxt, rew, term = c.domain_step(a)
        term = (term | (rng.random(N) < 0.25)).astype(np.uint8)
        rew = (rew + rng.uniform(-1.0, 2.0, size=N)).astype(np.float32)          # handle takes any reward: both signs of c occur
        t0 = c.step_count
        phi_s, phi_n = c.project(frm[:, :M]), c.project(nxt[:, :M])
        td = c.handle(frm[:, :M], a[:M], rew[:M], nxt[:, :M], term[:M])
        if c.step_count != t0 + 1:
            bad.append("handle is not one batch-step")
        want_td, w2, _, _, _ = cn.td_gate_f32(w[:M], project(order, frm[:, :M]), project(order, nxt[:, :M]), rew[:M], term[:M] != 0, kw["gamma"], kw["lr"])
        g_w = np.stack([c.get_weights(i)[:, 0] for i in range(N)])
        g_W = np.stack([c.get_policy_weights(i) for i in range(N)])
        want_W = np.stack([tn.handle(policy, w[i], W[i], phi_s[:, i], phi_n[:, i], float(a[i]), float(rew[i]), bool(term[i]), float(np.float32(kw["gamma"])),
                                     float(np.float32(kw["lr"])), kw["alpha"])[2] for i in range(M)])
        w[:M] = w2
        if not np.array_equal(bits(td), bits(want_td)):
            bad.append(f"td of call {call} (M {M})")
        if not np.array_equal(bits(g_w), bits(w)):
            bad.append(f"w of call {call} (M {M})")
        if not all(g_W[i].tobytes() == W[i].tobytes() for i in range(M, N)):
            bad.append(f"a learner past M = {M} moved in call {call}")
        fig = float(np.max(np.abs(g_W[:M].astype(np.float64) - want_W) / np.maximum(1.0, np.abs(want_W))))
        worst = max(worst, fig) if np.isfinite(fig) else np.inf
        if not fig <= F64_BOUND:
            bad.append(f"columns of call {call} against f64: {fig:.4g} > {F64_BOUND:.4g}")
        if kw["alpha"] > 0 and all(g_W[i].tobytes() == W[i].tobytes() for i in range(M)):
            bad.append(f"no learner's columns moved in call {call}")
        if kw["alpha"] == 0 and not np.array_equal(g_W, W):                      # (e = 0: fma(0, phi, w) is w as a value)
            bad.append(f"alpha = 0 moved a column in call {call}")
        W = g_W
    count(legs, "f64")
    legs["f64_max"] = max(legs.get("f64_max", 0.0), worst)
    return bad


def self_leg(kw, rng, legs, shard, ckpt):
    bad = []
    N, cap = kw["n_envs"], kw["max_episode_steps"]
    K = int(rng.integers(2, MAX_K + 1))
    ref, calls = cg.split_run(kw, rng, K, cg.draw_calls(rng, K, 0, 3), full, start)
    names = cg.differs(cg.trait_run(dict(kw, steps_per_launch=0), K, cap, trait_loop, full, start), ref)
    if names:
        bad.append(f"the trait loop != train {calls}: {names}")
    count(legs, "self")
    if shard and N % 2 == 0:
        names = diff(join_shards(*cg.shard_run(kw, K, (N // 2, N // 2), full, start)), ref[0])
        if names:
            bad.append(f"two shards of {N // 2} joined != train({K}): {names}")
        count(legs, "shard")
    if ckpt:
        k1, k2 = int(rng.integers(1, MAX_K)), int(rng.integers(1, MAX_K))
        bad += cg.twin_resume(kw, k1, k2, full, start)
        count(legs, "ckpt")
    return bad


def run_case(seed, idx, legs):
    rng = case_rng(seed, idx)
    kw = sample(rng)
    tag = f"{idx:4d} pol {kw['policy']} ord {kw['order']} N {kw['n_envs']:3d} off {kw['env_offset']:10d} cap {kw['max_episode_steps']:3d} spl {kw['steps_per_launch']:2d} " \
          f"gamma {kw['gamma']} lr {kw['lr']} alpha {kw['alpha']}"
    c, refused = cg.create(tag, kw)
    if refused:
        return refused
    with c:
        c.reset()
        bad = [f"f64: {b}" for b in f64_leg(c, kw, rng, legs)]
    bad += [f"self: {b}" for b in self_leg(kw, rng, legs, idx % 3 == 0, idx % 3 == 1)]
    return cg.verdict(tag, kw, bad)


def main():
    n_cases, seed = cg.parse_cases(sys.argv[1:])
    legs = {}
    cg.run(lambda idx: run_case(seed, idx, legs), n_cases, seed, extras=lambda failures: {"legs": legs})


if __name__ == "__main__":
    main()
