#!/usr/bin/env python3
"""Random campaign over the gradient-TD prediction agents -- GTD2 (30), TDC (31) -- in the shape of tests/fuzz_episodic.py: every register-family
Fourier order at random learner counts (partial blocks), env offsets (ids that straddle 2^31, the top of the id range), discounts, rates in
[0, 0.05] (0 and 0.05 among them), episode caps (0: none; 1: every step ends an episode) and launch depths; horizons up to 60 batch-steps.  Legs:

    handle   learners given random theta and w (|.| <= 0.5) and a partial batch of M <= N transitions (domain_step's from random states, a quarter
             more flagged terminal), two calls in a row: td, theta and w of every learner bit for bit against tests/gtd_numpy.rule_f32; learners
             M .. N-1 keep every byte
    self     one uninterrupted train(K) against random splits with read-only calls between them (the checksum equal around each) and against two
             env_offset shards joined (even n_envs) -- bit for bit, the second column included
    td       the TD identity: RSRL_TDC with lr_td = 0 and w = 0 beside an RSRL_TD ctx of the same configuration after train(K) -- the weights equal
             as values, w still zero, states, actions, episode steps and the statistics identical; for a GTD2 case (and for TDC at its own rates)
             the environment side alone: states, actions, episode steps and the integer statistics are RSRL_TD's

    python tests/fuzz_gtd.py [n_cases=200] [seed=0] [agents=GTD2,TDC]      (GPU box; test infrastructure: imports oracle/)

One line per case and a SUMMARY {json} line (tests/campaign.run); exit code 1 on any mismatch."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rsrl_amd as ra  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import gtd_numpy as gn  # noqa: E402
from tests import campaign as cg  # noqa: E402
from tests.agent_contract import diff, join_shards, rand_states, snapshot  # noqa: E402
from tests.campaign import TOP_OF_IDS, bits, count  # noqa: E402

NAMES = {30: "GTD2", 31: "TDC"}
AGENTS = (30, 31)
REG = [(0, o) for o in (1, 2, 3, 4, 5)] + [(1, 1), (2, 1)]          # the register-family Fourier orders check_config admits for them
MAX_K = 60
SUITE_SEED, SUITE_CASES = 20261020, 30                              # the slice tests/test_gpu_gtd.py runs


def case_rng(seed, idx, agents=AGENTS):
    return cg.case_rng(seed, idx, agents[idx % len(agents)])


def sample(rng, idx=None, agents=AGENTS):
    algo = agents[idx % len(agents)] if idx is not None else int(rng.choice(agents))
    domain, order = REG[int(rng.integers(0, len(REG)))]
    kw = dict(domain=domain, order=order, algo=algo, policy=ra.RANDOM, seed=int(rng.integers(0, 1 << 20)), gamma=float(rng.choice([0.0, 0.9, 0.99, 1.0])),
              lr=float(rng.choice([0.0, 0.001, 0.02, 0.05])), lr_td=float(rng.choice([0.0, 0.005, 0.02, 0.05])),
              n_envs=int(rng.choice([1, 3, 5, 63, 64, 65, 130, 257])), env_offset=int(rng.choice([0, 64, 1000003, (1 << 31) - 65, TOP_OF_IDS])),
              max_episode_steps=int(rng.choice([0, 1, 2, 7, 25, 200])), steps_per_launch=int(rng.choice([0, 1, 5, 64])))
    return cg.top_of_ids(kw)


def columns(c):
    """(theta, w), each (N, F)"""
    return (np.stack([c.get_weights(i)[:, 0] for i in range(c.N)]), np.stack([c.get_td_weights(i)[:, 0] for i in range(c.N)]))


def full(c):
    out = snapshot(c)
    out["td_weights"] = np.stack([c.get_td_weights(i) for i in range(c.N)])
    return out


def handle_leg(c, kw, rng, legs):
    bad = []
    N, F, dom, order, al = c.N, c.F, kw["domain"], kw["order"], kw["algo"]
    th, w = rng.uniform(-0.5, 0.5, size=(N, F)).astype(np.float32), rng.uniform(-0.5, 0.5, size=(N, F)).astype(np.float32)
    for i in range(N):
        c.set_weights(th[i].reshape(F, 1), i)
        c.set_td_weights(w[i].reshape(F, 1), i)
    M = int(rng.integers(1, N + 1))
    for call in range(2):
        c.states = rand_states(orc, dom, N, rng)
        frm, nxt, rew, term = c.domain_step(rng.integers(0, c.A, size=N).astype(np.int32))
        term = (term | (rng.random(N) < 0.25)).astype(np.uint8)
        t0 = c.step_count
        td = c.handle(frm[:, :M], np.zeros(M, np.int32), rew[:M], nxt[:, :M], term[:M])
        if c.step_count != t0 + 1:
            bad.append("handle is not one batch-step")
        want_td, th[:M], w[:M] = gn.rule_f32(al, th[:M], w[:M], gn.project(orc, dom, order, frm[:, :M]), gn.project(orc, dom, order, nxt[:, :M]), rew[:M],
                                             term[:M] != 0, kw["gamma"], kw["lr"], kw["lr_td"])
        g_th, g_w = columns(c)
        if not np.array_equal(bits(td), bits(want_td)):
            bad.append(f"td of call {call} (M {M})")
        if not np.array_equal(bits(g_th[:M]), bits(th[:M])) or not np.array_equal(bits(g_w[:M]), bits(w[:M])):
            bad.append(f"theta or w of call {call} (M {M})")
        if not np.array_equal(bits(g_th[M:]), bits(th[M:])) or not np.array_equal(bits(g_w[M:]), bits(w[M:])):
            bad.append(f"a learner past M = {M} moved in call {call}")
    count(legs, "handle")
    return bad


def read_only_calls(c, rng, tmp):
    """this campaign's named calls, on its own draws, through tests/campaign.read_only_calls -> (findings, the calls made)"""
    N = c.N
    M = int(rng.integers(1, N + 1))
    S = rand_states(orc, c.cfg.domain, M, rng)
    i = int(rng.integers(0, N))
    calls = {"q_evaluate": lambda: c.q_evaluate(S), "get_weights": lambda: c.get_weights(i), "get_td_weights": lambda: c.get_td_weights(i),
             "checksum": lambda: c.checksum(), "policy_sample": lambda: c.policy_sample(S), "states": lambda: c.states, "actions": lambda: c.actions,
             "episode_steps": lambda: c.episode_steps, "project": lambda: c.project(S), "q_find_max": lambda: c.q_find_max(S),
             "get_traces": lambda: c.get_traces(i), "save_weights": lambda: c.save_weights(os.path.join(tmp, "q.ckpt"))}
    return cg.read_only_calls(c, rng, calls)


def self_leg(kw, rng, legs):
    bad, made = [], []
    N = kw["n_envs"]
    K = int(rng.choice([10, 25, 40, MAX_K]))
    ref = cg.reference_run(kw, K, full)
    if not (np.isfinite(ref[0]["weights"]).all() and np.isfinite(ref[0]["td_weights"]).all()):
        return bad, f"train({K}) left a non-finite column"
    with tempfile.TemporaryDirectory() as td:
        def between(c):
            b_, m_ = read_only_calls(c, rng, td)
            bad.extend(b_); made.extend(m_)
        got, calls = cg.split_run(kw, rng, K, cg.draw_calls(rng, K, 1, 4), full, between=between)
    names = cg.differs(got, ref)
    if names:
        bad.append(f"train {calls} with {made} != train({K}): {names}")
    count(legs, "split+query")
    if N % 2 == 0:
        names = diff(join_shards(*cg.shard_run(kw, K, (N // 2, N // 2), full)), ref[0])
        if names:
            bad.append(f"two shards of {N // 2} joined != train({K}): {names}")
        count(legs, "shard")
    return bad, None


def td_leg(kw, rng, legs):
    K = int(rng.integers(1, MAX_K + 1))
    td_kw = dict(kw, algo=ra.TD, lr_td=0.0)
    bad = cg.env_side(kw, td_kw, K)                                  # the environment side at the case's own rates
    count(legs, "env")
    # TDC without its estimator is TD
    with ra.Context(**dict(kw, algo=ra.TDC, lr_td=0.0)) as c, ra.Context(**td_kw) as t:
        c.reset()
        t.reset()
        sc, stt = c.train(K), t.train(K)
        th, w = columns(c)
        tw = np.stack([t.get_weights(i)[:, 0] for i in range(t.N)])
        if np.isfinite(tw).all():
            if not np.array_equal(th, tw):
                bad.append(f"TDC(lr_td = 0, w = 0) weights after train({K}) != RSRL_TD's")
            if w.any():
                bad.append("w moved at lr_td = 0")
            if sc != stt:
                bad.append(f"statistics {sc} != RSRL_TD's {stt}")
        for name in ("states", "actions", "episode_steps"):
            if not np.array_equal(getattr(c, name).view(np.uint32), getattr(t, name).view(np.uint32)):
                bad.append(f"TDC(lr_td = 0): {name} after train({K}) != RSRL_TD's")
    count(legs, "identity")
    return bad


def run_case(seed, idx, agents, legs):
    rng = case_rng(seed, idx, agents)
    kw = sample(rng, idx, agents)
    al = kw["algo"]
    tag = f"{idx:4d} {NAMES[al]:5s} dom {kw['domain']} ord {kw['order']} N {kw['n_envs']:3d} off {kw['env_offset']:10d} cap {kw['max_episode_steps']:3d} " \
          f"spl {kw['steps_per_launch']:2d} gamma {kw['gamma']} lr {kw['lr']} lr_td {kw['lr_td']}"
    c, refused = cg.create(tag, kw)
    if refused:
        return refused
    with c:
        c.reset()
        bad = [f"handle: {b}" for b in handle_leg(c, kw, rng, legs)]
    b_, why = self_leg(kw, rng, legs)
    bad += [f"self: {b}" for b in b_]
    bad += [f"td: {b}" for b in td_leg(kw, rng, legs)]
    return cg.verdict(tag, kw, bad, why)


def main():
    n_cases, seed = cg.parse_cases(sys.argv[1:])
    agents = cg.parse_agents(sys.argv[1:], NAMES) or AGENTS
    legs = {}
    cg.run(lambda idx: run_case(seed, idx, agents, legs), n_cases, seed, NAMES, lambda failures: {"legs": legs})


if __name__ == "__main__":
    main()
