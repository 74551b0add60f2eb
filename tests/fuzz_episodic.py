#!/usr/bin/env python3
"""Random campaign over the agents that keep a per-learner episode record -- GradientMC (23), LSTD (25), LSTDLambda (26) -- in the style of
tests/fuzz_agents.py: every register-family Fourier order at random learner counts (idle and ragged lane groups of 4 / 16 / 64 lanes), env offsets
(ids that straddle 2^31, the top of the id range), discounts, lambdas, step sizes, episode caps (1: every step ends an episode; 200 above the horizon:
the record never closes) and launch depths.  Neither LSTD agent reads a batch or solve-interval field of the config (check_reg_only: n_steps is not
read for 25 / 26; they solve at every episode end), so there is none to draw.  Legs:

    batch    GradientMC: handle_batch on a random T in [1, cap] with ragged lengths (0 and T among them) for learners given random weights --
             returns and weights bit for bit against tests/gmc_numpy.td_chain(..., "f32d").  LSTD / LSTDLambda: handle_transitions with ragged
             lengths and random terminal flags from random pre-set theta / A / b / z / singular counter -- A, b, z against
             tests/lstd_batch_numpy.handle at tests/test_gpu_lstd_batch.py's bound, theta bit for bit against lu_solve of the device's own A and
             b, after the call and after lstd_solve, the singular counter exactly; one case in four plants a crafted matrix (permuted triangular,
             equal first-column magnitudes, two equal rows) in a learner the call does not name.  Learners with length 0 keep every byte, and
             nobody's open record or episode_steps moves
    self     one uninterrupted train(K) against random splits with read-only calls between them (the checksum equal around each), the host
             trait loop, two env_offset shards joined (even n_envs), a checkpoint saved at a random step and resumed with the caller carrying
             states, actions, episode_steps and the record -- bit for bit, the f64 state and the record in the snapshot
    env      the same seed, N, cap and domain under RSRL_TD: states, actions, episode_steps and the integer statistics bit-equal

    python tests/fuzz_episodic.py [n_cases=200] [seed=0] [agents=GradientMC,LSTD,LSTDLambda]      (GPU box; test infrastructure: imports oracle/)

Case idx draws everything from case_rng(seed, idx, agents) -- the host inputs of its batch leg first -- so that a case's inputs can be rebuilt without
a device (tests/test_fuzz_late_cpu.py).  An LSTD case whose f64 accumulators are not finite is counted as `diverged`, with the reason printed.
One line per case and a SUMMARY {json} line (tests/campaign.run); exit code 1 on any mismatch."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rsrl_amd as ra  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import campaign as cg  # noqa: E402
from tests.agent_contract import diff, gmc_trait_loop, join_shards, learner_state, lstd_batch_trait_loop, rand_states, record_bits, snapshot  # noqa: E402
from tests.campaign import TOP_OF_IDS, bits, count  # noqa: E402
from tests.gmc_numpy import td_chain  # noqa: E402
from tests.lstd_batch_numpy import handle, lu_solve, state_of  # noqa: E402
from tests.test_gpu_lstd_batch import crafted  # noqa: E402

NAMES = {23: "GradientMC", 25: "LSTD", 26: "LSTDLambda"}
AGENTS = (23, 25, 26)
REG = [(0, o) for o in (1, 2, 3, 4, 5)] + [(1, 1), (2, 1)]          # the register-family Fourier orders check_config admits for them
N_DIM = {0: 2, 1: 4, 2: 4}
EPS64 = np.finfo(np.float64).eps
MAX_K = 60           # horizon of the self and env legs, batch-steps
MAX_T_LSTD = 12      # rows of the LSTD batch leg (the restatement is Python loops over F^2 per row)
REPLAYED = 8
SUITE_SEED, SUITE_CASES = 20261020, 24      # the slice tests/test_gpu_fuzz.py runs per agent (tests/test_fuzz_late_cpu.py checks its shares on the CPU)


def case_rng(seed, idx, agents=AGENTS):
    """case idx's generator: keyed by the seed, the case and its agent, so that an agent's slice is not another's with the algo swapped"""
    return cg.case_rng(seed, idx, agents[idx % len(agents)])


def sample(rng, idx=None, agents=AGENTS):
    """-> device kwargs of one configuration (case idx: the agents in turn)"""
    algo = agents[idx % len(agents)] if idx is not None else int(rng.choice(agents))
    domain, order = REG[int(rng.integers(0, len(REG)))]
    F = (order + 1) ** N_DIM[domain]
    kw = dict(domain=domain, order=order, algo=algo, policy=ra.RANDOM, seed=int(rng.integers(0, 1 << 20)), gamma=float(rng.choice([0.0, 0.9, 0.99, 1.0])),
              lam=float(rng.choice([0.0, 0.5, 0.8, 1.0])), lr=float(rng.choice([0.02, 0.2])) / F,
              n_envs=int(rng.choice([1, 3, 5, 63, 64, 65, 130, 257])), env_offset=int(rng.choice([0, 64, 1000003, (1 << 31) - 65, TOP_OF_IDS])),
              max_episode_steps=int(rng.choice([1, 2, 7, 25, 200])), steps_per_launch=int(rng.choice([0, 1, 5, 64])))
    return cg.top_of_ids(kw)


def batch_inputs(rng, kw):
    """the host side of the batch leg, no device: the arrays handed to handle_batch / handle_transitions, the learners' pre-set state, the
    learners replayed and the steps trained before the call (so that the ctx holds open records the call must not touch)"""
    N, cap, dom, al = kw["n_envs"], kw["max_episode_steps"], kw["domain"], kw["algo"]
    F = (kw["order"] + 1) ** N_DIM[dom]
    T = int(rng.integers(1, (cap if al == 23 else min(cap, MAX_T_LSTD)) + 1))
    io = dict(T=T, F=F, k0=int(rng.integers(0, 6)), S=np.stack([rand_states(orc, dom, N, rng) for _ in range(T)]), R=rng.normal(0.0, 1.0, size=(T, N)).astype(np.float32))
    rep = sorted(set([0, N - 1] + [int(x) for x in rng.integers(0, N, size=REPLAYED - 2)]))
    L = rng.integers(0, T + 1, size=N).astype(np.uint32)
    L[rep[0]], L[rep[-1]] = 0, T                                    # (an empty batch and a full one among the replayed learners; N = 1: the full one)
    if al == 23:
        io["W"] = rng.normal(0.0, 0.3, size=(N, F)).astype(np.float32)
    else:
        io["S2"] = np.stack([rand_states(orc, dom, N, rng) for _ in range(T)])
        io["Tm"] = (rng.random((T, N)) < 0.3).astype(np.uint8)
        io["init"] = [[rng.normal(0.0, 0.5, size=F), np.eye(F) + 0.1 * rng.normal(0.0, 1.0, size=(F, F)) / np.sqrt(F), rng.normal(0.0, 1.0, size=F),
                       rng.normal(0.0, 1.0, size=F), int(rng.integers(0, 4))] for _ in range(N)]
        io["planted"] = None
        if rng.integers(0, 4) == 0:
            j, kind = int(rng.integers(0, N)), int(rng.integers(1, 4))
            io["init"][j][1], io["init"][j][2] = crafted(F, kind, rng)
            L[j] = 0                                                # (not named by the call: lstd_solve meets the crafted matrix itself)
            io["planted"] = (j, kind)
            rep = sorted(set(rep + [j]))
    io["L"], io["rep"] = L, rep
    return io


def lstd_replay(kw, io, i):
    """learner i's batch through the restatement -> (its state dict after handle, the diagnostics)"""
    dom, order, n = kw["domain"], kw["order"], int(io["L"][i])
    theta, A, b, z, sing = io["init"][i]
    lam = kw["lam"] if kw["algo"] == 26 else None
    st = state_of(theta, A, b, z if lam is not None else None, sing)
    rows = [(orc.fourier_project(dom, order, io["S"][k, :, i]), orc.fourier_project(dom, order, io["S2"][k, :, i]), float(io["R"][k, i]), bool(io["Tm"][k, i]))
            for k in range(n)]
    return st, handle(st, rows, kw["gamma"], lam)


def finite_state(st):
    return all(np.isfinite(np.asarray(st[k], dtype=np.float64)).all() for k in ("theta", "A", "b") + (("z",) if "z" in st else ()))


def full(c, learners=None):
    out = snapshot(c, learners)
    out.update(record_bits(c))
    return out


def batch_leg_gmc(c, kw, io, worst):
    bad = []
    N, T, L, rep = c.N, io["T"], io["L"], io["rep"]
    c.train(io["k0"], want_stats=False)
    for i in range(N):
        c.set_weights(io["W"][i].reshape(c.F, 1), i)
    rec0, ep0, t0 = record_bits(c), c.episode_steps, c.step_count
    ret = c.handle_batch(io["S"], None, io["R"], L, returns=True)
    if c.step_count != t0 + 1:
        bad.append("handle_batch is not one batch-step")
    got = np.stack([c.get_weights(i)[:, 0] for i in range(N)])
    idle = L == 0
    if not np.array_equal(bits(got[idle]), bits(io["W"][idle])) or not np.isnan(ret[:, idle]).all():
        bad.append("a learner with length 0 moved")
    if diff(record_bits(c), rec0) or not np.array_equal(c.episode_steps, ep0):
        bad.append("the open record or episode_steps moved")
    ag = orc.make_agent(domain=kw["domain"], order=kw["order"], algo=orc.TD, policy=orc.RANDOM, gamma=kw["gamma"], lr=kw["lr"])
    for i in rep:
        n = int(L[i])
        w = io["W"][i].copy()
        _, rets = td_chain(orc, ag, w, io["S"][:n, :, i], io["R"][:n, i], kw["gamma"], "f32d")
        if not np.array_equal(bits(ret[:n, i]), bits(rets)) or not np.isnan(ret[n:, i]).all():
            bad.append(f"returns of learner {i} (length {n} of {T})")
        if not np.array_equal(bits(got[i]), bits(w)):
            bad.append(f"weights of learner {i} (length {n} of {T})")
        count(worst, "replayed")
    return bad


def batch_leg_lstd(c, kw, io, worst):
    bad = []
    N, T, L, rep, F = c.N, io["T"], io["L"], io["rep"], c.F
    lam = kw["algo"] == 26
    c.train(io["k0"], want_stats=False)
    for i, (theta, A, b, z, sing) in enumerate(io["init"]):
        c.set_lstd_batch_state(theta, A, b, z if lam else None, sing, i)
    rec0, ep0, t0 = record_bits(c), c.episode_steps, c.step_count
    idle = [int(i) for i in np.flatnonzero(L == 0)]
    before = {i: learner_state(c, i) for i in idle}
    td = c.handle_transitions(io["S"], io["R"], io["S2"], io["Tm"], L, td=True)
    if c.step_count != t0 + 1:
        bad.append("handle_transitions is not one batch-step")
    if any(diff(learner_state(c, i), before[i]) for i in idle) or not np.isnan(td[:, idle]).all():
        bad.append("a learner with length 0 moved")
    if diff(record_bits(c), rec0) or not np.array_equal(c.episode_steps, ep0):
        bad.append("the open record or episode_steps moved")
    tol = 16.0 * F * T * EPS64                                      # tests/test_gpu_lstd_batch.py: 16 F eps per step relative to the state's magnitude
    after = {i: c.get_lstd_batch_state(i) for i in rep}
    c.lstd_solve()
    for i in rep:
        n = int(L[i])
        g_theta, g_A, g_b, g_z, g_sing = after[i]
        s_theta, s_A, s_b, s_z, s_sing = c.get_lstd_batch_state(i)
        sing0 = io["init"][i][4]
        if s_A.tobytes() != g_A.tobytes() or s_b.tobytes() != g_b.tobytes() or (lam and s_z.tobytes() != g_z.tobytes()):
            bad.append(f"lstd_solve moved A, b or z of learner {i}")
        x = lu_solve(g_A, g_b)
        s = int(x is None)
        if n > 0:
            st, want_td = lstd_replay(kw, io, i)
            if not finite_state(st):
                return bad, f"learner {i}: the f64 accumulators of the restatement are not finite"
            for name, g, key in (("A", g_A, "A"), ("b", g_b, "b")) + ((("z", g_z, "z"),) if lam else ()):
                w = np.array(st[key])
                frac = float(np.max(np.abs(g - w))) / (tol * (1.0 + float(np.max(np.abs(w)))))
                worst[name] = max(worst.get(name, 0.0), frac)
                if not frac <= 1.0:
                    bad.append(f"{name} of learner {i}: {frac:.3g} of the bound (T {T}, length {n})")
            for k in range(n):
                e = abs(float(td[k, i]) - want_td[k]) / (2.0 ** -22 * (1.0 + abs(want_td[k])))
                worst["td"] = max(worst.get("td", 0.0), e)
                if not e <= 1.0:
                    bad.append(f"td[{k}] of learner {i}: {e:.3g} of the bound")
            if not np.isnan(td[n:, i]).all():
                bad.append(f"td past the length of learner {i}")
            want_theta = io["init"][i][0] if x is None else np.array(x)
            if g_theta.tobytes() != np.asarray(want_theta, dtype=np.float64).tobytes() or g_sing != sing0 + s:
                bad.append(f"handle_transitions' solve of learner {i} (singular {g_sing}, want {sing0 + s})")
        want_theta = g_theta if x is None else np.array(x)
        if s_theta.tobytes() != np.asarray(want_theta, dtype=np.float64).tobytes() or s_sing != g_sing + s:
            bad.append(f"lstd_solve of learner {i}{' (planted kind %d)' % io['planted'][1] if io['planted'] and io['planted'][0] == i else ''}: "
                       f"singular {s_sing}, want {g_sing + s}")
        count(worst, "replayed")
    if io["planted"] and io["planted"][1] == 3 and F > 1 and c.get_lstd_batch_state(io["planted"][0])[4] != io["init"][io["planted"][0]][4] + 1:
        bad.append("two equal rows were not counted as an abandoned solve")
    return bad, None


def read_only_calls(c, rng, tmp):
    """this campaign's named calls, on its own draws, through tests/campaign.read_only_calls -> (findings, the calls made)"""
    N = c.N
    M = int(rng.integers(1, N + 1))
    S = rand_states(orc, c.cfg.domain, M, rng)
    i = int(rng.integers(0, N))
    calls = {"q_evaluate": lambda: c.q_evaluate(S), "get_weights": lambda: c.get_weights(i), "episode_record": lambda: c.episode_record,
             "checksum": lambda: c.checksum(), "policy_sample": lambda: c.policy_sample(S), "states": lambda: c.states, "actions": lambda: c.actions,
             "episode_steps": lambda: c.episode_steps, "project": lambda: c.project(S), "save_weights": lambda: c.save_weights(os.path.join(tmp, "q.ckpt"))}
    if c.cfg.algo in (25, 26):
        calls["get_lstd_batch_state"] = lambda: c.get_lstd_batch_state(i)
    return cg.read_only_calls(c, rng, calls)


def self_leg(kw, rng, legs):
    """-> (findings, the reason the case diverged or None)"""
    bad, made = [], []
    N, cap, al = kw["n_envs"], kw["max_episode_steps"], kw["algo"]
    K = int(rng.choice([10, 25, 40, MAX_K]))
    ref = cg.reference_run(kw, K, full)
    if al != 23 and not all(np.isfinite(ref[0][n]).all() for n in ("lstd_theta", "lstd_A", "lstd_b")):
        return bad, f"train({K}) left a non-finite f64 state"
    with tempfile.TemporaryDirectory() as td:
        def between(c):
            b_, m_ = read_only_calls(c, rng, td)
            bad.extend(b_); made.extend(m_)
        got, calls = cg.split_run(kw, rng, K, cg.draw_calls(rng, K, 1, 4), full, between=between)
    names = cg.differs(got, ref)
    if names:
        bad.append(f"train {calls} with {made} != train({K}): {names}")
    count(legs, "split+query")
    names = cg.differs(cg.trait_run(kw, K, cap, gmc_trait_loop if al == 23 else lstd_batch_trait_loop, full), ref, checksum=False)
    if names:
        bad.append(f"the host trait loop != train({K}): {names}")
    count(legs, "trait")
    if N % 2 == 0:
        names = diff(join_shards(*cg.shard_run(kw, K, (N // 2, N // 2), full)), ref[0])
        if names:
            bad.append(f"two shards of {N // 2} joined != train({K}): {names}")
        count(legs, "shard")
    k1 = int(rng.integers(1, K))

    def carry(a, b):
        b.episode_record = a.episode_record
    names = cg.differs(cg.resume_run(kw, K, k1, full, carry=carry), ref)
    if names:
        bad.append(f"checkpoint at {k1} resumed != train({K}): {names}")
    count(legs, "ckpt")
    return bad, None


def env_leg(kw, rng, legs):
    """tests/test_gpu_gmc.py test_environment_side_is_tds, randomised: both agents sample Random on the same draws"""
    bad = cg.env_side(kw, dict(kw, algo=ra.TD, lr=0.01), int(rng.integers(1, MAX_K + 1)))
    count(legs, "env")
    return bad


def run_case(seed, idx, agents, worst, legs):
    rng = case_rng(seed, idx, agents)
    kw = sample(rng, idx, agents)
    al = kw["algo"]
    io = batch_inputs(rng, kw)
    tag = f"{idx:4d} {NAMES[al]:10s} dom {kw['domain']} ord {kw['order']} N {kw['n_envs']:3d} off {kw['env_offset']:10d} cap {kw['max_episode_steps']:3d} " \
          f"spl {kw['steps_per_launch']:2d} gamma {kw['gamma']} lam {kw['lam']} T {io['T']:3d}"
    c, refused = cg.create(tag, kw)
    if refused:
        return refused
    bad, why = [], None
    with c:
        c.reset()
        w = worst.setdefault(NAMES[al], {})
        if al == 23:
            bad += [f"batch: {b}" for b in batch_leg_gmc(c, kw, io, w)]
        else:
            b_, why = batch_leg_lstd(c, kw, io, w)
            bad += [f"batch: {b}" for b in b_]
        count(legs, "batch")
    if why is None:
        b_, why = self_leg(kw, rng, legs)
        bad += [f"self: {b}" for b in b_]
    if why is None:
        bad += [f"env: {b}" for b in env_leg(kw, rng, legs)]
    return cg.verdict(tag, kw, bad, why)


def main():
    n_cases, seed = cg.parse_cases(sys.argv[1:])
    agents = cg.parse_agents(sys.argv[1:], NAMES) or AGENTS
    worst, legs = {}, {}
    cg.run(lambda idx: run_case(seed, idx, agents, worst, legs), n_cases, seed, NAMES, lambda failures: {"legs": legs, "worst": worst, "left_out": 0})


if __name__ == "__main__":
    main()
