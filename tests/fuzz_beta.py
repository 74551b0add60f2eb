#!/usr/bin/env python3
"""Random campaign over the two Beta-policy agents on ContinuousMountainCar -- the iLSTD ActorCritic (21; "BetaActorCritic") and NAC (28) -- in the
style of tests/fuzz_agents.py: Fourier orders 1-5 at random learner counts (idle and ragged lane groups), env offsets up to the top of the id range,
discounts, log-uniform rates, episode caps (0: none), launch depths, solve rounds 1-4 (21) and actor periods P in {1, 2, 7, 100} (28: every step,
and above the cap).  The policy columns put their weight on the constant feature so that each case holds learners in every branch of the device's
Softplus and its gradient -- a preference >= 10 (linear, sigma = 1), one in (-17, 10), one <= -20 (alpha is exactly 1 in f32 and the mode takes
the mean branch) -- next to learners with general columns; the actions handed to handle include 0 and 1 (clamped to 2^-24 and 1 - 2^-24), their
neighbours and interior values.  Legs:

    f64      handle on learners 0..M-1, M in {1, a random M, N}: learners M..N-1 bitwise untouched.  21: theta, A, mu and td_error_out bit for bit
             an RSRL_ILSTD ctx's on the same transitions, the columns against tests/beta_numpy.tdac_beta_rule from the device's own projection.
             28: w and delta against tests/nac_numpy.sarsa_handle, q_evaluate_f32 against q_value, nac_update under a random mask bit for bit
             nac_handle_f32 with ||g|| within 1e-4 (relative) of the 1e-3 floor on either side.  Both: policy_params / policy_mode / policy_pdf
             on random states against tests/beta_numpy at the bounds of tests/test_gpu_tdac_beta.py
    self     one uninterrupted train(K) from a start with learners near the goal (terminal ends occur) against random splits with read-only calls
             between them (the checksum equal around each), the host trait loop, two env_offset shards joined (even n_envs) and a checkpoint
             resumed -- bit for bit: the columns, w / the f64 critic, the pending f32 actions

    python tests/fuzz_beta.py [n_cases=200] [seed=0] [agents=BetaActorCritic,NAC]      (GPU box; test infrastructure: imports oracle/)

Case idx draws everything from case_rng(seed, idx, agents), the host inputs of its f64 leg first (tests/test_fuzz_late_cpu.py rebuilds them without
a device).  A learner-round whose decision the f64 restatement finds within a rounding of its boundary -- an inner draw within MARGIN of an
acceptance test (28), an |mu_j| next to iLSTD's tie band (21) -- is left out of the tolerance comparisons only; at most 5 % of the replayed
learner-rounds of a run, asserted here.  The bounds: bound_of below.  One line per case and a SUMMARY {json} line
(tests/campaign.run); exit code 1 on any mismatch."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rsrl_amd as ra  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import beta_numpy as bn  # noqa: E402
from tests import nac_numpy as nn  # noqa: E402
from tests import campaign as cg  # noqa: E402
from tests.agent_contract import diff, join_shards, learner_state, snapshot, trait_loop  # noqa: E402
from tests.campaign import TOP_OF_IDS, count  # noqa: E402
from tests.lstd_numpy import near_tie_band  # noqa: E402
from tests.test_gpu_nac_beta import MEASURED as NAC_MEASURED  # noqa: E402
from tests.test_gpu_tdac_beta import MEASURED as TDAC_MEASURED  # noqa: E402

NAMES = {21: "BetaActorCritic", 28: "NAC"}
AGENTS = (21, 28)
CMC = ra.CONTINUOUS_MOUNTAIN_CAR
MAX_K = 60
REPLAYED = 8
ROUNDS = 2
LEFT_OUT_CAP = 0.05
LO_S, HI_S = np.array([bn.X_BOUNDS[0], bn.V_BOUNDS[0]]), np.array([bn.X_BOUNDS[1], bn.V_BOUNDS[1]])

# The f32 chain of psi, ln and exp has no derivable bound (the docstrings of tests/test_gpu_tdac_beta.py and tests/test_gpu_nac_beta.py): every
# figure is asserted at four times a measured maximum, in those modules' normalisations.  Where the full campaign's maximum
# (profiles/fuzz_late_agents.md) stayed below a figure one of the two modules already bounds, that module's constant is the bound; OWN holds
# the figures they do not bound: orders 2 and 4; the learners whose columns lie outside the range of the modules' rule tests (cls below); the
# density at alpha + beta > PDF_WIDE, the largest sum the module's random preferences in [-3, 3] reach (it evaluates eight larger pairs, at
# actions away from their peaks): ln B passes through lgammaf(alpha + beta), whose f32 spacing grows with its value.
PDF_WIDE = 2.0 * (1.0 + float(np.log1p(np.exp(3.0))))
OWN = {
    ("rule", 2): 4 * 1.405e-7, ("rule", 4): 4 * 1.961e-7, ("rule_edge", 2): 4 * 4.085e-7, ("rule_edge", 4): 4 * 2.807e-7,
    ("w", 2): 4 * 1.541e-7, ("w", 4): 4 * 1.092e-7, ("w_edge", 1): 4 * 2.920e-7, ("w_edge", 2): 4 * 2.559e-7, ("w_edge", 4): 4 * 3.034e-7, ("w_edge", 5): 4 * 1.176e-6,
    ("delta", 2): 4 * 2.728e-7, ("delta", 4): 4 * 2.699e-7, ("delta_edge", 2): 4 * 4.471e-7, ("delta_edge", 4): 4 * 7.257e-7, ("delta_edge", 5): 4 * 3.618e-6,
    ("q", 2): 4 * 2.550e-7, ("q", 4): 4 * 1.988e-7, ("q_edge", 2): 4 * 3.814e-7, ("q_edge", 3): 4 * 1.215e-6, ("q_edge", 4): 4 * 5.654e-7, ("q_edge", 5): 4 * 3.143e-6,
    "pdf_wide": 4 * 3.426e-5,
}


def bound_of(name, order):
    """OWN's entry, else the module's constant for the figure (a learner class `_edge` whose maximum stayed below it shares it)"""
    if (name, order) in OWN or name in OWN:
        return OWN.get((name, order), OWN.get(name))
    base = name[:-5] if name.endswith("_edge") else name
    if base in ("params", "mode", "pdf"):
        return TDAC_MEASURED[base]
    return (TDAC_MEASURED if base == "rule" else NAC_MEASURED)[(base, order)]


def case_rng(seed, idx, agents=AGENTS):
    return cg.case_rng(seed, idx, agents[idx % len(agents)])


def sample(rng, idx=None, agents=AGENTS):
    """-> device kwargs of one configuration (case idx: the agents in turn)"""
    algo = agents[idx % len(agents)] if idx is not None else int(rng.choice(agents))
    kw = dict(domain=CMC, order=int(rng.integers(1, 6)), algo=algo, policy=ra.BETA, seed=int(rng.integers(0, 1 << 20)),
              gamma=float(rng.choice([0.0, 0.9, 0.99, 1.0])), lr=float(10 ** rng.uniform(-4, -1.3)), alpha=float(10 ** rng.uniform(-3, -0.5)),
              n_envs=int(rng.choice([1, 3, 5, 63, 64, 65, 130, 257])), env_offset=int(rng.choice([0, 64, 1000003, (1 << 31) - 65, TOP_OF_IDS])),
              max_episode_steps=int(rng.choice([0, 1, 7, 23, 200])), steps_per_launch=int(rng.choice([0, 1, 5, 64])),
              n_steps=int(rng.integers(1, 5)) if algo == 21 else int(rng.choice([1, 2, 7, 100])))
    return cg.top_of_ids(kw)


def preference(rng, branch):
    """a preference in branch 0 (>= 10: Softplus is the identity, its gradient 1), 1 (inside (-17, 10)) or 2 (<= -20: 1 + Softplus is 1 in f32)"""
    return float([rng.uniform(10.0, 30.0), rng.uniform(-16.9, 9.9), rng.uniform(-30.0, -20.0)][branch])


def columns(rng, N, F):
    """(N, F, 2) f32: three learners in four with all weight on the constant feature (the last one), the branches of the two columns cycling
    through all nine pairs from a random start; the fourth with general columns, sum |w| in [0.5, 3] as the modules' rule tests"""
    W = np.zeros((N, F, 2), dtype=np.float32)
    shift = int(rng.integers(0, 9))
    for i in range(N):
        if i % 4 == 3:
            w = rng.normal(size=(F, 2))
            W[i] = w * rng.uniform(0.5, 3.0, size=2) / np.abs(w).sum(axis=0)
        else:
            k = (i - i // 4 + shift) % 9
            W[i, F - 1] = [preference(rng, k % 3), preference(rng, k // 3)]
    return W


def edge_actions(rng, N):
    """f32 actions in [0, 1]: 0, 1, their neighbours, the clamp's own values and their neighbours, interior values"""
    one, zero = np.float32(1.0), np.float32(0.0)
    lo, hi = np.float32(bn.LO), np.float32(bn.HI)
    edges = np.array([0.0, 1.0, np.nextafter(zero, one), np.nextafter(one, zero), lo, hi, np.nextafter(lo, one), np.nextafter(lo, zero), 0.5], dtype=np.float32)
    a = rng.uniform(0.0, 1.0, size=N).astype(np.float32)
    pick = rng.random(N) < 0.4
    a[pick] = edges[rng.integers(0, len(edges), size=int(pick.sum()))]
    a[rng.integers(0, N)] = 0.0
    a[rng.integers(0, N)] = 1.0
    return a


def f64_inputs(rng, kw):
    """the host side of the f64 leg, no device"""
    N, al = kw["n_envs"], kw["algo"]
    F = (kw["order"] + 1) ** 2
    io = dict(F=F, W=columns(rng, N, F), rounds=[])
    if al == 21:
        io["init"] = [(rng.normal(0.0, 0.5, size=F), np.eye(F) + 0.1 * rng.normal(0.0, 1.0, size=(F, F)) / np.sqrt(F), rng.normal(0.0, 1.0, size=F)) for _ in range(N)]
    else:
        w = rng.normal(0.0, 1.0, size=(N, 3 * F))
        io["w"] = (w * rng.uniform(0.5, 3.0, size=(N, 1)) / np.abs(w).sum(axis=1, keepdims=True)).astype(np.float32)
    for _ in range(ROUNDS):
        frm = rng.uniform(LO_S, HI_S, size=(N, 2)).T.astype(np.float32)
        a = edge_actions(rng, N)
        nxt, rew, term = np.zeros_like(frm), np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.uint8)
        for i in range(N):
            ns, r, t = bn.cmc_step(frm[:, i], float(a[i]) if al == 21 else 2.0 * float(a[i]) - 1.0)
            nxt[:, i], rew[i], term[i] = np.asarray(ns, dtype=np.float32), np.float32(r), bool(t)
        term = (term.astype(bool) | (rng.random(N) < 0.25)).astype(np.uint8)
        M = int(rng.choice([1, int(rng.integers(1, N + 1)), N]))
        rep = sorted(set([0, M - 1] + [int(x) for x in rng.integers(0, M, size=REPLAYED - 2)]))
        io["rounds"].append((frm, a, rew, nxt, term, M, rep))
    io["S"] = rng.uniform(LO_S, HI_S, size=(N, 2)).T.astype(np.float32)
    io["a_pdf"] = edge_actions(rng, N)
    if al == 28:
        # NAC::handle(()): a random mask; where N allows, ||g|| a relative 1e-7 .. 1e-4 below and above the 1e-3 floor, and g = 0
        io["mask"] = (rng.random(N) < 0.7).astype(np.uint8)
        io["w_update"] = (rng.normal(size=(N, 3 * F)) * rng.uniform(0.01, 3.0, size=(N, 1))).astype(np.float32)
        for j, scale in zip(range(min(N, 3)), (1.0 - 10 ** rng.uniform(-7, -4), 1.0 + 10 ** rng.uniform(-7, -4), 0.0)):
            g = io["w_update"][j, :2 * F].astype(np.float64)
            io["w_update"][j, :2 * F] = (g / np.linalg.norm(g) * 1e-3 * scale).astype(np.float32)
            io["mask"][j] = 1
    return io


def features(kw, s):
    return orc.fourier_project(orc.MOUNTAIN_CAR, kw["order"], s)


def left_out_nac(kw, W, phi_n, i, t, term):
    """(the inner draw of learner i at step t in f64, whether the restatement leaves the learner-round out)"""
    xa, xb = float(phi_n @ W[:, 0]), float(phi_n @ W[:, 1])
    al, be = bn.beta_params(xa, xb)
    na, margin = bn.beta_sample(kw["seed"], np.array([kw["env_offset"] + i]), t, nn.BLK_INNER, float(al), float(be))
    return float(na[0]), bool(margin[0] < nn.MARGIN) and not term


def note(worst, name, order, fig):
    key = "%s/%d" % (name, order)
    worst[key] = max(worst.get(key, 0.0), float(fig))


def cls(name, i):
    """the figure's name for learner i: the learners with general columns (|x| <= 3: the range of the two modules' rule tests) keep the name and the
    modules' bounds, those with all weight on the constant feature (|x| up to 30) are `name`_edge with bounds of their own"""
    return name if i % 4 == 3 else name + "_edge"


def held(bad, worst, name, order, fig, what):
    note(worst, name, order, fig)
    bound = bound_of(name, order)
    if not fig <= bound:
        bad.append(f"{what}: {name} {fig:.4g} > {bound:.4g}")


def policy_side(c, kw, io, bad, worst):
    order, N = kw["order"], c.N
    W = np.stack([c.get_policy_weights(i) for i in range(N)]).astype(np.float64)
    S, a = io["S"], io["a_pdf"]
    phi = c.project(S).astype(np.float64)
    x = np.einsum("fn,nfk->nk", phi, W)
    al, be = bn.beta_params(x[:, 0], x[:, 1])
    ga, gb = c.policy_params(S)
    held(bad, worst, "params", order, max(float(np.max(np.abs(ga - al) / np.maximum(1.0, al))), float(np.max(np.abs(gb - be) / np.maximum(1.0, be)))), "policy_params")
    if ga.min() < 1.0 or gb.min() < 1.0:
        bad.append("a parameter below 1")
    mode = c.policy_mode(S)
    held(bad, worst, "mode", order, float(np.max(np.abs(mode - bn.beta_mode(ga.astype(np.float64), gb.astype(np.float64))))), "policy_mode")
    pdf = c.policy_pdf(S, a)
    wantp = bn.beta_pdf(al, be, a.astype(np.float64))
    if not np.isfinite(pdf).all():
        bad.append("policy_pdf is not finite")
    err = np.abs(pdf - wantp) / np.maximum(1.0, wantp)
    wide = al + be > PDF_WIDE
    for name, sel in (("pdf", ~wide), ("pdf_wide", wide)):
        if sel.any():
            j = int(np.flatnonzero(sel)[np.argmax(err[sel])])
            if err[j] > worst.get("%s/%d" % (name, order), 0.0):
                worst["%s_at/%d" % (name, order)] = [float(al[j]), float(be[j]), float(a[j]), float(wantp[j])]      # (alpha, beta, action, density) of the worst figure
            held(bad, worst, name, order, float(err[j]), "policy_pdf")


def untouched(c, M, N, rng):
    watch = sorted(set(list(range(M, min(N, M + 70))) + [N - 1] + [int(x) for x in (rng.integers(M, N, size=8) if M < N else [])]) - set(range(M)))
    return {j: learner_state(c, j) for j in watch}


def f64_leg_tdac(c, v, kw, io, rng, worst, tally):
    bad = []
    N, order = c.N, kw["order"]
    for i, (theta, A, mu) in enumerate(io["init"]):
        c.set_lstd_state(theta, A, mu, i)
        v.set_lstd_state(theta, A, mu, i)
        c.set_policy_weights(io["W"][i], i)
    policy_side(c, kw, io, bad, worst)                             # (on the columns as sampled: handle moves them)
    for rnd, (frm, a, rew, nxt, term, M, rep) in enumerate(io["rounds"]):
        before = untouched(c, M, N, rng)
        start = {i: (c.get_lstd_state(i), c.get_policy_weights(i).astype(np.float64)) for i in rep}
        sl = (slice(None), slice(0, M))
        phi32 = c.project(frm)
        td = c.handle(np.ascontiguousarray(frm[sl]), a[:M], rew[:M], np.ascontiguousarray(nxt[sl]), term[:M])
        td_v = v.handle(np.ascontiguousarray(frm[sl]), np.zeros(M, dtype=np.int32), rew[:M], np.ascontiguousarray(nxt[sl]), term[:M])
        if any(diff(learner_state(c, j), s) for j, s in before.items()):
            bad.append(f"round {rnd}: a learner >= M = {M} changed")
        if td.tobytes() != td_v.tobytes() or any(x.tobytes() != y.tobytes() for i in range(M) for x, y in zip(c.get_lstd_state(i), v.get_lstd_state(i))):
            bad.append(f"round {rnd}: the critic != an RSRL_ILSTD ctx's")
        for i in rep:
            (theta, A, mu), W = start[i]
            mus = []
            d, _, _, _, W2 = bn.tdac_beta_rule(theta, A, mu, W, features(kw, frm[:, i]), features(kw, nxt[:, i]), float(a[i]), float(rew[i]), bool(term[i]),
                                               kw["gamma"], kw["lr"], kw["n_steps"], kw["alpha"], rounds=mus, phi32=phi32[:, i].astype(np.float64))
            tally["replayed"] += 1
            if abs(float(td[i]) - d) > 2.0 ** -22 * (1.0 + abs(d)):
                bad.append(f"round {rnd}: the diagnostic of learner {i}")
            if any(near_tie_band(m) for m in mus):
                tally["left_out"] += 1
                continue
            got = c.get_policy_weights(i).astype(np.float64)
            held(bad, worst, cls("rule", i), order, float(np.max(np.abs(got - W2) / np.maximum(1.0, np.abs(W2)))), f"round {rnd} learner {i} action {a[i]!r}")
    return bad


def f64_leg_nac(c, kw, io, rng, worst, tally):
    bad = []
    N, order, F = c.N, kw["order"], c.F
    for i in range(N):
        c.set_weights(io["w"][i].reshape(-1, 1), i)
        c.set_policy_weights(io["W"][i], i)
    policy_side(c, kw, io, bad, worst)
    W64 = io["W"].astype(np.float64)
    for rnd, (frm, a, rew, nxt, term, M, rep) in enumerate(io["rounds"]):
        before = untouched(c, M, N, rng)
        start = {i: c.get_weights(i)[:, 0].astype(np.float64) for i in rep}
        phi_s, phi_n = c.project(frm).astype(np.float64), c.project(nxt).astype(np.float64)
        q = c.q_evaluate_f32(frm, a)
        wq = {i: nn.q_value(start[i], W64[i], phi_s[:, i], float(a[i])) for i in rep}
        for i in rep:
            held(bad, worst, cls("q", i), order, abs(float(q[i]) - wq[i]) / max(1.0, abs(wq[i])), f"round {rnd} q_evaluate_f32 of learner {i} action {a[i]!r}")
        sl = (slice(None), slice(0, M))
        t = c.step_count
        td = c.handle(np.ascontiguousarray(frm[sl]), a[:M], rew[:M], np.ascontiguousarray(nxt[sl]), term[:M])
        if any(diff(learner_state(c, j), s) for j, s in before.items()):
            bad.append(f"round {rnd}: a learner >= M = {M} changed")
        for i in rep:
            tally["replayed"] += 1
            if c.get_policy_weights(i).tobytes() != io["W"][i].tobytes():
                bad.append(f"round {rnd}: critic.handle moved the actor of learner {i}")
            na, out = left_out_nac(kw, W64[i], phi_n[:, i], i, t, bool(term[i]))
            if out:
                tally["left_out"] += 1
                continue
            d, w2 = nn.sarsa_handle(start[i], W64[i], phi_s[:, i], float(a[i]), float(rew[i]), phi_n[:, i], na, bool(term[i]), kw["gamma"], kw["lr"])
            got = c.get_weights(i)[:, 0].astype(np.float64)
            held(bad, worst, cls("delta", i), order, abs(float(td[i]) - d) / max(1.0, abs(d)), f"round {rnd} learner {i} action {a[i]!r}")
            held(bad, worst, cls("w", i), order, float(np.max(np.abs(got - w2) / np.maximum(1.0, np.abs(w2)))), f"round {rnd} learner {i} action {a[i]!r}")
    # NAC::handle(()) under the mask, bit for bit
    for i in range(N):
        c.set_weights(io["w_update"][i].reshape(-1, 1), i)
    t = c.step_count
    norm = c.nac_update(io["mask"])
    if c.step_count != t:
        bad.append("nac_update counted a batch-step")
    for i in range(N):
        got = c.get_policy_weights(i)
        if io["mask"][i]:
            want, wn = nn.nac_handle_f32(io["w_update"][i], io["W"][i], kw["alpha"])
            if got.tobytes() != want.tobytes() or norm[i].tobytes() != wn.tobytes():
                bad.append(f"nac_update of learner {i}: norm {norm[i]!r} want {wn!r}, max |d| {np.abs(got - want).max():.3g}")
        elif got.tobytes() != io["W"][i].tobytes() or norm[i] != 0.0:
            bad.append(f"nac_update moved learner {i} outside the mask")
        if c.get_weights(i)[:, 0].tobytes() != io["w_update"][i].tobytes():
            bad.append(f"nac_update moved the critic of learner {i}")
    return bad


def start_near_the_goal(c, off):
    """reset, then every fourth learner (by its index in the unsharded run) at x = 0.59, v = 0.06: terminal ends occur as well as cut ones"""
    c.reset()
    s = c.states
    s[:, (np.arange(c.N) + off) % 4 == 0] = np.array([[0.59], [0.06]], dtype=np.float32)
    c.states = s


def nac_trait_loop(c, K, cap):
    """the loop of nac_beta.rs through the trait calls (tests/test_gpu_nac_beta.py _nac_trait with the ctx's own period)"""
    P = int(c.cfg.n_steps)
    ep = c.episode_steps.astype(np.int64)
    for _ in range(K):
        update = (ep % P == 0).astype(np.uint8)
        a = c.actions
        frm, nxt, rew, term = c.domain_step()
        c.handle(frm, a, rew, nxt, term)
        ep += 1
        mask = (term.astype(bool) | ((ep >= cap) if cap > 0 else False)).astype(np.uint8)
        c.domain_reset(mask)
        ep[mask == 1] = 0
        c.policy_sample()
        c.nac_update(update)
    c.episode_steps = ep.astype(np.uint32)


def read_only_calls(c, rng, tmp):
    """this campaign's named calls, on its own draws, through tests/campaign.read_only_calls -> (findings, the calls made)"""
    N = c.N
    S = rng.uniform(LO_S, HI_S, size=(N, 2)).T.astype(np.float32)
    a = edge_actions(rng, N)
    i = int(rng.integers(0, N))
    calls = {"policy_params": lambda: c.policy_params(S), "policy_mode": lambda: c.policy_mode(S), "policy_pdf": lambda: c.policy_pdf(S, a),
             "policy_sample": lambda: c.policy_sample(S), "project": lambda: c.project(S), "get_weights": lambda: c.get_weights(i),
             "get_policy_weights": lambda: c.get_policy_weights(i), "checksum": lambda: c.checksum(), "states": lambda: c.states, "actions": lambda: c.actions,
             "episode_steps": lambda: c.episode_steps, "save_weights": lambda: c.save_weights(os.path.join(tmp, "q.ckpt"))}
    if c.cfg.algo == 21:
        calls.update({"q_evaluate": lambda: c.q_evaluate(S), "get_lstd_state": lambda: c.get_lstd_state(i)})
    else:
        calls["q_evaluate_f32"] = lambda: c.q_evaluate_f32(S, a)
    return cg.read_only_calls(c, rng, calls)


def self_leg(kw, rng, legs):
    """-> (findings, the reason the case diverged or None)"""
    bad, made = [], []
    N, cap, al = kw["n_envs"], kw["max_episode_steps"], kw["algo"]
    K = int(rng.choice([10, 25, 40, MAX_K]))
    ref = cg.reference_run(kw, K, snapshot, start_near_the_goal)
    if not all(np.isfinite(v).all() for v in ref[0].values()):
        return bad, f"train({K}) left non-finite state (lr {kw['lr']:.3g}, alpha {kw['alpha']:.3g})"
    with tempfile.TemporaryDirectory() as td:
        def between(c):
            b_, m_ = read_only_calls(c, rng, td)
            bad.extend(b_); made.extend(m_)
        got, calls = cg.split_run(kw, rng, K, cg.draw_calls(rng, K, 1, 4), snapshot, start_near_the_goal, between)
    names = cg.differs(got, ref)
    if names:
        bad.append(f"train {calls} with {made} != train({K}): {names}")
    count(legs, "split+query")
    names = cg.differs(cg.trait_run(kw, K, cap, trait_loop if al == 21 else nac_trait_loop, snapshot, start_near_the_goal), ref, checksum=False)
    if names:
        bad.append(f"the host trait loop != train({K}): {names}")
    count(legs, "trait")
    if N % 2 == 0:
        names = diff(join_shards(*cg.shard_run(kw, K, (N // 2, N // 2), snapshot, start_near_the_goal)), ref[0])
        if names:
            bad.append(f"two shards of {N // 2} joined != train({K}): {names}")
        count(legs, "shard")
    k1 = int(rng.integers(1, K))
    names = cg.differs(cg.resume_run(kw, K, k1, snapshot, start_near_the_goal), ref)
    if names:
        bad.append(f"checkpoint at {k1} resumed != train({K}): {names}")
    count(legs, "ckpt")
    return bad, None


def run_case(seed, idx, agents, worst, legs, tally):
    rng = case_rng(seed, idx, agents)
    kw = sample(rng, idx, agents)
    al = kw["algo"]
    io = f64_inputs(rng, kw)
    tag = f"{idx:4d} {NAMES[al]:15s} ord {kw['order']} N {kw['n_envs']:3d} off {kw['env_offset']:10d} cap {kw['max_episode_steps']:3d} spl {kw['steps_per_launch']:2d} " \
          f"gamma {kw['gamma']} lr {kw['lr']:.2e} alpha {kw['alpha']:.2e} n_steps {kw['n_steps']:3d}"
    c, refused = cg.create(tag, kw)
    if refused:
        return refused
    bad = []
    w = worst.setdefault(NAMES[al], {})
    with c:
        if al == 21:
            with ra.Context(**dict(kw, domain=ra.MOUNTAIN_CAR, algo=ra.ILSTD, policy=ra.RANDOM, alpha=kw["lr"])) as v:
                bad += [f"f64: {b}" for b in f64_leg_tdac(c, v, kw, io, rng, w, tally)]
        else:
            bad += [f"f64: {b}" for b in f64_leg_nac(c, kw, io, rng, w, tally)]
        count(legs, "f64")
    b_, why = self_leg(kw, rng, legs)
    bad += [f"self: {b}" for b in b_]
    return cg.verdict(tag, kw, bad, why)


def main():
    n_cases, seed = cg.parse_cases(sys.argv[1:])
    agents = cg.parse_agents(sys.argv[1:], NAMES) or AGENTS
    worst, legs, tally = {}, {}, {"replayed": 0, "left_out": 0}

    def left_out_cap(failures):
        if tally["left_out"] > LEFT_OUT_CAP * max(tally["replayed"], 1):
            line = f"{tally['left_out']} of {tally['replayed']} replayed learner-rounds left out: more than {LEFT_OUT_CAP:.0%}"
            failures.append({"case": None, "line": line, "config": None})
    cg.run(lambda idx: run_case(seed, idx, agents, worst, legs, tally), n_cases, seed, NAMES,
           lambda failures: {"legs": legs, "worst": worst, "replayed": tally["replayed"], "left_out": tally["left_out"]}, left_out_cap)


if __name__ == "__main__":
    main()
