#!/usr/bin/env python3
"""Random campaign over the newer agents -- ActorCritic / QActorCritic (10, 11), the TD ActorCritic (13), REINFORCE / BaselineREINFORCE (15, 16),
RecursiveLSTD / iLSTD (18, 19) on every register-family Fourier order, and the one-step agents on HIVTreatment (orders 1-3) -- at random learner
counts (ragged waves and LSTD lane groups), env offsets, discounts, step sizes, temperatures, episode caps and launch depths.  Legs:

    f64      Handler::handle on random in-bounds transitions (some terminal) for learners 0..M-1, M in {1, a random M < N, N}: learners M..N-1
             bitwise untouched, up to 8 of the handled learners replayed in f64 (tests/{ac,tdac,lstd,hiv}_numpy.py) at the per-agent tests' bounds
    batch    REINFORCE's handle_batch with a random T and ragged lengths (0 and T among them): returns bit for bit, theta against reinforce_batch
    self     one uninterrupted train() against random splits with queries between them (which must change nothing), the host trait loop,
             two env_offset shards, and a checkpoint saved and resumed -- bit for bit

    python tests/fuzz_agents.py [n_cases=200] [seed=0]          (GPU box; test infrastructure: imports oracle/)

One line per case and a SUMMARY {json} line (tests/campaign.run); exit code 1 on any mismatch."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rsrl_amd as ra  # noqa: E402
from oracle import oracle as orc  # noqa: E402
import fuzz_parity as fp  # noqa: E402
from tests import hiv_numpy as hv  # noqa: E402
from tests.ac_numpy import ac_rule, near_boundary  # noqa: E402
from tests import campaign as cg  # noqa: E402
from tests.agent_contract import diff, learner_state, rand_states, snapshot, trait_loop  # noqa: E402
from tests.campaign import TOP_OF_IDS, count  # noqa: E402
from tests.lstd_numpy import ilstd, near_tie_band, recursive_lstd  # noqa: E402
from tests.reinforce_numpy import reinforce_batch  # noqa: E402
from tests.tdac_numpy import tdac_rule  # noqa: E402

NAMES = {0: "HIV/QLearning", 1: "HIV/SARSA", 2: "HIV/ExpectedSARSA", 5: "HIV/PAL", 10: "ActorCritic", 11: "QActorCritic", 13: "TDActorCritic",
         15: "REINFORCE", 16: "BaselineREINFORCE", 18: "RecursiveLSTD", 19: "iLSTD"}
REG = [(0, o) for o in (1, 2, 3, 4, 5)] + [(1, 1), (2, 1)]          # the register-family Fourier orders check_config admits for them
N_DIM = {0: 2, 1: 4, 2: 4, 3: 6}
HIV_LO, HIV_HI = [-5.0] * 6, [8.0] * 6
EPS64 = np.finfo(np.float64).eps
TRAIT_LOOP = (10, 11, 13, 18, 19, 0, 1, 2, 5)                        # whose test file asserts train == the host trait loop


AGENTS = (10, 11, 13, 15, 16, 18, 19, -1)                           # -1: HIVTreatment with a one-step agent


def sample(rng, idx=None):
    """-> device kwargs of one configuration (case idx: the agents in turn)"""
    algo = AGENTS[idx % len(AGENTS)] if idx is not None else int(rng.choice(AGENTS))
    if algo < 0:
        algo = int(rng.choice([0, 1, 2, 5]))
    if algo in (0, 1, 2, 5):
        domain, order = 3, int(rng.integers(1, 4))
    else:
        domain, order = REG[int(rng.integers(0, len(REG)))]
    F = (order + 1) ** N_DIM[domain]
    kw = dict(domain=domain, order=order, algo=algo, seed=int(rng.integers(0, 1 << 20)), gamma=float(rng.choice([0.0, 0.9, 0.99, 1.0])),
              lr=float(rng.choice([0.02, 0.2])) / F, alpha=float(rng.choice([0.02, 0.2])) / F, tau=float(rng.choice([0.05, 0.5, 1.0, 5.0])),
              n_envs=int(rng.choice([1, 3, 5, 63, 64, 65, 130, 257, 1000])), env_offset=int(rng.choice([0, 64, 1000003, (1 << 31) - 65, TOP_OF_IDS])),
              max_episode_steps=int(rng.choice([0, 1, 25, 200])), steps_per_launch=int(rng.choice([0, 1, 5])))
    cg.top_of_ids(kw)                        # ((1 << 31) - 65: ids that straddle the sign bit)
    if algo in (10, 11, 13, 15, 16):
        kw["policy"] = ra.SOFTMAX
    elif algo in (18, 19):
        kw["policy"] = ra.RANDOM
        kw["n_steps"] = int(rng.choice([1, 2, 7, 32]))
    else:
        kw.update(policy=ra.EPSILON_GREEDY, epsilon=float(rng.choice([0.0, 0.1, 0.5])))
        if algo in (2, 5):
            kw["alpha"] = float(rng.choice([0.5, 1.0]))
    return kw


def hiv_rule(algo, W, phi_s, phi_n, a, r, gamma, alpha, eps, x_inner):
    """the one-step agents' TD error and the error sent on, f64 (tests/test_gpu_hiv.py; HIVTreatment never terminates)"""
    qs, qn = W.T @ phi_s, W.T @ phi_n
    if algo == ra.QLEARNING:
        d = r + gamma * qn.max() - qs[a]
        return d, d
    if algo == ra.SARSA:
        na = orc.policy_sample(orc.EGREEDY, qn, x_inner, eps=eps)
        d = r + gamma * qn[na] - qs[a]
        return d, d
    if algo == ra.EXPECTED_SARSA:
        p = orc.policy_probs(orc.EGREEDY, qn, eps=eps)
        d = r + gamma * float(np.dot(qn, p)) - qs[a]
        return d, alpha * d
    ast, nast = orc.argmax_first(qs), orc.argmax_first(qn)
    td = r + gamma * qn[ast] - qs[a]
    d = max(td - alpha * (qs[ast] - qs[a]), td - alpha * (qn[nast] - qn[a]))
    return d, alpha * d


def randomise(c, rng, i):
    al, F, A = c.cfg.algo, c.F, c.A
    if al in (18, 19):
        M = rng.normal(0.0, 1.0, size=(F, F))
        if al == 18:
            c.set_lstd_state(rng.normal(0.0, 0.5, size=F), 1e-3 * (np.eye(F) + (M + M.T) / (4.0 * F)), None, i)
        else:
            c.set_lstd_state(rng.normal(0.0, 0.5, size=F), np.eye(F) + 0.1 * M / np.sqrt(F), rng.normal(0.0, 1.0, size=F), i)
        return
    if al != ra.REINFORCE:
        c.set_weights(rng.normal(0.0, 0.1 if c.cfg.domain == 3 else 0.3, size=(F, c.n_out)).astype(np.float32), i)
    if al in (10, 11, 13, 15, 16):
        c.set_policy_weights(rng.normal(0.0, 0.3, size=(F, A)).astype(np.float32), i)


def f64_leg(c, kw, rng, worst):
    """handle rounds on learners 0..M-1 against the f64 rules; -> findings"""
    bad = []
    N, al, dom, order = c.N, kw["algo"], kw["domain"], kw["order"]
    gamma, lr, alpha, tau = kw["gamma"], kw["lr"], kw["alpha"], kw["tau"]
    for i in sorted(set([0, N - 1] + list(rng.integers(0, N, size=min(N, 24))))):
        randomise(c, rng, i)
    for rnd in range(int(rng.integers(2, 4))):
        M = int(rng.choice([1, int(rng.integers(1, N)) if N > 1 else 1, N]))
        if dom != 3:
            c.states = rand_states(orc, dom, N, rng)
        a = rng.integers(0, c.A, size=N).astype(np.int32)
        frm, nxt, rew, term = c.domain_step(a)
        if dom != 3:
            term = (term | (rng.random(N) < 0.25)).astype(np.uint8)
        watch = sorted(set(list(range(M, min(N, M + 70))) + [N - 1] + list(rng.integers(M, N, size=8) if M < N else [])) - set(range(M)))
        before = {j: learner_state(c, j) for j in watch}
        rep = sorted(set([0, M - 1] + list(rng.integers(0, M, size=6))))
        start = {i: list(learner_state(c, i).values()) for i in rep}
        t = c.step_count
        td = c.handle(frm[:, :M], a[:M], rew[:M], nxt[:, :M], term[:M])
        for j in watch:
            if diff(learner_state(c, j), before[j]):
                bad.append(f"round {rnd}: learner {j} >= M = {M} changed")
                break
        for i in rep:
            r, tm, ai = float(rew[i]), bool(term[i]), int(a[i])
            got = list(learner_state(c, i).values())
            if dom == 3:
                phi_s, phi_n = hv.fourier(frm[:, i:i + 1], order, HIV_LO, HIV_HI)[:, 0], hv.fourier(nxt[:, i:i + 1], order, HIV_LO, HIV_HI)[:, 0]
            else:
                phi_s, phi_n = orc.fourier_project(dom, order, frm[:, i]), orc.fourier_project(dom, order, nxt[:, i])
            x = orc.draw(kw["seed"], kw["env_offset"] + i, t, orc.BLK_INNER)
            sphi = float(np.abs(phi_s).sum())
            if al in (18, 19):
                theta, mat = start[i][0], start[i][1]
                if al == 18:
                    d, theta, mat = recursive_lstd(theta, mat, phi_s, phi_n, r, tm, gamma)
                    want = [theta, mat]
                else:
                    rounds = []
                    d, theta, mat, mu = ilstd(theta, mat, start[i][2], phi_s, phi_n, r, tm, gamma, alpha, kw["n_steps"], rounds=rounds)
                    if any(near_tie_band(m) for m in rounds):
                        continue                                   # (an |mu_j| within 1e-9 of the 1e-7 tie band: which j is chosen is a rounding)
                    want = [theta, mat, mu]
                tol = 16.0 * c.F * (1 + (kw["n_steps"] if al == 19 else 0)) * EPS64
                ok_td = abs(float(td[i]) - d) <= 2.0 ** -22 * (1.0 + abs(d))
                errs = [float(np.max(np.abs(g - w))) / (1.0 + float(np.max(np.abs(w)))) for g, w in zip(got, want)]
                fracs = [e / tol for e in errs]
            elif dom == 3:
                W = start[i][0].astype(np.float64)
                d, e = hiv_rule(al, W, phi_s, phi_n, ai, r, gamma, alpha, kw["epsilon"], x)
                ok_td = abs(float(td[i]) - d) <= 2e-5 * (1 + abs(d))
                want_col = W[:, ai] + lr * e * phi_s
                err = float(np.max(np.abs(got[0][:, ai] - want_col)))
                errs = [err / (1.0 + float(np.max(np.abs(want_col))))]
                fracs = [err / (3e-6 * (1 + abs(d)) * max(1.0, sphi))]
            else:
                W, Th = start[i][0].astype(np.float64), start[i][1].astype(np.float64)
                if al in (10, 11):
                    if not tm and near_boundary(orc.policy_probs(orc.SOFTMAX, Th.T @ phi_n, tau=tau), x):
                        continue
                    d, W2, T2 = ac_rule(orc, al == 11, W, Th, phi_s, phi_n, ai, r, tm, gamma, lr, alpha, tau, x)
                    pairs = ((got[0], W2, W), (got[1], T2, Th))
                else:
                    d, w2, T2 = tdac_rule(W, Th, phi_s, phi_n, ai, r, tm, gamma, lr, alpha, tau)
                    pairs = ((got[0][:, 0], w2, W[:, 0]), (got[1], T2, Th))
                ok_td = abs(float(td[i]) - d) <= 2e-5 * (1 + abs(d))
                errs, fracs = [], []
                for g, w, old in pairs:
                    bound = 3e-6 * (1 + float(np.max(np.abs(w - old)))) * sphi + 3e-6 * float(np.max(np.abs(old)))
                    err = float(np.max(np.abs(g - w)))
                    errs.append(err / (1.0 + float(np.max(np.abs(w)))))
                    fracs.append(err / max(bound, 1e-300))
            ok_w = all(f <= 1.0 for f in fracs)
            wr = worst.setdefault(NAMES[al], {"td": 0.0, "w": 0.0, "bound_used": 0.0, "replayed": 0})
            wr["td"] = max(wr["td"], abs(float(td[i]) - d) / (1 + abs(d)))
            wr["w"] = max([wr["w"]] + errs)
            wr["bound_used"] = max([wr["bound_used"]] + fracs)
            wr["replayed"] += 1
            if not (ok_td and ok_w):
                bad.append(f"round {rnd} M {M}: learner {i} td {float(td[i]):.6g} vs f64 {d:.6g}, state errors {['%.1e' % e for e in errs]}")
    return bad


def f32_returns(rewards, gamma):
    g, gm, out = np.float32(0.0), np.float32(gamma), []
    for r in rewards:
        g = np.float32(np.float32(r) + np.float32(gm * g))
        out.append(g)
    return out


def batch_leg(c, kw, rng, worst):
    """REINFORCE's Handler<&Batch> with ragged lengths; -> findings"""
    bad = []
    N, T, dom, order = c.N, int(rng.integers(1, 13)), kw["domain"], kw["order"]
    rep = sorted(set([0, N - 1] + list(rng.integers(0, N, size=6))))
    base = kw["algo"] == ra.BASELINE_REINFORCE
    for i in rep:
        randomise(c, rng, i)
    Ts = {i: c.get_policy_weights(i) for i in rep}
    Bs = {i: c.get_weights(i) for i in rep} if base else None
    thb0, g0 = {i: c.get_behaviour_weights(i) for i in rep}, c.return_carry
    S = np.stack([rand_states(orc, dom, N, rng) for _ in range(T)])
    A = rng.integers(0, c.A, size=(T, N)).astype(np.int32)
    R = rng.normal(0.0, 1.0, size=(T, N)).astype(np.float32)
    L = rng.integers(0, T + 1, size=N).astype(np.uint32)
    L[rep[0]], L[rep[-1]] = 0, T                                    # (an empty batch and a full one among the replayed learners)
    ret = c.handle_batch(S, A, R, L, returns=True)
    for i in rep:
        n = int(L[i])
        if not np.array_equal(ret[:n, i].view(np.uint32), np.array(f32_returns(R[:n, i], kw["gamma"]), dtype=np.float32).view(np.uint32)) or \
                not np.isnan(ret[n:, i]).all():
            bad.append(f"returns of learner {i}")
        got = c.get_policy_weights(i)
        if n == 0:
            if not np.array_equal(got, Ts[i]):
                bad.append(f"learner {i} with an empty batch moved")
            continue
        phis = [orc.fourier_project(dom, order, S[t, :, i]) for t in range(n)]
        want, _ = reinforce_batch(Ts[i], phis, A[:n, i], R[:n, i].astype(np.float64), kw["gamma"], kw["alpha"], kw["tau"], None if Bs is None else Bs[i])
        sphi = sum(np.abs(p).sum() for p in phis)
        bound = 3e-6 * (1 + float(np.max(np.abs(want - Ts[i])))) * sphi + 3e-6 * float(np.max(np.abs(Ts[i])))
        err = float(np.max(np.abs(got - want)))
        wr = worst.setdefault(NAMES[kw["algo"]], {"td": 0.0, "w": 0.0, "bound_used": 0.0, "replayed": 0})
        wr["w"] = max(wr["w"], err / (1.0 + float(np.max(np.abs(want)))))
        wr["bound_used"] = max(wr["bound_used"], err / max(bound, 1e-300))
        wr["replayed"] += 1
        if err > bound:
            bad.append(f"theta of learner {i}: {err:.2e} > {bound:.2e}")
        if not np.array_equal(c.get_behaviour_weights(i), thb0[i]):
            bad.append(f"theta_b of learner {i} moved")
    if not np.array_equal(c.return_carry, g0):
        bad.append("the running returns moved")
    return bad


def self_leg(kw, rng, legs):
    """-> findings: random splits with queries between, the trait loop, shards, a checkpoint -- each against one uninterrupted run.  Three
    learners are compared, and the checksum with the split alone; the trait, shard and checkpoint parts run in half of the cases each"""
    bad, made, counter = [], [], {}
    N, K = kw["n_envs"], int(rng.choice([10, 25, 40]))
    look = sorted(set([0, N // 2, N - 1]))

    def full(c):
        return snapshot(c, look)
    ref = cg.reference_run(kw, K, full)
    with tempfile.TemporaryDirectory() as td:
        def between(c):
            b_, m_ = fp.query_leg(c, rng, td, counter)
            bad.extend(b_); made.extend(m_)
        got, calls = cg.split_run(kw, rng, K, cg.draw_calls(rng, K, 1, 4), full, between=between)
    if cg.differs(got, ref):
        bad.append(f"train {calls} with queries {made} != train({K})")
    count(legs, "split+query")
    if kw["algo"] in TRAIT_LOOP and rng.random() < 0.5:
        if cg.differs(cg.trait_run(kw, K, kw["max_episode_steps"], trait_loop, full), ref, checksum=False):
            bad.append("the host trait loop != train")
        count(legs, "trait")
    if N >= 3 and rng.random() < 0.5:
        # a ragged shard point, and its own comparison: the env side and the learners on either side of each seam against a second unsharded run
        n1 = int(rng.integers(1, N))
        parts = cg.shard_run(kw, K, (n1, N - n1), lambda cs: (cs.states, cs.actions, learner_state(cs, 0), learner_state(cs, cs.N - 1)))
        with ra.Context(**kw) as cf:
            cf.reset()
            cf.train(K, want_stats=False)
            okp = np.array_equal(np.concatenate([parts[0][0], parts[1][0]], axis=1), cf.states) and \
                np.array_equal(np.concatenate([parts[0][1], parts[1][1]]), cf.actions) and \
                not diff(parts[0][2], learner_state(cf, 0)) and not diff(parts[0][3], learner_state(cf, n1 - 1)) and \
                not diff(parts[1][2], learner_state(cf, n1)) and not diff(parts[1][3], learner_state(cf, N - 1))
        if not okp:
            bad.append(f"shards {n1} + {N - n1} != the unsharded run")
        count(legs, "shard")
    if rng.random() < 0.5:
        k1 = int(rng.integers(1, K))

        def carry(c, c2):
            if kw["domain"] == 3:
                c2.set_hidden_states(c.get_hidden_states())            # (after the observations: set_states re-derives the hidden state from them)
            if kw["algo"] in (15, 16):
                c2.return_carry = c.return_carry
                for i in range(N):
                    c2.set_behaviour_weights(c.get_behaviour_weights(i), i)
        if cg.differs(cg.resume_run(kw, K, k1, full, carry=carry), ref, checksum=False):
            bad.append(f"checkpoint at {k1} resumed != train({K})")
        count(legs, "ckpt")
    return bad


def run_case(rng, idx, worst, legs):
    kw = sample(rng, idx)
    al = kw["algo"]
    tag = f"{idx:4d} {NAMES[al]:18s} dom {kw['domain']} ord {kw['order']} N {kw['n_envs']:4d} off {kw['env_offset']:7d} cap {kw['max_episode_steps']:3d} " \
          f"spl {kw['steps_per_launch']}"
    c, refused = cg.create(tag, kw)
    if refused:
        return refused
    bad = []
    with c:
        c.reset()
        if al in (15, 16):
            bad += [f"batch: {b}" for b in batch_leg(c, kw, rng, worst)]
            count(legs, "batch")
        else:
            bad += [f"f64: {b}" for b in f64_leg(c, kw, rng, worst)]
            count(legs, "f64")
    bad += [f"self: {b}" for b in self_leg(kw, rng, legs)]
    return cg.verdict(tag, kw, bad)


def main():
    n_cases, seed = cg.parse_cases(sys.argv[1:])
    rng = np.random.default_rng(seed)                               # one generator through the whole run: a leg's draws decide the next case
    worst, legs = {}, {}
    cg.run(lambda idx: run_case(rng, idx, worst, legs), n_cases, seed, NAMES, lambda failures: {"legs": legs, "worst_vs_f64": worst})


if __name__ == "__main__":
    main()
