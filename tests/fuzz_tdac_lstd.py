#!/usr/bin/env python3
"""Random campaign over the iLSTD ActorCritic (RSRL_ILSTD_ACTOR_CRITIC, 21), in the style of tests/fuzz_agents.py and kept apart from it: every
register-family Fourier order at random learner counts (ragged waves and lane groups), env offsets, discounts, rates, temperatures, solve rounds,
episode caps and launch depths.  Legs:

    f64      Handler::handle on random in-bounds transitions (some terminal) for learners 0..M-1, M in {1, a random M < N, N}: learners M..N-1
             bitwise untouched, up to 8 of the handled learners replayed with tests/tdac_lstd_numpy.py at tests/test_gpu_tdac_lstd.py's bounds
    critic   the same transitions through an iLSTD ctx (19): theta / A / mu and td_error_out bit for bit
    self     one uninterrupted train() against random splits with policy queries between them (which must change nothing), the host trait loop,
             two env_offset shards, and a checkpoint saved and resumed -- bit for bit

    python tests/fuzz_tdac_lstd.py [n_cases=100] [seed=0] [agents=21]          (GPU box; test infrastructure: imports oracle/)

One line per case and a SUMMARY {json} line (tests/campaign.run); exit code 1 on any mismatch."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rsrl_amd as ra  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import campaign as cg  # noqa: E402
from tests.agent_contract import diff, join_shards, learner_state, rand_states, snapshot, trait_loop  # noqa: E402
from tests.lstd_numpy import near_tie_band  # noqa: E402
from tests.tdac_lstd_numpy import tdac_lstd_rule  # noqa: E402

REG = [(0, o) for o in (1, 2, 3, 4, 5)] + [(1, 1), (2, 1)]
EPS64 = np.finfo(np.float64).eps
NAME = "iLSTDActorCritic"


def draw_config(rng):
    domain, order = REG[int(rng.integers(len(REG)))]
    N = int(rng.choice([1, 3, 16, 17, 63, 64, 65, int(rng.integers(2, 200))]))
    return dict(domain=domain, order=order, algo=ra.ILSTD_ACTOR_CRITIC, policy=ra.SOFTMAX, n_envs=N, seed=int(rng.integers(1 << 30)),
                env_offset=int(rng.choice([0, 0, int(rng.integers(1, 1 << 20))])), gamma=float(rng.uniform(0.8, 0.999)),
                lr=float(10 ** rng.uniform(-4, -1.3)), alpha=float(10 ** rng.uniform(-3, -0.5)), tau=float(rng.uniform(0.3, 2.0)),
                n_steps=int(rng.integers(1, 5)), max_episode_steps=int(rng.choice([0, 7, 23, 200])), steps_per_launch=int(rng.choice([0, 0, 1, 5, 64])))


def randomise(c, rng, also=()):
    F, init = c.F, []
    for i in range(c.N):
        theta, M, mu = rng.normal(0.0, 0.5, size=F), rng.normal(0.0, 1.0, size=(F, F)), rng.normal(0.0, 1.0, size=F)
        A, Th = np.eye(F) + 0.1 * M / np.sqrt(F), rng.normal(0.0, 0.3, size=(F, c.A)).astype(np.float32)
        for x in (c,) + tuple(also):
            x.set_lstd_state(theta, A, mu, i)
        c.set_policy_weights(Th, i)
        init.append((theta, A, mu, Th))
    return init


def leg_f64(kw, rng):
    """-> list of failures"""
    bad = []
    N = kw["n_envs"]
    ikw = dict(kw, algo=ra.ILSTD, policy=ra.RANDOM, alpha=kw["lr"])
    with ra.Context(**kw) as c, ra.Context(**ikw) as v:
        init = randomise(c, rng, also=(v,))
        c.states = rand_states(orc, kw["domain"], N, rng)
        a = rng.integers(0, c.A, size=N).astype(np.int32)
        frm, nxt, rew, term = c.domain_step(a)
        term = (term | (rng.random(N) < 0.25)).astype(np.uint8)
        M = int(rng.choice([1, N, int(rng.integers(1, N + 1))]))
        before = [learner_state(c, i) for i in range(M, N)]
        sl = (slice(None), slice(0, M))
        td = c.handle(np.ascontiguousarray(frm[sl]), a[:M], rew[:M], np.ascontiguousarray(nxt[sl]), term[:M])
        td_v = v.handle(np.ascontiguousarray(frm[sl]), a[:M], rew[:M], np.ascontiguousarray(nxt[sl]), term[:M])
        if any(diff(before[i - M], learner_state(c, i)) for i in range(M, N)):
            bad.append("learners M..N-1 moved")
        if td.tobytes() != td_v.tobytes() or any(x.tobytes() != y.tobytes() for i in range(M) for x, y in zip(c.get_lstd_state(i), v.get_lstd_state(i))):
            bad.append("critic != iLSTD ctx")
        F = c.F
        tol = 16.0 * F * (1 + kw["n_steps"]) * EPS64
        for i in rng.choice(M, size=min(M, 8), replace=False):
            theta, A, mu, Th = init[i]
            phi_s, phi_n = orc.fourier_project(kw["domain"], kw["order"], frm[:, i]), orc.fourier_project(kw["domain"], kw["order"], nxt[:, i])
            mus = []
            d, th2, A2, mu2, T2 = tdac_lstd_rule(theta, A, mu, Th.astype(np.float64), phi_s, phi_n, int(a[i]), float(rew[i]), bool(term[i]), kw["gamma"],
                                                 kw["lr"], kw["n_steps"], kw["alpha"], kw["tau"], rounds=mus)
            if abs(float(td[i]) - d) > 2.0 ** -22 * (1.0 + abs(d)):
                bad.append(f"delta of learner {i}")
            if not any(near_tie_band(m) for m in mus):
                for g, w in zip(c.get_lstd_state(i), (th2, A2, mu2)):
                    if np.max(np.abs(g - w)) > tol * (1.0 + np.max(np.abs(w))):
                        bad.append(f"f64 state of learner {i}")
            old = Th.astype(np.float64)
            bound = 3e-6 * (1 + np.max(np.abs(T2 - old))) * np.abs(phi_s).sum() + 3e-6 * np.max(np.abs(old))
            if np.max(np.abs(c.get_policy_weights(i) - T2)) > bound:
                bad.append(f"actor of learner {i}")
    return bad


def leg_self(kw, rng):
    """(this campaign's drift, kept: every train call asks for statistics, the calls are drawn one by one until they sum to K, the queries run
    after the last call too, no checksum is compared and the checkpoint loads into a ctx that has not trained)"""
    bad = []
    K, N, cap = int(rng.integers(5, 40)), kw["n_envs"], kw["max_episode_steps"]
    ref = cg.reference_run(kw, K, snapshot, want_stats=True)
    done = []

    def calls():
        while sum(done) < K:
            done.append(int(rng.integers(1, K - sum(done) + 1)))
            yield done[-1]

    def queries(c):
        S = c.states
        c.policy_probs(S); c.policy_sample(S); c.q_evaluate(S)
    if cg.differs(cg.split_run(kw, rng, K, calls(), snapshot, between=queries, after_last=True)[0], ref, checksum=False):
        bad.append("splits with queries")
    if cg.differs(cg.trait_run(kw, K, cap, trait_loop, snapshot), ref, checksum=False):
        bad.append("trait loop")
    if N >= 2:
        if diff(join_shards(*cg.shard_run(kw, K, (N // 2, N - N // 2), snapshot, want_stats=True)), ref[0]):
            bad.append("shards")
    k1 = int(rng.integers(1, K))
    if cg.differs(cg.resume_run(kw, K, k1, snapshot, overwrite=False, want_stats=True), ref, checksum=False):
        bad.append("checkpoint resume")
    return bad


def run_case(kw, rng, case):
    """-> (status, line, kw[, the failure's record]).  An exception inside a leg is a finding of the case, whose configuration is known: it is
    reported as a MISMATCH with the configuration, not as the runner's ERROR"""
    try:
        with ra.Context(**kw):
            pass
    except ra.RsrlHipError as e:
        return "refused", f"case {case}: REFUSED {str(e)[:90]} {json.dumps(kw)}", kw
    try:
        bad = [("f64", x) for x in leg_f64(kw, rng)] + [("self", x) for x in leg_self(kw, rng)]
    except Exception as e:      # noqa: BLE001
        bad = [("error", f"{type(e).__name__}: {str(e)[:200]}")]
    line = f"case {case}: {'FAIL ' + json.dumps(bad) if bad else 'ok'} {json.dumps(kw)}"
    return ("MISMATCH", line, kw, {"case": case, "legs": bad, "config": kw}) if bad else ("ok", line, kw)


def main():
    n_cases, seed = cg.parse_cases(sys.argv[1:], 100)
    agents = cg.parse_agents(sys.argv[1:], {21: NAME})
    if agents not in (None, (21,)):                                 # (the one agent of this campaign: the argument exists for the suite's uniform call)
        sys.exit(f"agents= must be 21 or {NAME}")
    rng = np.random.default_rng(seed)                               # one generator through the whole run: a leg's draws decide the next case
    cg.run(lambda case: run_case(draw_config(rng), rng, case), n_cases, seed, {21: NAME}, lambda failures: {"failures": failures, "failed": len(failures)})


if __name__ == "__main__":
    main()
