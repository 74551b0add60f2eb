#!/usr/bin/env python3
"""Adversarial campaign against the C ABI: configurations with out-of-range, non-finite and contradictory fields, and calls with null pointers, learner
indices and batch sizes out of range, non-finite states, actions outside the action set.  Whatever comes in, every entry point must RETURN (an error
code with a message, or success) -- no crash, no hang, no NaN-poisoned neighbour: after every abuse a small healthy ctx on the same device must still
train to the same checksum.  After the random cases, late_agents_leg aims a fixed list of such arguments at the entry points of GradientMC, LSTD,
LSTDLambda, the Beta iLSTD ActorCritic and NAC.

    python tests/fuzz_abi.py [n_cases=300] [seed=0]        (GPU box; each case runs in this process: a crash ends the campaign with its number)"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rsrl_amd as ra  # noqa: E402
from rsrl_amd import _abi  # noqa: E402

VALID_ALGOS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 16, 18, 19)       # 12, 14 and 17 are no algo
BAD_F = [float("nan"), float("inf"), -float("inf"), -1.0, 0.0, 1e308, -1e-320, 2.0]
INT_FIELDS = {
    "domain": [-1, 4, 99, 0, 1, 2, 3], "basis": [-1, 2, 0, 1], "order": [-3, 0, 8, 100, 1, 5, 7], "n_tilings": [-1, 0, 3, 5, 64, 4, 8, 16],
    "tiles_per_dim": [-1, 0, 1, 2, 1000, 65536, 8], "algo": [-1, 12, 14, 17, 20, 255] + list(VALID_ALGOS), "policy": [-1, 4, 7, 0, 1, 2, 3],
    "weight_mode": [-1, 2, 0, 1], "weight_dtype": [-1, 2, 5, 0, 1], "trace": [-1, 3, 0, 1, 2], "agent_policy": [-2, 4, -1, 0, 1, 2],
    "exchange": [-1, 3, 9, 0, 1, 2], "n_steps": [-1, 0, 33, 1000, 1, 4, 32], "peer_timeout_ms": [-5, 0, 1, 10 ** 9], "device": [-1, 1, 99, 0],
}
F_FIELDS = ["gamma", "lr", "alpha", "epsilon", "tau", "lam", "lr_td", "agent_epsilon", "agent_tau", "sigma", "epsilon_decay", "epsilon_min"]


def healthy_checksum():
    with ra.Context(n_envs=64, policy=1, seed=3, max_episode_steps=50) as c:
        c.reset()
        c.train(40, want_stats=False)
        return c.checksum()


def poke(L, h, rng, log):
    """a created ctx: abuse every entry point that takes arguments"""
    N = int(L.rsrl_hip_n_envs(h)); D = L.rsrl_hip_state_dim(h); A = L.rsrl_hip_n_actions(h); F = L.rsrl_hip_n_features(h); O = L.rsrl_hip_n_outputs(h)
    big = np.zeros(max(1, F * max(O, A)) + 16, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)       # noqa: E731
    st = _abi.Stats()
    calls = [
        lambda: L.rsrl_hip_reset(h),
        lambda: L.rsrl_hip_train(h, 3, C.byref(st)),
        lambda: L.rsrl_hip_train(h, 0, None),
        lambda: L.rsrl_hip_train(h, -5, None),
        lambda: L.rsrl_hip_get_weights(h, -1, p(big)), lambda: L.rsrl_hip_get_weights(h, N, p(big)), lambda: L.rsrl_hip_get_weights(h, 2 ** 40, p(big)),
        lambda: L.rsrl_hip_get_weights(h, 0, None), lambda: L.rsrl_hip_set_weights(h, 0, None), lambda: L.rsrl_hip_set_weights(h, N + 7, p(big)),
        lambda: L.rsrl_hip_get_traces(h, N, p(big)), lambda: L.rsrl_hip_set_traces(h, -3, p(big)), lambda: L.rsrl_hip_get_td_weights(h, N, p(big)),
        lambda: L.rsrl_hip_get_states(h, None), lambda: L.rsrl_hip_set_states(h, None), lambda: L.rsrl_hip_set_actions(h, None),
        lambda: L.rsrl_hip_set_episode_steps(h, None), lambda: L.rsrl_hip_set_q_carry(h, None),
        lambda: L.rsrl_hip_q_evaluate(h, None, 4, p(big)), lambda: L.rsrl_hip_q_evaluate(h, p(big), -1, p(big)), lambda: L.rsrl_hip_q_evaluate(h, p(big), 0, p(big)),
        lambda: L.rsrl_hip_save_weights(h, None), lambda: L.rsrl_hip_load_weights(h, None), lambda: L.rsrl_hip_load_weights(h, b"/nonexistent/dir/x"),
        lambda: L.rsrl_hip_save_weights(h, b"/nonexistent/dir/x"),
    ]
    # non-finite states and actions outside the action set through the setters, then a few steps: the ctx may learn garbage, it may not fault
    def bad_state():
        s = np.full((D, N), rng.choice([np.nan, np.inf, -np.inf, 1e30, -1e30]), dtype=np.float32)
        rc = L.rsrl_hip_set_states(h, p(s))
        a = np.full(N, int(rng.choice([-7, A, 2 ** 31 - 1, -2 ** 31])), dtype=np.int32)
        rc2 = L.rsrl_hip_set_actions(h, p(a))
        rc3 = L.rsrl_hip_train(h, 4, None)
        L.rsrl_hip_sync(h)
        return (rc, rc2, rc3)
    calls.append(bad_state)
    def bad_weights():
        w = np.full(F * O, rng.choice([np.nan, np.inf, 3e38]), dtype=np.float32)
        rc = L.rsrl_hip_set_weights(h, 0, p(w))
        rc2 = L.rsrl_hip_train(h, 3, None)
        L.rsrl_hip_sync(h)
        return (rc, rc2)
    calls.append(bad_weights)
    def handle_bad():
        M = int(rng.choice([0, 1, N, N + 5]))
        if M <= 0:
            return L.rsrl_hip_handle(h, p(big), p(big), p(big), p(big), p(big), M, p(big))
        s = np.zeros((D, M), dtype=np.float32); a = np.full(M, int(rng.choice([-1, A + 3, 0])), dtype=np.int32)
        r = np.full(M, rng.choice([np.nan, 1.0]), dtype=np.float32); t = np.full(M, 7, dtype=np.uint8); out = np.zeros(M, dtype=np.float32)
        return L.rsrl_hip_handle(h, p(s), p(a), p(r), p(s), p(t), M, p(out))
    calls.append(handle_bad)
    def eval_bad():                                    # the query entry points on non-finite / huge states
        M = int(rng.choice([1, 5, N]))
        s = np.full((D, M), rng.choice([np.nan, np.inf, -np.inf, 1e30, -3e38]), dtype=np.float32)
        out = np.zeros((max(A, O) + 1) * M + 64, dtype=np.float32); iout = np.zeros(64 * M + 64, dtype=np.int32)
        rcs = [L.rsrl_hip_q_evaluate(h, p(s), M, p(out)), L.rsrl_hip_q_find_max(h, p(s), M, p(iout), p(out)), L.rsrl_hip_policy_mode(h, p(s), M, p(iout))]
        if hasattr(L, "rsrl_hip_tile_indices"):
            rcs.append(L.rsrl_hip_tile_indices(h, p(s), M, p(iout)))
        L.rsrl_hip_sync(h)
        return rcs
    calls.append(eval_bad)
    def rollout_bad():
        n_st = np.zeros(N, dtype=np.uint32); tot = np.zeros(N, dtype=np.float32)
        return [L.rsrl_hip_rollout_greedy(h, int(v), p(n_st), p(tot)) for v in (-1, 1, 2, 30)]
    calls.append(rollout_bad)
    def ranks_bad():                                   # the multi-rank entry points: null lists, duplicates, counts and ranks out of range, garbage handles
        hbuf = (C.c_uint8 * (128 * 4))(*[int(x) for x in rng.integers(0, 256, 512)])
        two = (C.c_void_p * 2)(h, h); nul = (C.c_void_p * 2)(h, None)
        ws, rk, ex = C.c_int(0), C.c_int(0), C.c_int(0); ident = C.c_uint64(0)
        rcs = [L.rsrl_hip_peer_export(h, int(v), None) for v in (-1, 0, 1)]
        rcs += [L.rsrl_hip_peer_export(h, int(v), hbuf) for v in (-1, 0, 100000)]
        rcs += [L.rsrl_hip_peer_connect(h, None, 2, 0), L.rsrl_hip_peer_connect(h, hbuf, 2, 5), L.rsrl_hip_peer_connect(h, hbuf, 0, 0),
                L.rsrl_hip_peer_connect(h, hbuf, 2, int(rng.integers(0, 2)))]
        rcs += [L.rsrl_hip_comm_init(h, None, 1, 0), L.rsrl_hip_comm_init(h, hbuf, 0, 0), L.rsrl_hip_comm_init(h, hbuf, 2, 7), L.rsrl_hip_comm_init(h, hbuf, -1, -1)]
        rcs += [L.rsrl_hip_group_create(None, 2), L.rsrl_hip_group_create(two, 0), L.rsrl_hip_group_create(two, -3), L.rsrl_hip_group_create(two, 2),
                L.rsrl_hip_group_create(nul, 2), L.rsrl_hip_group_train(None, 1, 3), L.rsrl_hip_group_train(two, 2, 2), L.rsrl_hip_group_train(nul, 2, 2),
                L.rsrl_hip_group_train(two, 1, -4)]
        rcs += [L.rsrl_hip_can_access_peer(-1, 0), L.rsrl_hip_can_access_peer(0, 99), L.rsrl_hip_device_identity(99, C.byref(ident)), L.rsrl_hip_device_identity(0, None),
                L.rsrl_hip_comm_info(h, None, None, None), L.rsrl_hip_comm_info(h, C.byref(ws), C.byref(rk), C.byref(ex)), L.rsrl_hip_comm_unique_id(None)]
        rcs.append(L.rsrl_hip_train(h, 2, None))
        L.rsrl_hip_sync(h)
        return rcs
    calls.append(ranks_bad)
    def newer_bad():                                   # the newer agents' entry points (REINFORCE's batches, LSTD's f64 state, the actor's theta, HIV's hidden state):
        T = int(rng.choice([1, 3]))                    # null arrays, non-finite values, learner indices out of range, lengths[i] > T, T < 0 -- on every ctx
        nonfin = float(rng.choice([np.nan, np.inf, -np.inf, 1e30]))
        sb = np.zeros((T, D, N), dtype=np.float32); ab = np.zeros((T, N), dtype=np.int32); rb = np.full((T, N), nonfin, dtype=np.float32)
        ln = rng.integers(0, T + 1, N).astype(np.uint32); ret = np.zeros((T, N), dtype=np.float32)
        over = ln.copy(); over[int(rng.integers(0, N))] = T + 1
        badact = ab.copy(); badact[0, int(rng.integers(0, N))] = int(rng.choice([-1, A, 2 ** 31 - 1]))
        rcs = [L.rsrl_hip_handle_batch(h, -1, p(sb), p(ab), p(rb), p(ln), p(ret)), L.rsrl_hip_handle_batch(h, -2 ** 40, None, None, None, p(ln), None),
               L.rsrl_hip_handle_batch(h, T, p(sb), p(ab), p(rb), p(over), p(ret)), L.rsrl_hip_handle_batch(h, T, p(sb), p(badact), p(rb), p(np.full(N, T, np.uint32)), None),
               L.rsrl_hip_handle_batch(h, T, None, p(ab), p(rb), p(ln), None), L.rsrl_hip_handle_batch(h, T, p(sb), p(ab), p(rb), None, None),
               L.rsrl_hip_handle_batch(h, 0, None, None, None, p(np.zeros(N, np.uint32)), None),
               L.rsrl_hip_handle_batch(h, T, p(sb), p(ab), p(rb), p(ln), p(ret))]
        th = np.full(F * A + 16, nonfin, dtype=np.float32)
        for j in (-1, N, 2 ** 40, 0):
            rcs += [L.rsrl_hip_get_policy_weights(h, j, p(big) if F * A <= big.size else None), L.rsrl_hip_get_behaviour_weights(h, j, p(big) if F * A <= big.size else None)]
        rcs += [L.rsrl_hip_get_policy_weights(h, 0, None), L.rsrl_hip_set_policy_weights(h, 0, None), L.rsrl_hip_set_policy_weights(h, N, p(th)),
                L.rsrl_hip_set_policy_weights(h, 0, p(th)), L.rsrl_hip_get_behaviour_weights(h, 0, None), L.rsrl_hip_set_behaviour_weights(h, -1, p(th)),
                L.rsrl_hip_set_behaviour_weights(h, N - 1, p(th)), L.rsrl_hip_set_behaviour_weights(h, 0, None)]
        g = np.full(N, nonfin, dtype=np.float32)
        rcs += [L.rsrl_hip_get_return_carry(h, None), L.rsrl_hip_set_return_carry(h, None), L.rsrl_hip_get_return_carry(h, p(g)), L.rsrl_hip_set_return_carry(h, p(g))]
        theta, mat, mu = np.full(F, nonfin), np.full((F, F), nonfin), np.full(F, nonfin)
        for j in (-1, N, 2 ** 40):
            rcs += [L.rsrl_hip_get_lstd_state(h, j, p(theta), p(mat), p(mu)), L.rsrl_hip_set_lstd_state(h, j, p(theta), p(mat), p(mu))]
        rcs += [L.rsrl_hip_get_lstd_state(h, 0, None, p(mat), None), L.rsrl_hip_get_lstd_state(h, 0, p(theta), None, None),
                L.rsrl_hip_set_lstd_state(h, 0, None, p(mat), None), L.rsrl_hip_set_lstd_state(h, 0, p(theta), None, p(mu)),
                L.rsrl_hip_set_lstd_state(h, N - 1, p(theta), p(mat), None if rng.random() < 0.5 else p(mu))]
        y = np.full((6, N), float(rng.choice([np.nan, np.inf, -1.0, 0.0, 1e300])), dtype=np.float64)
        rcs += [L.rsrl_hip_get_hidden_states(h, None), L.rsrl_hip_set_hidden_states(h, None), L.rsrl_hip_set_hidden_states(h, p(y))]
        rcs.append(L.rsrl_hip_train(h, 3, None))
        L.rsrl_hip_sync(h)
        return rcs
    calls.append(newer_bad)
    order = rng.permutation(len(calls))[: int(rng.integers(3, 12))]
    for j in order:
        rc = calls[int(j)]()
        log.append((int(j), rc if not isinstance(rc, tuple) else list(rc)))
    L.rsrl_hip_sync(h)


LATE = {"GradientMC": dict(domain=0, order=3, algo=23, policy=3, max_episode_steps=7, lr=0.01),
        "LSTD": dict(domain=0, order=2, algo=25, policy=3, max_episode_steps=7),
        "LSTDLambda": dict(domain=1, order=1, algo=26, policy=3, max_episode_steps=5, lam=0.8),
        "BetaActorCritic": dict(domain=4, order=3, algo=21, policy=4, n_steps=2, lr=0.02, alpha=0.2, max_episode_steps=9),
        "NAC": dict(domain=4, order=2, algo=28, policy=4, n_steps=3, lr=0.01, alpha=0.1, max_episode_steps=9)}


def late_agents_leg(L, rng):
    """the entry points of the five newest agents -- the *_f32 twins, handle_transitions, handle_batch on GradientMC, lstd_solve, nac_update, the
    episode-record accessors, policy_params, policy_pdf, set_lstd_batch_state, set_episode_steps -- with arguments the ABI's validation is documented
    to reject (null pointers, T < 0, a huge T with no arrays, lengths above T, non-finite f32 actions, batch sizes outside [1, n_envs], episode_steps
    above the cap, the int32 calls on the continuous domain and the f32 ones on a discrete one) or to accept (lengths of T rows above the cap, finite
    actions outside [0, 1], non-finite A / b / z, an all-zero mask, T = 0).  Every call returns; a refusal (rc != 0) moves nothing (checksum).
    -> (findings, {agent: [calls, refused]})"""
    bad, tally = [], {}
    p = lambda a: a.ctypes.data_as(C.c_void_p)       # noqa: E731
    for name, kw in LATE.items():
        N = int(rng.choice([5, 66]))
        with ra.Context(n_envs=N, seed=int(rng.integers(1 << 20)), env_offset=int(rng.choice([0, (1 << 31) - 3])), **kw) as c:
            h, D, F, cap, al = c._h, c.D, c.F, kw["max_episode_steps"], kw["algo"]
            c.reset()
            c.train(4, want_stats=False)
            nonfin = float(rng.choice([np.nan, np.inf, -np.inf]))
            T = 3
            S, R = np.zeros((T, D, N), np.float32), np.zeros((T, N), np.float32)
            S[:, 0, :] = -0.5
            Tm, ln, over = np.zeros((T, N), np.uint8), np.full(N, T, np.uint32), np.full(N, T, np.uint32)
            over[int(rng.integers(0, N))] = T + 1
            td, ai, out_i = np.zeros((cap + 3, N), np.float32), np.zeros(N, np.int32), np.zeros(N, np.int32)
            s1, af, r1, t1, o1, o2 = S[0].copy(), np.full(N, 0.5, np.float32), np.zeros(N, np.float32), np.zeros(N, np.uint8), np.zeros(N, np.float32), np.zeros(N, np.float32)
            a_nonfin, a_out = af.copy(), af.copy()
            a_nonfin[int(rng.integers(0, N))] = nonfin
            a_out[int(rng.integers(0, N))] = float(rng.choice([-3.0, 1.5, 1e30]))
            steps_over = np.zeros(N, np.uint32)
            steps_over[int(rng.integers(0, N))] = cap + 1
            Sl, Rl = np.zeros((cap + 3, D, N), np.float32), np.zeros((cap + 3, N), np.float32)
            Sl[:, 0, :] = -0.5
            theta, A, b, z, sing = np.zeros(F), np.full((F, F), nonfin), np.full(F, nonfin), np.full(F, nonfin), np.zeros(1, np.uint32)
            rec_s, rec_r = np.zeros((cap, D, N), np.float32), np.zeros((cap, N), np.float32)
            calls = [  # (what, the call, the codes it may return: None = any refusal, 0 = must succeed)
                ("handle_transitions T < 0", lambda: L.rsrl_hip_handle_transitions(h, -1, p(S), None, p(R), p(S), p(Tm), p(ln), None), None),
                ("handle_transitions huge T, no arrays", lambda: L.rsrl_hip_handle_transitions(h, 2 ** 40, None, None, None, None, None, p(ln), None), None),
                ("handle_transitions null lengths", lambda: L.rsrl_hip_handle_transitions(h, T, p(S), None, p(R), p(S), p(Tm), None, None), None),
                ("handle_transitions null rewards", lambda: L.rsrl_hip_handle_transitions(h, T, p(S), None, None, p(S), p(Tm), p(ln), None), None),
                ("handle_transitions lengths above T", lambda: L.rsrl_hip_handle_transitions(h, T, p(S), None, p(R), p(S), p(Tm), p(over), None), None),
                ("handle_batch T < 0", lambda: L.rsrl_hip_handle_batch(h, -7, p(S), None, p(R), p(ln), None), None),
                ("handle_batch huge T, no arrays", lambda: L.rsrl_hip_handle_batch(h, 2 ** 40, None, None, None, p(ln), None), None),
                ("handle_batch lengths above T", lambda: L.rsrl_hip_handle_batch(h, T, p(S), None, p(R), p(over), None), None),
                ("handle_batch null lengths", lambda: L.rsrl_hip_handle_batch(h, T, p(S), None, p(R), None, None), None),
                ("set_episode_steps above the cap", lambda: L.rsrl_hip_set_episode_steps(h, p(steps_over)), None if al in (23, 25, 26) else 0),
                ("set_episode_steps null", lambda: L.rsrl_hip_set_episode_steps(h, None), None),
                ("get_episode_record null", lambda: L.rsrl_hip_get_episode_record(h, None, p(rec_r)), None),
                ("set_episode_record null", lambda: L.rsrl_hip_set_episode_record(h, p(rec_s), None), None),
                ("get_lstd_batch_state out of range", lambda: L.rsrl_hip_get_lstd_batch_state(h, N, p(theta), p(A.copy()), p(b.copy()), None, p(sing)), None),
                ("set_lstd_batch_state null A", lambda: L.rsrl_hip_set_lstd_batch_state(h, 0, p(theta), None, p(b), None, p(sing)), None),
                ("set_lstd_batch_state index -1", lambda: L.rsrl_hip_set_lstd_batch_state(h, -1, p(theta), p(A), p(b), p(z), p(sing)), None),
                ("handle_f32 null actions", lambda: L.rsrl_hip_handle_f32(h, p(s1), None, p(r1), p(s1), p(t1), N, p(o1)), None),
                ("handle_f32 M = 0", lambda: L.rsrl_hip_handle_f32(h, p(s1), p(af), p(r1), p(s1), p(t1), 0, p(o1)), None),
                ("handle_f32 M > N", lambda: L.rsrl_hip_handle_f32(h, p(s1), p(af), p(r1), p(s1), p(t1), N + 1, p(o1)), None),
                ("handle_f32 non-finite action", lambda: L.rsrl_hip_handle_f32(h, p(s1), p(a_nonfin), p(r1), p(s1), p(t1), N, p(o1)), None),
                ("set_actions_f32 non-finite", lambda: L.rsrl_hip_set_actions_f32(h, p(a_nonfin)), None),
                ("set_actions_f32 out of bounds", lambda: L.rsrl_hip_set_actions_f32(h, p(a_out)), None),
                ("set_actions_f32 null", lambda: L.rsrl_hip_set_actions_f32(h, None), None),
                ("domain_step_f32 non-finite action", lambda: L.rsrl_hip_domain_step_f32(h, p(a_nonfin), p(s1.copy()), p(s1.copy()), p(r1), p(t1)), None),
                ("policy_sample_f32 null out", lambda: L.rsrl_hip_policy_sample_f32(h, p(s1), N, None), None),
                ("policy_sample_f32 own envs, M != N", lambda: L.rsrl_hip_policy_sample_f32(h, None, N - 1, p(o1)), None),
                ("policy_mode_f32 M < 0", lambda: L.rsrl_hip_policy_mode_f32(h, p(s1), -4, p(o1)), None),
                ("policy_params null states", lambda: L.rsrl_hip_policy_params(h, None, N, p(o1), p(o2)), None),
                ("policy_params null out", lambda: L.rsrl_hip_policy_params(h, p(s1), N, p(o1), None), None),
                ("policy_params M > N", lambda: L.rsrl_hip_policy_params(h, p(s1), N + 9, p(o1), p(o2)), None),
                ("policy_pdf non-finite action", lambda: L.rsrl_hip_policy_pdf(h, p(s1), p(a_nonfin), N, p(o1)), None),
                ("policy_pdf null actions", lambda: L.rsrl_hip_policy_pdf(h, p(s1), None, N, p(o1)), None),
                ("q_evaluate_f32 non-finite action", lambda: L.rsrl_hip_q_evaluate_f32(h, p(s1), p(a_nonfin), N, p(o1)), None),
                ("q_evaluate_f32 M = 0", lambda: L.rsrl_hip_q_evaluate_f32(h, p(s1), p(af), 0, p(o1)), None),
            ]
            if al in (21, 28):       # the int32 calls on the continuous domain
                calls += [("handle (int32)", lambda: L.rsrl_hip_handle(h, p(s1), p(ai), p(r1), p(s1), p(t1), N, p(o1)), None),
                          ("set_actions (int32)", lambda: L.rsrl_hip_set_actions(h, p(ai)), None), ("get_actions (int32)", lambda: L.rsrl_hip_get_actions(h, p(out_i)), None),
                          ("policy_sample (int32)", lambda: L.rsrl_hip_policy_sample(h, p(s1), N, p(out_i)), None),
                          ("domain_step (int32)", lambda: L.rsrl_hip_domain_step(h, p(ai), p(s1.copy()), p(s1.copy()), p(r1), p(t1)), None),
                          ("handle_transitions", lambda: L.rsrl_hip_handle_transitions(h, T, p(S), None, p(R), p(S), p(Tm), p(ln), None), None),
                          ("lstd_solve", lambda: L.rsrl_hip_lstd_solve(h), None), ("get_episode_record", lambda: L.rsrl_hip_get_episode_record(h, p(rec_s), p(rec_r)), None),
                          # ... and what it accepts: finite actions outside [0, 1] are clamped by the update, the score and the density
                          ("handle_f32 actions outside [0, 1]", lambda: L.rsrl_hip_handle_f32(h, p(s1), p(a_out), p(r1), p(s1), p(t1), N, p(o1)), 0),
                          ("policy_pdf actions outside [0, 1]", lambda: L.rsrl_hip_policy_pdf(h, p(s1), p(a_out), N, p(o1)), 0),
                          ("policy_params", lambda: L.rsrl_hip_policy_params(h, p(s1), N, p(o1), p(o2)), 0)]
            else:                    # ... and the f32 ones on a discrete one
                calls += [("handle_f32", lambda: L.rsrl_hip_handle_f32(h, p(s1), p(af), p(r1), p(s1), p(t1), N, p(o1)), None),
                          ("get_actions_f32", lambda: L.rsrl_hip_get_actions_f32(h, p(o1)), None), ("set_actions_f32", lambda: L.rsrl_hip_set_actions_f32(h, p(af)), None),
                          ("policy_sample_f32", lambda: L.rsrl_hip_policy_sample_f32(h, p(s1), N, p(o1)), None),
                          ("policy_params", lambda: L.rsrl_hip_policy_params(h, p(s1), N, p(o1), p(o2)), None),
                          ("policy_pdf", lambda: L.rsrl_hip_policy_pdf(h, p(s1), p(af), N, p(o1)), None),
                          ("q_evaluate_f32", lambda: L.rsrl_hip_q_evaluate_f32(h, p(s1), p(af), N, p(o1)), None),
                          ("nac_update", lambda: L.rsrl_hip_nac_update(h, None, p(o1)), None)]
            if al == 28:
                calls += [("nac_update, an all-zero mask", lambda: L.rsrl_hip_nac_update(h, p(np.zeros(N, np.uint8)), p(o1)), 0),
                          ("q_evaluate_f32 actions outside [0, 1]", lambda: L.rsrl_hip_q_evaluate_f32(h, p(s1), p(a_out), N, p(o1)), 0)]
            else:
                calls += [("nac_update", lambda: L.rsrl_hip_nac_update(h, None, p(o1)), None), ("q_evaluate_f32", lambda: L.rsrl_hip_q_evaluate_f32(h, p(s1), p(af), N, p(o1)), None)]
            if al == 23:
                calls += [("handle_batch, T rows above the cap", lambda: L.rsrl_hip_handle_batch(h, cap + 3, p(Sl), None, p(Rl), p(np.full(N, cap + 3, np.uint32)), p(td)), 0),
                          ("handle_batch T = 0", lambda: L.rsrl_hip_handle_batch(h, 0, None, None, None, p(np.zeros(N, np.uint32)), None), 0),
                          ("handle_transitions", lambda: L.rsrl_hip_handle_transitions(h, T, p(S), None, p(R), p(S), p(Tm), p(ln), None), None),
                          ("lstd_solve", lambda: L.rsrl_hip_lstd_solve(h), None)]
            if al in (25, 26):
                calls += [("handle_batch", lambda: L.rsrl_hip_handle_batch(h, T, p(S), None, p(R), p(ln), None), None),
                          ("handle_transitions, T rows above the cap", lambda: L.rsrl_hip_handle_transitions(h, cap + 3, p(Sl), None, p(Rl), p(Sl), p(np.zeros((cap + 3, N), np.uint8)),
                                                                                                       p(np.full(N, cap + 3, np.uint32)), p(td)), 0),
                          ("set_lstd_batch_state non-finite A, b, z", lambda: L.rsrl_hip_set_lstd_batch_state(h, N - 1, p(theta), p(A), p(b), p(z) if al == 26 else None, p(sing)), 0),
                          ("lstd_solve over a non-finite matrix", lambda: L.rsrl_hip_lstd_solve(h), 0),
                          ("handle_transitions onto a non-finite matrix", lambda: L.rsrl_hip_handle_transitions(h, T, p(S), None, p(R), p(S), p(Tm), p(ln), None), 0)]
            n_ref = 0
            order = list(rng.permutation(len(calls)))
            for j in order:
                what, call, want = calls[int(j)]
                before = c.checksum()
                rc = call()
                L.rsrl_hip_sync(h)
                if not isinstance(rc, int):
                    bad.append(f"{name}: {what} returned {rc!r}")
                elif want == 0 and rc != 0:
                    bad.append(f"{name}: {what} refused with {rc}: {(L.rsrl_hip_last_error() or b'').decode()[:80]}")
                elif want is None and rc == 0:
                    bad.append(f"{name}: {what} was accepted")
                if rc != 0:
                    n_ref += 1
                    if c.checksum() != before:
                        bad.append(f"{name}: {what} was refused ({rc}) and moved the ctx")
            if al in (25, 26):                                    # (in this order, whatever the permutation above made of it)
                rcs = [L.rsrl_hip_set_lstd_batch_state(h, N - 1, p(theta), p(A), p(b), p(z) if al == 26 else None, p(sing)), L.rsrl_hip_lstd_solve(h)]
                if rcs != [0, 0] or c.get_lstd_batch_state(N - 1)[4] != 1:
                    bad.append(f"{name}: the solve of a non-finite matrix was not counted as abandoned ({rcs})")
            rc = L.rsrl_hip_train(h, 3, None)                     # the ctx still trains (whatever it learnt from the garbage it accepted)
            L.rsrl_hip_sync(h)
            if rc != 0:
                bad.append(f"{name}: train after the leg: {rc}")
            tally[name] = [len(calls), n_ref]
    return bad, tally


def draw_config(L, rng):
    """a plausible base, then 0-4 fields pushed out of range"""
    cfg = _abi.Config()
    L.rsrl_hip_config_init(C.byref(cfg))
    cfg.n_envs = int(rng.choice([1, 3, 64, 300, 2000]))
    cfg.seed = int(rng.integers(0, 1 << 30))
    cfg.domain = int(rng.integers(0, 4)); cfg.basis = int(rng.integers(0, 2)); cfg.algo = int(rng.integers(0, 20)); cfg.policy = int(rng.integers(0, 4))
    cfg.order = int(rng.choice([1, 2, 3, 5, 7])); cfg.weight_mode = int(rng.random() < 0.25)
    if cfg.algo in (10, 11, 13, 15, 16, 18, 19) and rng.random() < 0.75:     # the actor-critics / REINFORCE (Gibbs: Softmax) and LSTD (Random) on their own ground
        cfg.policy, cfg.basis, cfg.weight_mode = (3 if cfg.algo >= 18 else 2), 0, 0
        cfg.order = int(rng.integers(1, 6)) if cfg.domain == 0 else 1
    if cfg.domain == 3 and cfg.algo not in (10, 11, 13, 15, 16, 18, 19) and rng.random() < 0.75:     # HIVTreatment: a one-step agent, Fourier order 1-3
        cfg.algo, cfg.basis, cfg.weight_mode, cfg.order = int(rng.choice([0, 1, 2, 5])), 0, 0, int(rng.integers(1, 4))
    for _ in range(int(rng.integers(0, 5))):
        k = rng.integers(0, 4)
        if k == 0:
            name = str(rng.choice(list(INT_FIELDS)))
            setattr(cfg, name, int(rng.choice(INT_FIELDS[name])))
        elif k == 1:
            setattr(cfg, str(rng.choice(F_FIELDS)), float(rng.choice(BAD_F)))
        elif k == 2:
            cfg.n_envs = int(rng.choice([0, -1, -2 ** 40, 2 ** 62, 1]))
        else:
            name = str(rng.choice(["env_offset", "max_episode_steps", "steps_per_launch", "struct_size"]))
            val = {"env_offset": [-1, 2 ** 40, 2 ** 32 - 1], "max_episode_steps": [0, 1, 2 ** 32 - 1], "steps_per_launch": [0, 1, 2 ** 32 - 1, 3],
                   "struct_size": [0, 4, 17, 10 ** 6, C.sizeof(_abi.Config) - 8]}[name]
            setattr(cfg, name, int(rng.choice(val)))
    # never ask for more than ~2 GB: a table of F*A floats (twice with an auxiliary matrix) per learner
    dims = {0: 2, 3: 6}.get(cfg.domain, 4)
    feats = (max(1, min(8, cfg.order)) + 1) ** dims if cfg.basis == 0 else max(1, min(16, cfg.n_tilings)) * max(1, min(64, cfg.tiles_per_dim)) ** dims
    per_learner = feats * 4 * 4 * 2 + (feats * feats * 8 if cfg.algo in (18, 19) else 0)      # (RecursiveLSTD / iLSTD: an f64 F x F matrix each)
    if 0 < cfg.n_envs <= 10 ** 7 and cfg.weight_mode == 0 and per_learner * cfg.n_envs > 2e9:
        cfg.n_envs = max(1, int(2e9 / per_learner))
    if cfg.peer_timeout_ms == 0 or cfg.peer_timeout_ms > 300:
        cfg.peer_timeout_ms = 200                               # (a rank whose peers never show up gives up after 0.2 s instead of the default 4 s)
    return cfg


def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    rng = np.random.default_rng(seed)
    L = _abi.lib()
    ref = healthy_checksum()
    created = refused = 0
    for idx in range(n_cases):
        cfg = draw_config(L, rng)
        h = C.c_void_p()
        rc = L.rsrl_hip_create(C.byref(cfg), C.byref(h))
        log = []
        if rc == 0 and h:
            created += 1
            poke(L, h, rng, log)
            L.rsrl_hip_destroy(h)
        else:
            refused += 1
            msg = L.rsrl_hip_last_error()
            assert msg and len(msg) > 3, (idx, rc)
        now = healthy_checksum()
        ok = now == ref
        print(f"{idx:4d} create rc {rc:3d} {'poked ' + str(len(log)) if rc == 0 else 'refused'}  healthy {'ok' if ok else 'CHANGED'}", flush=True)
        if not ok:
            print("SUMMARY " + json.dumps({"cases": idx + 1, "failed_at": idx, "log": log}), flush=True)
            sys.exit(1)
    # the five newest agents' entry points, then the healthy ctx once more
    failures, late = late_agents_leg(L, rng)
    if healthy_checksum() != ref:
        failures.append("the healthy ctx changed after the late agents' leg")
    for f in failures:
        print("LATE " + f, flush=True)
    # null handles
    for fn in ("rsrl_hip_reset", "rsrl_hip_sync", "rsrl_hip_destroy"):
        getattr(L, fn)(None)
    print("SUMMARY " + json.dumps({"cases": n_cases, "seed": seed, "created": created, "refused": refused, "late": late, "failures": failures}), flush=True)
    sys.exit(1 if failures else 0)


if __name__ == "__main__":
    main()
