"""Array arguments may be HOST or DEVICE pointers (include/rsrl_hip.h, conventions): device pointers are used in place and the call is asynchronous on the
ctx's stream.  Every entry point that takes arrays, with raw hipMalloc buffers (rsrl_amd/_devmem.py: the HIP runtime through ctypes, what a Rust caller's hip-sys binding hands over --
no torch: its first GPU use costs a cold box minutes), against the same call with host arrays on a twin ctx -- bit for bit."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import rsrl_amd as ra
from rsrl_amd._devmem import DeviceBuffer
from tests.agent_contract import assert_same, snapshot

pytestmark = pytest.mark.gpu

CASES = {
    "reg": dict(domain=0, order=5, algo=0, policy=1, epsilon=0.2, gamma=0.9, lr=0.001, n_envs=96, seed=3, max_episode_steps=60),
    "tile_shared": dict(domain=1, basis=1, n_tilings=8, tiles_per_dim=8, algo=1, policy=1, epsilon=0.1, gamma=0.99, lr=0.1 / 8 / 96, weight_mode=1, n_envs=96, seed=3,
                        max_episode_steps=60),
    "wave_bf16": dict(domain=2, order=7, algo=2, policy=2, tau=1.0, gamma=0.99, lr=2.5e-4, alpha=1.0, weight_dtype=1, n_envs=8, seed=3, max_episode_steps=60),
    "generic_tdl": dict(domain=1, order=2, algo=8, policy=3, gamma=0.9, lam=0.5, trace=1, n_envs=96, seed=3, max_episode_steps=60),
    "lambda_tile": dict(domain=0, basis=1, n_tilings=4, tiles_per_dim=8, algo=3, policy=1, epsilon=0.2, gamma=0.99, alpha=0.02, lam=0.8, n_envs=16, seed=3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_device_pointer_arguments_equal_host_arguments(name):
    import rsrl_amd as ra
    from rsrl_amd._devmem import DeviceBuffer
    kw = CASES[name]
    with ra.Context(**kw) as h, ra.Context(**kw) as d:
        L = d._L
        N, D, A, F, O = d.N, d.D, d.A, d.F, d.n_out
        ptr = lambda b: C.c_void_p(b.ptr)       # noqa: E731
        f32, i32, u8 = np.float32, np.int32, np.uint8

        def like(b, host):                         # a fresh device buffer holding `host`
            n = DeviceBuffer(b.count, b.dtype); n.from_host(host)
            return n
        ok = lambda rc: ra._abi.check(rc)               # noqa: E731
        for c in (h, d):
            c.reset()
            c.train(25, want_stats=False)
        # get_states / get_actions / episode steps into device memory
        ds = DeviceBuffer(D * N, f32); da = DeviceBuffer(N, i32)
        de = DeviceBuffer(N, i32)
        ok(L.rsrl_hip_get_states(d._h, ptr(ds))); ok(L.rsrl_hip_get_actions(d._h, ptr(da))); ok(L.rsrl_hip_get_episode_steps(d._h, ptr(de)))
        d.sync()
        assert np.array_equal(ds.to_host((D, N)), h.states) and np.array_equal(da.to_host(), h.actions)
        assert np.array_equal(de.to_host().view(np.uint32), h.episode_steps)
        # q_evaluate / policy_mode on device states, device outputs
        dq = DeviceBuffer(O * N, f32)
        ok(L.rsrl_hip_q_evaluate(d._h, ptr(ds), N, ptr(dq)))
        d.sync()
        assert np.array_equal(dq.to_host((O, N)), h.q_evaluate(h.states), equal_nan=True)
        if kw["algo"] not in (7, 8):
            dm = DeviceBuffer(N, i32)
            ok(L.rsrl_hip_policy_mode(d._h, ptr(ds), N, ptr(dm)))
            d.sync()
            assert np.array_equal(dm.to_host(), h.policy_mode(h.states))
        # domain_step with device outputs, then handle with device inputs (sparse / shared-trace agents aside, every agent has a handle)
        frm_h, nxt_h, rew_h, term_h = h.domain_step(h.actions)
        dfrm = DeviceBuffer(D * N, f32); dnxt = DeviceBuffer(D * N, f32)
        drew = DeviceBuffer(N, f32); dterm = DeviceBuffer(N, u8)
        ok(L.rsrl_hip_domain_step(d._h, ptr(da), ptr(dfrm), ptr(dnxt), ptr(drew), ptr(dterm)))
        d.sync()
        assert np.array_equal(dnxt.to_host((D, N)), nxt_h) and np.array_equal(drew.to_host(), rew_h) and np.array_equal(dterm.to_host(), term_h)
        td_h = h.handle(frm_h, h.actions, rew_h, nxt_h, term_h)
        dtd = DeviceBuffer(N, f32)
        ok(L.rsrl_hip_handle(d._h, ptr(dfrm), ptr(da), ptr(drew), ptr(dnxt), ptr(dterm), N, ptr(dtd)))
        d.sync()
        assert np.array_equal(dtd.to_host(), td_h, equal_nan=True)
        # get_weights / set_weights through device memory: learner 0 (or the shared approximator)
        dw = DeviceBuffer(F * O, f32)
        ok(L.rsrl_hip_get_weights(d._h, 0, ptr(dw)))
        d.sync()
        assert np.array_equal(dw.to_host((F, O)), h.get_weights(0))
        w2_h = dw.to_host((F, O)) * np.float32(0.5)
        w2 = like(dw, w2_h)
        ok(L.rsrl_hip_set_weights(d._h, 0, ptr(w2)))
        h.set_weights(w2_h, 0)
        assert np.array_equal(d.get_weights(0), h.get_weights(0))
        # set_states from device memory: the array is checked ON the device by the host path's rule (ABI 9; it used to be clamped silently, NaN passing) --
        # a non-finite / far-out-of-range component refuses the call and leaves the ctx's states untouched; set_actions clamps a device array (no host copy)
        before = d.states
        for bad in (float("inf"), float("nan"), 1e30):
            bad_h = ds.to_host((D, N)); bad_h[0, 0] = bad
            bad_s = like(ds, bad_h)
            assert L.rsrl_hip_set_states(d._h, ptr(bad_s)) == -1 and b"device array of states" in L.rsrl_hip_last_error()
            assert np.array_equal(d.states, before)
        bad_h = da.to_host(); bad_h[0] = 77
        bad_a = like(da, bad_h)
        ok(L.rsrl_hip_set_actions(d._h, ptr(bad_a)))
        d.sync()
        assert 0 <= d.actions[0] < A
        ok(L.rsrl_hip_set_states(d._h, ptr(dnxt))); ok(L.rsrl_hip_set_actions(d._h, ptr(da)))
        h.states, h.actions = nxt_h, h.actions
        for c in (h, d):
            c.train(20, want_stats=False)
        assert np.array_equal(d.states, h.states) and np.array_equal(d.get_weights(0), h.get_weights(0), equal_nan=True)
        # greedy rollout with device outputs
        if kw["algo"] not in (7, 8):
            dn = DeviceBuffer(N, i32); dt = DeviceBuffer(N, f32)
            ok(L.rsrl_hip_rollout_greedy(d._h, 40, ptr(dn), ptr(dt)))
            d.sync()
            n_h, t_h = h.rollout_greedy(40)
            assert np.array_equal(dn.to_host().view(np.uint32), n_h) and np.array_equal(dt.to_host(), t_h)


# ---- the entry points of the newer agents, mixed host / device arguments in one call, and the contract for host inputs.  Same style: twin ctxs,
# `h` called with host arrays and `d` with raw DeviceBuffers, compared bit for bit after sync().  96 learners, Fourier order 3, each agent's
# configuration as its own test module admits it.
F32, I32, U8, U32 = np.float32, np.int32, np.uint8, np.uint32
T_ROWS = 3
CMC = ra.CONTINUOUS_MOUNTAIN_CAR
AGENTS = {
    "reinforce": dict(domain=ra.MOUNTAIN_CAR, order=3, algo=ra.REINFORCE, policy=ra.SOFTMAX, n_envs=96, seed=5, gamma=0.95, alpha=0.05, tau=1.0, max_episode_steps=19),
    "gmc": dict(domain=ra.MOUNTAIN_CAR, order=3, algo=ra.GRADIENT_MC, policy=ra.RANDOM, n_envs=96, seed=0, gamma=0.95, lr=0.01, max_episode_steps=7),
    "lstd": dict(domain=ra.MOUNTAIN_CAR, order=3, algo=ra.LSTD, policy=ra.RANDOM, n_envs=96, seed=5, gamma=0.95, max_episode_steps=7, lam=0.8),
    "tdac_beta": dict(domain=CMC, order=3, algo=ra.ILSTD_ACTOR_CRITIC, policy=ra.BETA, n_envs=96, seed=5, gamma=0.95, lr=0.05, alpha=0.3, n_steps=3, max_episode_steps=19),
    "nac": dict(domain=CMC, order=3, algo=ra.NAC, policy=ra.BETA, n_envs=96, seed=5, gamma=0.95, lr=0.01, alpha=0.1, n_steps=100, max_episode_steps=19),
}


def ptr(b):
    return C.c_void_p(b.ptr)


def hp(a):                                      # a host array's address, as the wrapper passes it
    assert a.flags.c_contiguous
    return a.ctypes.data_as(C.c_void_p)


def dev(host, dtype):
    b = DeviceBuffer(np.size(host), dtype)
    b.from_host(host)
    return b


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: U32, 1: U8}[a.dtype.itemsize])


def ok(rc):
    ra._abi.check(rc)


@contextlib.contextmanager
def twins(kw, warm=25):
    """(h, d): two ctxs of the same configuration after the same reset and `warm` batch-steps of train"""
    with ra.Context(**kw) as h, ra.Context(**kw) as d:
        for c in (h, d):
            c.reset()
            c.train(warm, want_stats=False)
        yield h, d


def rand_states(c, M, rng):
    lo, hi = c.state_bounds()
    return np.ascontiguousarray(rng.uniform(lo, hi, size=(M, c.D)).T.astype(F32))


def ragged_batch(c, rng, actions=True):
    """T_ROWS rows for every learner, lengths 0 .. 3 among them: states / to-states (T, D, N), actions, rewards, terminal flags (T, N), lengths (N,)"""
    N = c.N
    S = np.stack([rand_states(c, N, rng) for _ in range(T_ROWS)])
    S2 = np.stack([rand_states(c, N, rng) for _ in range(T_ROWS)])
    A_ = rng.integers(0, c.A, size=(T_ROWS, N)).astype(I32) if actions else None
    R = rng.normal(0.0, 1.0, size=(T_ROWS, N)).astype(F32)
    Tm = (rng.random((T_ROWS, N)) < 0.2).astype(U8)
    L = (np.arange(N) % (T_ROWS + 1)).astype(U32)
    return S, S2, A_, R, Tm, L


def same_learners(h, d, what):
    d.sync()
    assert_same(snapshot(d), snapshot(h), what)


@pytest.mark.parametrize("name", ["reinforce", "gmc"])
def test_handle_batch_device_arrays_and_host_inputs_overwritten_on_return(name):
    rng = np.random.default_rng(11)
    with twins(AGENTS[name]) as (h, d):
        N, D = h.N, h.D
        S, _, A_, R, _, L = ragged_batch(h, rng)
        dS, dA, dR, dL, dG = dev(S, F32), dev(A_, I32), dev(R, F32), dev(L, U32), DeviceBuffer(T_ROWS * N, F32)
        d.handle_batch(dS.ptr, dA.ptr, dR.ptr, dL.ptr, returns=dG.ptr, T=T_ROWS)
        ret_h = h.handle_batch(S, A_, R, L, returns=True)
        # the contract for host inputs: they have been read when the call returns
        S.fill(np.nan); R.fill(np.nan); A_.fill(0x7fc00000); L.fill(0xffffffff)
        d.sync()
        assert np.array_equal(bits(dG.to_host((T_ROWS, N))), bits(ret_h)), "returns_out in device memory"
        assert np.isnan(ret_h[:, 0]).all() and not np.isnan(ret_h[:, 3::4]).any()      # (lengths 0 and 3: nothing / every row handled)
        same_learners(h, d, name + " after handle_batch")
        if name == "gmc":                        # the open episodes into device memory
            cap = int(h.cfg.max_episode_steps)
            dRS, dRR = DeviceBuffer(cap * D * N, F32), DeviceBuffer(cap * N, F32)
            ok(d._L.rsrl_hip_get_episode_record(d._h, ptr(dRS), ptr(dRR)))
            d.sync()
            rs_h, rr_h = h.episode_record
            assert h.episode_steps.any()
            assert np.array_equal(bits(dRS.to_host((cap, D, N))), bits(rs_h)) and np.array_equal(bits(dRR.to_host((cap, N))), bits(rr_h))


def test_lstd_handle_transitions_device_arrays_then_solve():
    rng = np.random.default_rng(12)
    with twins(AGENTS["lstd"]) as (h, d):
        N = h.N
        S, S2, _, R, Tm, L = ragged_batch(h, rng, actions=False)
        dTD = DeviceBuffer(T_ROWS * N, F32)
        bufs = [dev(S, F32), dev(R, F32), dev(S2, F32), dev(Tm, U8), dev(L, U32)]
        d.handle_transitions(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, td=dTD.ptr, T=T_ROWS)
        td_h = h.handle_transitions(S, R, S2, Tm, L, td=True)
        d.sync()
        assert np.array_equal(bits(dTD.to_host((T_ROWS, N))), bits(td_h)), "td_out in device memory"
        assert not np.isnan(td_h[:, 3::4]).any()
        for c in (h, d):
            c.lstd_solve()
        same_learners(h, d, "lstd after handle_transitions and solve")


def test_beta_actor_critic_f32_entry_points_on_device_arrays():
    rng = np.random.default_rng(13)
    with twins(AGENTS["tdac_beta"]) as (h, d):
        L, N, D = d._L, d.N, d.D
        # domain_step_f32 on the pending actions read into device memory, every output on the device
        da = DeviceBuffer(N, F32)
        ok(L.rsrl_hip_get_actions_f32(d._h, ptr(da)))
        act_h = h.actions
        frm_h, nxt_h, rew_h, term_h = h.domain_step(act_h)
        dfrm, dnxt, drew, dterm = DeviceBuffer(D * N, F32), DeviceBuffer(D * N, F32), DeviceBuffer(N, F32), DeviceBuffer(N, U8)
        ok(L.rsrl_hip_domain_step_f32(d._h, ptr(da), ptr(dfrm), ptr(dnxt), ptr(drew), ptr(dterm)))
        d.sync()
        assert np.array_equal(da.to_host(), act_h) and np.array_equal(dfrm.to_host((D, N)), frm_h) and np.array_equal(dnxt.to_host((D, N)), nxt_h)
        assert np.array_equal(drew.to_host(), rew_h) and np.array_equal(dterm.to_host(), term_h)
        # handle_f32 on exactly those arrays
        dtd = DeviceBuffer(N, F32)
        ok(L.rsrl_hip_handle_f32(d._h, ptr(dfrm), ptr(da), ptr(drew), ptr(dnxt), ptr(dterm), N, ptr(dtd)))
        td_h = h.handle(frm_h, act_h, rew_h, nxt_h, term_h)
        d.sync()
        assert np.array_equal(bits(dtd.to_host()), bits(td_h))
        # the policy side: sample (explicit states, then the ctx's own), mode, the shape parameters, the density
        X = rand_states(h, N, rng)
        dX, do0, do1 = dev(X, F32), DeviceBuffer(N, F32), DeviceBuffer(N, F32)
        ok(L.rsrl_hip_policy_sample_f32(d._h, ptr(dX), N, ptr(do0)))
        d.sync()
        smp_h = h.policy_sample(X)
        assert np.array_equal(bits(do0.to_host()), bits(smp_h))
        ok(L.rsrl_hip_policy_sample_f32(d._h, None, N, ptr(do0)))
        d.sync()
        assert np.array_equal(bits(do0.to_host()), bits(h.policy_sample())) and np.array_equal(bits(d.actions), bits(h.actions))
        ok(L.rsrl_hip_policy_mode_f32(d._h, ptr(dX), N, ptr(do0)))
        d.sync()
        assert np.array_equal(bits(do0.to_host()), bits(h.policy_mode(X)))
        ok(L.rsrl_hip_policy_params(d._h, ptr(dX), N, ptr(do0), ptr(do1)))
        d.sync()
        al_h, be_h = h.policy_params(X)
        assert np.array_equal(bits(do0.to_host()), bits(al_h)) and np.array_equal(bits(do1.to_host()), bits(be_h))
        dsm = dev(smp_h, F32)
        ok(L.rsrl_hip_policy_pdf(d._h, ptr(dX), ptr(dsm), N, ptr(do0)))
        d.sync()
        assert np.array_equal(bits(do0.to_host()), bits(h.policy_pdf(X, smp_h)))
        same_learners(h, d, "the Beta iLSTD ActorCritic")


def test_nac_entry_points_on_device_arrays():
    rng = np.random.default_rng(14)
    with twins(AGENTS["nac"]) as (h, d):
        L, N = d._L, d.N
        X, a = rand_states(h, N, rng), rng.uniform(0.0, 1.0, size=N).astype(F32)
        dX, da, dq = dev(X, F32), dev(a, F32), DeviceBuffer(N, F32)
        ok(L.rsrl_hip_q_evaluate_f32(d._h, ptr(dX), ptr(da), N, ptr(dq)))
        d.sync()
        assert np.array_equal(bits(dq.to_host()), bits(h.q_evaluate_f32(X, a)))
        mask = (np.arange(N) % 3 != 0).astype(U8)
        dm, dn = dev(mask, U8), DeviceBuffer(N, F32)
        ok(L.rsrl_hip_nac_update(d._h, ptr(dm), ptr(dn)))
        d.sync()
        norm_h = h.nac_update(mask)
        assert np.array_equal(bits(dn.to_host()), bits(norm_h)) and not norm_h[::3].any() and norm_h[1::3].any()
        dns, dt = DeviceBuffer(N, U32), DeviceBuffer(N, F32)
        ok(L.rsrl_hip_rollout_greedy(d._h, 40, ptr(dns), ptr(dt)))
        d.sync()
        n_h, t_h = h.rollout_greedy(40)
        assert np.array_equal(dns.to_host(), n_h) and np.array_equal(bits(dt.to_host()), bits(t_h))
        same_learners(h, d, "NAC")


def test_reg_trajectory_outputs_and_qop_inputs_on_the_device():
    rng = np.random.default_rng(15)
    with twins(CASES["reg"]) as (h, d):
        L, N, D, A = d._L, d.N, d.D, d.A
        SL = 5
        dn, dt, dst = DeviceBuffer(N, U32), DeviceBuffer(N, F32), DeviceBuffer(SL * D * N, F32)
        dac, drw, dtm = DeviceBuffer((SL - 1) * N, I32), DeviceBuffer((SL - 1) * N, F32), DeviceBuffer(N, U8)
        ok(L.rsrl_hip_rollout_trajectory(d._h, SL, N, ptr(dn), ptr(dt), ptr(dst), ptr(dac), ptr(drw), ptr(dtm)))
        d.sync()
        tr = h.rollout_trajectory(SL)
        assert np.array_equal(dn.to_host(), tr["n_states"]) and np.array_equal(bits(dt.to_host()), bits(tr["total_reward"]))
        assert np.array_equal(bits(dst.to_host((SL, D, N))), bits(tr["states"])) and np.array_equal(dac.to_host((SL - 1, N)), tr["actions"])
        assert np.array_equal(bits(drw.to_host((SL - 1, N))), bits(tr["rewards"])) and np.array_equal(dtm.to_host(), tr["terminal"])
        # the two inputs of the Q operations besides the states: probabilities (f32), actions (int32)
        X = rand_states(h, N, rng)
        P = rng.dirichlet(np.ones(A), size=N).T.astype(F32)
        acts = rng.integers(0, A, size=N).astype(I32)
        dX, dP, dacts, dout = dev(X, F32), dev(P, F32), dev(acts, I32), DeviceBuffer(N, F32)
        ok(L.rsrl_hip_q_expected_value(d._h, ptr(dX), N, ptr(dP), ptr(dout)))
        d.sync()
        assert np.array_equal(bits(dout.to_host()), bits(h.q_expected_value(X, P)))
        ok(L.rsrl_hip_policy_prob(d._h, ptr(dX), ptr(dacts), N, ptr(dout)))
        d.sync()
        assert np.array_equal(bits(dout.to_host()), bits(h.policy_prob(X, acts)))


def test_handle_with_host_and_device_arguments_in_one_call():
    """every pointer of a call is placed on its own: host actions and rewards next to device states, flags and td_out; device inputs next to a host
    td_out.  And the contract for host inputs: overwritten the moment the call returns, they have been read"""
    with twins(CASES["reg"]) as (h, d):
        L, N = d._L, d.N
        for mixed in ("host actions and rewards", "host td_out"):
            act = h.actions
            frm, nxt, rew, term = h.domain_step(act)
            got = d.domain_step(act)
            assert all(np.array_equal(x, y) for x, y in zip(got, (frm, nxt, rew, term)))
            dfrm, dnxt, dterm = dev(frm, F32), dev(nxt, F32), dev(term, U8)
            if mixed == "host td_out":
                dact, drew, td_d = dev(act, I32), dev(rew, F32), np.full(N, np.nan, dtype=F32)
                ok(L.rsrl_hip_handle(d._h, ptr(dfrm), ptr(dact), ptr(drew), ptr(dnxt), ptr(dterm), N, hp(td_d)))
            else:
                act_d, rew_d, dtd = act.copy(), rew.copy(), DeviceBuffer(N, F32)
                ok(L.rsrl_hip_handle(d._h, ptr(dfrm), hp(act_d), hp(rew_d), ptr(dnxt), ptr(dterm), N, ptr(dtd)))
                act_d.fill(0x7fc00000); rew_d.fill(np.nan)
                d.sync()
                td_d = dtd.to_host()
            td_h = np.empty(N, dtype=F32)
            ok(L.rsrl_hip_handle(h._h, hp(frm), hp(act), hp(rew), hp(nxt), hp(term), N, hp(td_h)))
            frm.fill(np.nan); nxt.fill(np.nan); rew.fill(np.nan); act.fill(0x7fc00000); term.fill(0xff)
            assert np.array_equal(bits(td_d), bits(td_h)), mixed
            same_learners(h, d, mixed)
            for c in (h, d):
                c.domain_reset(); c.policy_sample()
