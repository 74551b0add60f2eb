"""GradientMC (RSRL_GRADIENT_MC; train_gmc.hip) on the device: handle_batch bit for bit against the backward chain of the oracle's TD terminal update in
device order (tests/gmc_numpy.py td_chain, "f32d"), length-1 trajectories against an RSRL_TD ctx's handle, train against the host trait loop / launch
depths / shards bit for bit with the per-learner episode record among what is compared, the environment side against RSRL_TD's, checkpoints with
the open record carried by the caller, the refusals and the C++ example.  N = 260 throughout: one full block of 256 learners and a ragged second."""
import os

import numpy as np
import pytest

import rsrl_amd as ra
from rsrl_amd import RsrlHipError
from rsrl_amd._devmem import DeviceBuffer
from tests.agent_contract import (assert_same, check_foreign_checkpoints_refused, check_train_invariance, gmc_trait_loop, rand_states, run_example,
                                  snapshot)
from tests.gmc_numpy import f32_returns, td_chain

pytestmark = pytest.mark.gpu

N = 260
PAIRS = [(ra.MOUNTAIN_CAR, 1), (ra.MOUNTAIN_CAR, 2), (ra.MOUNTAIN_CAR, 3), (ra.MOUNTAIN_CAR, 5), (ra.CART_POLE, 1), (ra.ACROBOT, 1)]
EINVAL, ESTATE = -1, -5
BASE = dict(domain=ra.MOUNTAIN_CAR, order=3, algo=ra.GRADIENT_MC, policy=ra.RANDOM, n_envs=N, seed=0, gamma=0.95, lr=0.01, max_episode_steps=7)
# (a) every end is a truncation; (b) ragged ends inside one wave, terminal and truncated
CASE_A = dict(domain=ra.MOUNTAIN_CAR, order=3, max_episode_steps=7)
CASE_B = dict(domain=ra.CART_POLE, order=1, max_episode_steps=40)


def ctx(**kw):
    return ra.Context(**dict(BASE, **kw))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def assert_same_record(a, b, what):
    """two records as the accessor shows them, bit for bit (the harness's assert_same refuses any NaN; a record has NaN past each learner's rows)"""
    assert list(a) == list(b) == ["record_states", "record_rewards"], what
    for n in a:
        assert a[n].shape == b[n].shape and np.array_equal(bits(a[n]), bits(b[n])), "%s: %s differ" % (what, n)


def all_weights(c):
    return np.stack([c.get_weights(i)[:, 0] for i in range(c.N)])


def set_all_weights(c, W):
    for i in range(c.N):
        c.set_weights(W[i].reshape(c.F, 1), i)


@pytest.mark.parametrize("domain,order", PAIRS)
def test_handle_batch_is_the_device_order_chain_bit_for_bit(orc, domain, order):
    T, gamma, lr = 7, 0.95, 0.01
    rng = np.random.default_rng(100 * domain + order)
    ag = orc.make_agent(domain=domain, order=order, algo=orc.TD, policy=orc.RANDOM, gamma=gamma, lr=lr)
    with ctx(domain=domain, order=order, gamma=gamma, lr=lr) as c:
        F, D = c.F, c.D
        W0 = rng.normal(0.0, 0.3, size=(N, F)).astype(np.float32)
        S = np.stack([rand_states(orc, domain, N, rng) for _ in range(T)])
        R = rng.normal(0.0, 1.0, size=(T, N)).astype(np.float32)
        L = np.array([0, 1, 2, 7], dtype=np.uint32)[np.arange(N) % 4]
        # the reference, once: learner i's backward chain over its rows, the return formed in f32
        want_w, want_ret = W0.copy(), np.full((T, N), np.nan, dtype=np.float32)
        for i in range(N):
            n = int(L[i])
            _, rets = td_chain(orc, ag, want_w[i], S[:n, :, i], R[:n, i], gamma, "f32d")
            want_ret[:n, i] = rets
            assert np.array_equal(bits(rets), bits(f32_returns(R[:n, i], gamma)))
        assert np.array_equal(bits(want_w[L == 0]), bits(W0[L == 0])) and not np.array_equal(want_w[L == 7], W0[L == 7])

        # ---- host arrays (actions given: not read)
        set_all_weights(c, W0)
        t0 = c.step_count
        ret = c.handle_batch(S, rng.integers(0, c.A, size=(T, N)).astype(np.int32), R, L, returns=True)
        assert c.step_count == t0 + 1
        assert np.array_equal(bits(ret), bits(want_ret)), "returns_out (host arrays)"
        got = all_weights(c)
        assert np.array_equal(bits(got), bits(want_w)), np.flatnonzero((bits(got) != bits(want_w)).any(axis=1))[:8]
        with pytest.raises(RsrlHipError) as e:                     # a host length above T is refused, nothing moves
            c.handle_batch(S, None, R, np.where(L == 7, 10, L).astype(np.uint32))
        assert e.value.code == EINVAL and np.array_equal(bits(all_weights(c)), bits(want_w))

        # ---- device arrays, no actions, a length of 10 where the host's said 7: clamped to T
        set_all_weights(c, W0)
        dS, dR = DeviceBuffer(T * D * N, np.float32), DeviceBuffer(T * N, np.float32)
        dL, dG = DeviceBuffer(N, np.uint32), DeviceBuffer(T * N, np.float32)
        dS.from_host(S); dR.from_host(R); dL.from_host(np.where(L == 7, 10, L).astype(np.uint32))
        c.handle_batch(dS.ptr, None, dR.ptr, dL.ptr, returns=dG.ptr, T=T)
        c.sync()
        assert np.array_equal(bits(dG.to_host((T, N))), bits(want_ret)), "returns_out (device arrays)"
        assert np.array_equal(bits(all_weights(c)), bits(want_w))
        # the ctx's own open record and episode steps are not touched
        assert not c.episode_steps.any() and np.isnan(c.episode_record[1]).all()
        for b in (dS, dR, dL, dG):
            b.free()


@pytest.mark.parametrize("domain,order", PAIRS)
def test_length_one_trajectories_are_tds_terminal_transitions(orc, domain, order):
    rng = np.random.default_rng(7 + 10 * domain + order)
    kw = dict(domain=domain, order=order, gamma=0.9, lr=0.02)
    with ctx(**kw) as c, ctx(algo=ra.TD, **kw) as t:
        W0 = rng.normal(0.0, 0.3, size=(N, c.F)).astype(np.float32)
        set_all_weights(c, W0)
        set_all_weights(t, W0)
        S, R = rand_states(orc, domain, N, rng), rng.normal(0.0, 1.0, size=N).astype(np.float32)
        ret = c.handle_batch(S[None], None, R[None], np.ones(N, dtype=np.uint32), returns=True)
        td = t.handle(S, np.zeros(N, dtype=np.int32), R, rand_states(orc, domain, N, rng), np.ones(N, dtype=np.uint8))
        assert np.array_equal(bits(ret[0]), bits(R))
        assert np.array_equal(bits(all_weights(c)), bits(all_weights(t)))
        assert np.abs(td).max() > 0 and not np.array_equal(all_weights(c), W0)


class Recording(ra.Context):
    """a Context that leaves its episode record (as the accessor shows it: NaN past each learner's episode_steps) behind when its `with` ends: the
    contract harness's snapshot does not read it"""
    log = []

    def __exit__(self, *exc):
        if exc[0] is None:
            s, r = self.episode_record
            Recording.log.append(dict(record_states=s, record_rewards=r))
        return super().__exit__(*exc)


@pytest.mark.parametrize("case,K,first_split", [(CASE_A, 50, 10), (CASE_B, 120, 33)], ids=["mountain-car-truncations", "cart-pole-ragged"])
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(case, K, first_split):
    cap = case["max_episode_steps"]
    Recording.log = []
    st, ref = check_train_invariance(lambda **kw: Recording(**dict(BASE, **kw)), dict(case, n_envs=N), K, cap, depths=(1, 16), first_split=first_split,
                                     kernel="k_train_gmc", trait=gmc_trait_loop)
    print("statistics", st)
    assert st["env_steps"] == N * K and st["episodes"] > 0
    if case is CASE_B:
        assert st["episodes"] - st["episodes_truncated"] > 0
    else:
        assert st["episodes"] == st["episodes_truncated"] and (ref["episode_steps"] == K % cap).all()      # one open row is left at the end
    assert np.isfinite(ref["weights"]).all() and np.abs(ref["weights"]).max() > 0
    # the same four-way comparison for the episode record: train, the trait loop, the split at both depths, the shards joined
    train, trait, d1, d16, s0, s1 = Recording.log
    rows = np.arange(cap)[:, None] < ref["episode_steps"][None, :]
    assert np.array_equal(np.isnan(train["record_rewards"]), ~rows) and (case is CASE_A or len(set(ref["episode_steps"][:64])) > 1)      # (b: ragged inside one wave)
    assert_same_record(trait, train, "the trait loop's record against train's")
    assert_same_record(d1, train, "the split train's record at steps_per_launch 1")
    assert_same_record(d16, train, "the split train's record at steps_per_launch 16")
    assert_same_record({n: np.concatenate([s0[n], s1[n]], axis=-1) for n in s0}, train, "two shards' records joined")


@pytest.mark.parametrize("case,K", [(CASE_A, 50), (CASE_B, 120)], ids=["mountain-car", "cart-pole"])
def test_environment_side_is_tds(case, K):
    """both agents sample Random on the same draw (BLK_RESET is BLK_STEP's alias): same seed, N, cap and domain give the same episodes"""
    with ctx(**case) as c, ctx(algo=ra.TD, **case) as t:
        c.reset()
        t.reset()
        sc, stt = c.train(K), t.train(K)
        for name in ("states", "actions", "episode_steps"):
            assert np.array_equal(getattr(c, name).view(np.uint32), getattr(t, name).view(np.uint32)), name
        for name in ("env_steps", "episodes", "episodes_truncated", "sum_episode_steps"):
            assert sc[name] == stt[name], (name, sc[name], stt[name])
        assert sc["episodes"] > 0 and sc["sum_reward"] == stt["sum_reward"]


def _record(c):
    s, r = c.episode_record
    return dict(record_states=s, record_rewards=r)


def test_checkpoint_holds_the_weights_and_the_caller_carries_the_record(tmp_path):
    path = os.path.join(str(tmp_path), "gmc.ckpt")
    with ctx(**CASE_A) as a, ctx(**CASE_A) as b:
        a.reset()
        a.train(10)
        a.save_weights(path)
        b.load_weights(path)
        b.states, b.actions, b.episode_steps, b.episode_record = a.states, a.actions, a.episode_steps, a.episode_record
        assert (a.episode_steps == 3).all() and b.step_count == a.step_count == 10
        for when, k in (("after the load", 0), ("20 steps after the load", 20)):
            if k:
                a.train(k)
                b.train(k)
            assert_same(snapshot(b), snapshot(a), when)
            assert_same_record(_record(b), _record(a), "the record " + when)
            assert a.checksum() == b.checksum(), when
        assert np.abs(snapshot(a)["weights"]).max() > 0
    with open(path, "rb") as f:
        head = f.read(72)
    # weights only, under the header's algo 23: version 2, aux_kind 0, RSRL_TD's layout
    assert int.from_bytes(head[8:12], "little") == 2 and int.from_bytes(head[44:48], "little") == 23 and int.from_bytes(head[52:56], "little") == 0
    assert os.path.getsize(path) == 72 + N * 16 * 4
    check_foreign_checkpoints_refused(ctx, CASE_A, path, [dict(BASE, **dict(CASE_A, algo=ra.TD))], tmp_path)


def test_refusals_and_the_record_accessors(orc):
    rng = np.random.default_rng(3)
    cap = 7
    with ctx(**CASE_A) as c:
        assert c.n_out == 1
        S = rand_states(orc, ra.MOUNTAIN_CAR, N, rng)
        assert c.q_evaluate(S).shape == (1, N) and c.get_weights(0).shape == (c.F, 1)
        calls = [lambda: c.handle(S, np.zeros(N, np.int32), np.zeros(N, np.float32), S, np.zeros(N, np.uint8)),
                 lambda: c.q_find_max(S), lambda: c.q_find_min(S), lambda: c.q_expected_value(S, np.full((c.A, N), 1.0 / c.A, dtype=np.float32)),
                 lambda: c.get_traces(0), lambda: c.set_traces(np.zeros((c.F, 1)), 0), lambda: c.get_td_weights(0),
                 lambda: c.set_td_weights(np.zeros((c.F, c.A)), 0), lambda: c.get_policy_weights(0), lambda: c.set_policy_weights(np.zeros((c.F, c.A)), 0),
                 lambda: c.get_lstd_state(0), lambda: getattr(c, "return_carry"), lambda: setattr(c, "return_carry", np.zeros(N))]
        for k, call in enumerate(calls):
            with pytest.raises(RsrlHipError) as e:
                call()
            assert e.value.code == ESTATE, k
            if k == 0:
                assert "handle_batch" in str(e.value)
        # set_episode_steps above the cap: EINVAL, nothing changes
        c.reset()
        c.train(3)
        before = c.episode_steps
        steps = before.copy()
        steps[N - 1] = cap + 1
        with pytest.raises(RsrlHipError) as e:
            c.episode_steps = steps
        assert e.value.code == EINVAL and np.array_equal(c.episode_steps, before) and (before == 3).all()
        steps[N - 1] = cap                                                        # ... the cap itself is a full record
        c.episode_steps = steps
        assert c.episode_steps[N - 1] == cap
        # a set / get round trip: the rows below each learner's episode_steps come back, NaN past them
        Sr, Rr = rng.normal(size=(cap, c.D, N)).astype(np.float32), rng.normal(size=(cap, N)).astype(np.float32)
        ep = (np.arange(N) % (cap + 1)).astype(np.uint32)
        c.episode_steps = ep
        c.episode_record = (Sr, Rr)
        gs, gr = c.episode_record
        live = np.arange(cap)[:, None] < ep[None, :]
        assert np.array_equal(np.isnan(gr), ~live) and np.array_equal(gr[live], Rr[live])
        for d in range(c.D):
            assert np.array_equal(np.isnan(gs[:, d, :]), ~live) and np.array_equal(gs[:, d, :][live], Sr[:, d, :][live])
        c.reset()                                                                 # reset empties every record
        assert np.isnan(c.episode_record[1]).all() and not c.episode_steps.any()
        c.episode_steps = ep
        mask = (np.arange(N) % 2).astype(np.uint8)
        c.domain_reset(mask)                                                      # ... domain_reset the restarted learners'
        gr = c.episode_record[1]
        assert np.isnan(gr[:, mask == 1]).all() and np.array_equal(np.isnan(gr[:, mask == 0]), ~live[:, mask == 0])
    with ctx(algo=ra.TD, **CASE_A) as t:                                         # the record accessors are GradientMC's only
        for call in (lambda: getattr(t, "episode_record"), lambda: setattr(t, "episode_record", (np.zeros((cap, t.D, N)), np.zeros((cap, N))))):
            with pytest.raises(RsrlHipError) as e:
                call()
            assert e.value.code == ESTATE


def test_gradient_mc_example_builds_and_runs(tmp_path):
    out = run_example(tmp_path, "gradient_mc", [64, 2, 300, 3, 50])
    assert "Batch 2:" in out and "(16 features)" in out and "20-step trajectory handled" in out
    wmax = float(out.split("max |w| of learner 0:")[1].split()[0])
    moved = float(out.split("moved by")[1].split()[0])
    assert np.isfinite(wmax) and wmax > 0.0 and moved > 0.0
