"""What every agent's test module asserts the same way, once (a plain helper module like tests/edge_helpers.py: no fixtures, no pytest settings).

The contract of an agent with a driver loop: train(K) leaves the bits of the host trait loop (domain_step -> handle -> domain_reset(ended) ->
policy_sample), of the same K steps split over several calls at any launch depth, and of two env_offset shards joined; a checkpoint resumes to
the same bits and no other agent's file loads.  "The same bits" is `diff` over `snapshot`: one definition of both.  A snapshot is an ordered
mapping name -> array; the names of PER_CTX are the ctx's own arrays ([D][N] / [N], the learner on the LAST axis), every other entry is one
array per learner stacked on axis 0.  Which axis a shard joins on follows from the name, never from the entry's position."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rsrl_amd as ra
from rsrl_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_CTX = ("states", "hidden", "actions", "episode_steps", "return_carry")
EINVAL = -1


def rand_states(orc, domain, n, rng):
    lo, hi = orc.domain_bounds(domain)
    return rng.uniform(lo, hi, size=(n, len(lo))).T.astype(np.float32)


def learner_state(c, i):
    """everything learner i learns, name -> array: the f64 least-squares state, the value weights (REINFORCE has none; BaselineREINFORCE's are its
    baseline; the iLSTD agents' are f32(lstd_theta) and left out; LSTD's and LSTDLambda's f32(lstd_theta) stay next to theta / A / b / z and the
    singular counter; NAC's are the critic's 3F rows), the actor's theta (the Gibbs actor's A columns, the Beta policy's two), REINFORCE's
    behaviour snapshot"""
    al, out = c.cfg.algo, {}
    if al in (ra.RECURSIVE_LSTD, ra.ILSTD, ra.ILSTD_ACTOR_CRITIC):
        out["lstd_theta"], out["lstd_matrix"], mu = c.get_lstd_state(i)
        if mu is not None:
            out["lstd_mu"] = mu
    elif al != ra.REINFORCE:
        out["weights"] = c.get_weights(i)
    if al in (ra.LSTD, ra.LSTD_LAMBDA):
        out["lstd_theta"], out["lstd_A"], out["lstd_b"], z, sing = c.get_lstd_batch_state(i)
        if z is not None:
            out["lstd_z"] = z
        out["singular_solves"] = np.array(sing, dtype=np.uint32)
    if al in (ra.ACTOR_CRITIC, ra.Q_ACTOR_CRITIC, ra.TD_ACTOR_CRITIC, ra.REINFORCE, ra.BASELINE_REINFORCE, ra.ILSTD_ACTOR_CRITIC, ra.NAC):
        out["theta"] = c.get_policy_weights(i)
    if al in (ra.REINFORCE, ra.BASELINE_REINFORCE):
        out["theta_b"] = c.get_behaviour_weights(i)
    return out


def snapshot(c, learners=None):
    """the learners' state (all of them, or those listed) stacked on axis 0, then the ctx's own arrays"""
    per = [learner_state(c, i) for i in (range(c.N) if learners is None else learners)]
    out = {name: np.stack([p[name] for p in per]) for name in per[0]}
    out["states"] = c.states
    if c.cfg.domain == ra.HIV_TREATMENT:
        out["hidden"] = c.get_hidden_states()
    out["actions"], out["episode_steps"] = c.actions, c.episode_steps
    if c.cfg.algo in (ra.REINFORCE, ra.BASELINE_REINFORCE):
        out["return_carry"] = c.return_carry
    return out


def _same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and x.tobytes() == y.tobytes() and bool(np.array_equal(x, y))


def diff(a, b):
    """the names that differ, [] when none does.  The same: in both mappings, the same shape, the same bytes AND np.array_equal -- so -0.0
    against 0.0 differs, and so does any NaN"""
    return [n for n in list(a) + [n for n in b if n not in a] if n not in a or n not in b or not _same(a[n], b[n])]


def assert_same(a, b, what):
    """(this module's asserts are not rewritten by pytest: the message names what differs)"""
    names = diff(a, b)
    assert not names, "%s: %s differ" % (what, ", ".join(names))


def join_shards(a, b):
    return {n: np.concatenate([a[n], b[n]], axis=-1 if n in PER_CTX else 0) for n in a}


def trait_loop(c, K, cap):
    """K iterations of domain_step -> handle -> domain_reset(terminal or at the cap) -> policy_sample(NULL); Domain::transition does not count
    steps, so the loop's driver does.  cap 0: no cap, as max_episode_steps = 0.  (HIVTreatment never reports a terminal: the same loop.)"""
    ep = c.episode_steps.astype(np.int64)
    for _ in range(K):
        frm, nxt, rew, term = c.domain_step(c.actions)
        c.handle(frm, c.actions, rew, nxt, term)
        ep += 1
        mask = (term.astype(bool) | ((ep >= cap) if cap > 0 else False)).astype(np.uint8)
        c.domain_reset(mask)
        ep[mask == 1] = 0
        c.policy_sample()
    c.episode_steps = ep.astype(np.uint32)


def record_bits(c):
    """the episode record of GradientMC / LSTD / LSTDLambda as bit patterns with the learner on axis 0, where every per-learner entry joins:
    name -> uint32 array (N, cap, D) / (N, cap).  The accessor shows NaN past each learner's rows, which `diff` refuses raw"""
    s, r = c.episode_record
    return dict(record_states=np.moveaxis(np.ascontiguousarray(s).view(np.uint32), -1, 0), record_rewards=np.moveaxis(np.ascontiguousarray(r).view(np.uint32), -1, 0))


def gmc_trait_loop(c, K, cap):
    """GradientMC: domain_step -> append (from, r) on the host -> handle_batch(the length of the episodes that just ended, else 0) ->
    domain_reset(ended) -> policy_sample(); at the end the open rows become the ctx's record"""
    D = c.D
    S, R = np.zeros((cap, D, c.N), np.float32), np.zeros((cap, c.N), np.float32)
    ep = c.episode_steps.astype(np.int64)
    cols = np.arange(c.N)
    for _ in range(K):
        frm, _, rew, term = c.domain_step(c.actions)
        S[ep, :, cols] = frm.T
        R[ep, cols] = rew
        ep += 1
        ended = term.astype(bool) | (ep >= cap)
        c.handle_batch(S, None, R, np.where(ended, ep, 0).astype(np.uint32))
        c.domain_reset(ended.astype(np.uint8))
        ep[ended] = 0
        c.policy_sample()
    c.episode_steps = ep.astype(np.uint32)
    c.episode_record = (S, R)


def lstd_batch_trait_loop(c, K, cap):
    """LSTD / LSTDLambda: domain_step -> append the transition on the host -> handle_transitions(the length of the episodes that just ended,
    else 0) -> domain_reset(ended) -> policy_sample(); at the end the open rows become the ctx's record"""
    D = c.D
    S, S2 = np.zeros((cap, D, c.N), np.float32), np.zeros((cap, D, c.N), np.float32)
    R, Tm = np.zeros((cap, c.N), np.float32), np.zeros((cap, c.N), np.uint8)
    ep = c.episode_steps.astype(np.int64)
    cols = np.arange(c.N)
    for _ in range(K):
        frm, nxt, rew, term = c.domain_step(c.actions)
        S[ep, :, cols] = frm.T
        S2[ep, :, cols] = nxt.T
        R[ep, cols] = rew
        Tm[ep, cols] = term
        ep += 1
        ended = term.astype(bool) | (ep >= cap)
        c.handle_transitions(S, R, S2, Tm, np.where(ended, ep, 0).astype(np.uint32))
        c.domain_reset(ended.astype(np.uint8))
        ep[ended] = 0
        c.policy_sample()
    c.episode_steps = ep.astype(np.uint32)
    c.episode_record = (S, R)


def check_train_invariance(make_ctx, kw, K, cap, depths, first_split, kernel=None, setup=None, trait=trait_loop):
    """one train(K) against: the host trait loop; train(first_split) + train(1) + train(the rest) at every steps_per_launch of `depths`; two
    env_offset shards of N / 2 joined.  setup(c, env_offset) prepares a fresh ctx (default: c.reset()); trait(c, K, cap) may return the
    snapshot to compare where the ctx's own is not it; `kernel` is the name timing_read must report for the train.
    -> (the train's statistics, its snapshot) for what the caller asserts besides"""
    N = kw["n_envs"]
    setup = setup or (lambda c, off: c.reset())
    with make_ctx(**kw) as c:
        setup(c, 0)
        if kernel is not None:
            c.timing_enable(True)
        st = c.train(K)
        if kernel is not None:
            assert c.timing_read()[2] == kernel, c.timing_read()[2]
        ref = snapshot(c)
    with make_ctx(**kw) as c:
        setup(c, 0)
        host = trait(c, K, cap)
        assert_same(snapshot(c) if host is None else host, ref, "the host trait loop against train(%d)" % K)
    for spl in depths:
        with make_ctx(steps_per_launch=spl, **kw) as c:
            setup(c, 0)
            c.train(first_split)
            c.train(1)
            c.train(K - first_split - 1)
            assert_same(snapshot(c), ref, "train(%d) + train(1) + train(%d) at steps_per_launch %d against train(%d)" % (first_split, K - first_split - 1, spl, K))
    shards = []
    for off in (0, N // 2):
        with make_ctx(env_offset=off, **dict(kw, n_envs=N // 2)) as c:
            setup(c, off)
            c.train(K)
            shards.append(snapshot(c))
    assert_same(join_shards(*shards), ref, "two env_offset shards joined against the unsharded train(%d)" % K)
    return st, ref


def _carry_over(a, b, carry):
    """what a checkpoint does not hold, from a to b (the hidden state after the observations: set_states re-derives it from them)"""
    assert set(carry) <= {"states", "hidden", "actions", "episode_steps", "return_carry", "theta_b"}, carry
    if "states" in carry:
        b.states = a.states
    if "hidden" in carry:
        b.set_hidden_states(a.get_hidden_states())
    if "actions" in carry:
        b.actions = a.actions
    if "episode_steps" in carry:
        b.episode_steps = a.episode_steps
    if "return_carry" in carry:
        b.return_carry = a.return_carry
    if "theta_b" in carry:
        for i in range(a.N):
            b.set_behaviour_weights(a.get_behaviour_weights(i), i)


def check_checkpoint_resume(make_ctx, kw, path, k1, k2, carry, at_save=None, then=None):
    """save after train(k1), load into a fresh ctx, carry over what the file does not hold: the same snapshot and checksum there and after
    train(k2) on both.  at_save(a) runs on the saved ctx before it moves on, then(a, b) at the end while both are open"""
    with make_ctx(**kw) as a, make_ctx(**kw) as b:
        a.reset()
        a.train(k1)
        a.save_weights(path)
        if at_save is not None:
            at_save(a)
        b.load_weights(path)
        _carry_over(a, b, carry)
        assert b.step_count == a.step_count, (b.step_count, a.step_count)
        assert_same(snapshot(b), snapshot(a), "the loaded ctx against the saved one")
        assert a.checksum() == b.checksum(), "checksums after the load"
        a.train(k2)
        b.train(k2)
        assert_same(snapshot(b), snapshot(a), "%d steps after the load" % k2)
        assert a.checksum() == b.checksum(), "checksums %d steps after the load" % k2
        if then is not None:
            then(a, b)


def check_foreign_checkpoints_refused(make_ctx, kw, path, others, tmp_path):
    """the file at `path` (make_ctx(**kw)'s) is EINVAL to every ctx of `others` (Context keyword sets) and theirs to make_ctx(**kw); a refused
    load leaves the ctx as it was"""
    opath = os.path.join(str(tmp_path), "other.ckpt")
    for other in others:
        with ra.Context(**other) as o, make_ctx(**kw) as b:
            o.save_weights(opath)
            for c, p in ((o, path), (b, opath)):
                before = c.checksum()
                with pytest.raises(ra.RsrlHipError) as e:
                    c.load_weights(p)
                assert e.value.code == EINVAL and c.checksum() == before, (other, p, e.value.code)


def _gxx(tmp_path, flags, out):
    out = os.path.join(str(tmp_path), out)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall"] + flags + ["-o", out], check=True, timeout=300)
    return out


def compile_example(tmp_path, name):
    """examples/<name>.cpp compiles without a warning (no library, no GPU)"""
    obj = _gxx(tmp_path, ["-Werror", "-c", os.path.join(ROOT, "examples", name + ".cpp")], name + ".o")
    assert os.path.getsize(obj) > 0


def run_example(tmp_path, name, args):
    """examples/<name>.cpp built against the library (once per tmp_path) and run with args -> stdout"""
    exe, lib = os.path.join(str(tmp_path), name), os.path.join(ROOT, "rsrl_amd", "lib")
    if not os.path.exists(exe):
        _gxx(tmp_path, [os.path.join(ROOT, "examples", name + ".cpp"), "-L" + lib, "-lrsrl_hip", "-Wl,-rpath," + lib], name)
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, check=True).stdout


def create_rc(base, **kw):
    """rsrl_hip_create on the config `base` with kw on top -> (return code, last error); a ctx that was created is destroyed"""
    L = _abi.lib()
    cfg = _abi.Config()
    assert L.rsrl_hip_config_init(C.byref(cfg)) == 0
    for k, v in dict(base, **kw).items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    rc = L.rsrl_hip_create(C.byref(cfg), C.byref(h))
    msg = (L.rsrl_hip_last_error() or b"").decode()
    if rc == 0:
        L.rsrl_hip_destroy(h)
    return rc, msg
