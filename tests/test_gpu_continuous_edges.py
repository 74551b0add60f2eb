"""The Gaussian and the Beta policy code (cont_policy.hpp: softplus_dev, softplus_grad_dev, gauss_params .. gauss_coef,
beta_params .. beta_sample, digamma_dev) against the reference's f64 semantics on the crafted table of tests/continuous_edges.py: sd at its 0.01
floor, Softplus's switch at 10 from both sides, a = mu, |a - mu| = sd (where d^2 - Sigma cancels), the far tail and the underflow of the density,
sd^2 beyond fp32, Beta's clamp edges and parameters a few ulps above 1, NaN and the infinities as preferences.  The comparison is staged
(continuous_edges.py's docstring): stage A, the parameters RELATIVE TO THEMSELVES; stage B, everything downstream in f64 at the device's own fp32
parameters, in units of 2^-24 cond(row), against four times what a float32 numpy evaluation of the reference gives on the same rows.

The preferences are set through the weights (ce.columns: the constant feature alone), so they hold at EVERY state; each leg first checks that
policy_params on random states returns the same parameters at every state.  One learner per row.

  read-only legs     k_cont_policy under Gaussian (from NAC) and under Beta (from the iLSTD ActorCritic) at orders 1 (packed), 2 (unpacked), 5 (the largest
                     register footprint), the non-finite rows included: params, mode, pdf, two policy_sample(states) calls; twice the same bits;
                     the checksum and step_count unchanged
  coefficient legs   NAC (Gaussian, Beta): q_evaluate_f32 with the critic's w a unit vector at the state whose features are all exactly 1 is c_m /
                     c_s (c_a / c_b) itself, and one handle from w = 0 with lr r = 1 leaves (c_0, c_1, 1) in w's three blocks.  CACLA (33), the TD
                     ActorCritic (35, Gaussian and Beta) and the Beta iLSTD ActorCritic (21): handle there with lr = 0, w = 0, a terminal
                     transition and e a power of two (35, 21: alpha = 0.5, r = 2, e = 1; 33: alpha = 1, e = fl32(a - mu)) moves every zero row of
                     a column to fl32(e c): those rows are held at stage B, the constant row to sign and size, w and td to the critic's bits, the
                     learners past a partial batch to their bytes; CACLA's closed gate (r < 0) to the columns' bits
  driver-loop legs   alpha = 0, lr = 0, reset, train(1), train(2) per agent on the rows with finite coefficients: columns and w bit-identical, the
                     actions after reset / step 0 / step 2 at the stage-B sample bar on the loop's own draws (BLK_INIT at t, BLK_STEP at t, t + 2)
  Philox extremes    gauss_normal at the words tests/golden/philox_extremes.json lists (u1 = 2^-24 and just above, u1 = 1, u2 = 0, u2 beside 1/4 and
                     3/4): one n_envs = 1 ctx per hit

Every test prints its figures before it asserts.  Measured on an MI355X: profiles/continuous_edges.md."""
import functools
import json
import os

import numpy as np
import pytest

import rsrl_amd as ra
from tests import beta_numpy as bn
from tests import continuous_edges as ce
from tests import gaussian_numpy as gn
from tests.lstd_numpy import ilstd, ilstd_init
from tests.tdac_lstd_numpy import critic_target

pytestmark = pytest.mark.gpu

G, B = ce.GAUSSIAN, ce.BETA
CMC = ra.CONTINUOUS_MOUNTAIN_CAR
SEED, OFFSET = ce.SEED, ce.OFFSET
PID = {G: "gaussian", B: "beta"}
NAC_G = dict(algo=ra.NAC, policy=G, n_steps=100)
NAC_B = dict(algo=ra.NAC, policy=B, n_steps=100)
ILSTD_B = dict(algo=ra.ILSTD_ACTOR_CRITIC, policy=B, n_steps=2)
CACLA_G = dict(algo=33, policy=G)
TDAC_G = dict(algo=35, policy=G)
TDAC_B = dict(algo=35, policy=B)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "philox_extremes.json")


def ctx(agent, order, n, **kw):
    return ra.Context(**dict(dict(domain=CMC, order=order, n_envs=n, seed=SEED, env_offset=OFFSET, gamma=0.95, max_episode_steps=100000), **agent, **kw))


def craft(c, p0, p1):
    for i in range(len(p0)):
        c.set_policy_weights(ce.columns(c.F, p0[i], p1[i]), i)


def rand_states(c, M, seed):
    lo, hi = c.state_bounds()
    rng = np.random.default_rng(seed)
    return (lo[:, None] + (hi - lo)[:, None] * rng.random((c.D, M))).astype(np.float32)


def ones_state(c, M):
    """the lower corner of the bounds: every Fourier feature is cos(0) = 1 exactly"""
    lo, _ = c.state_bounds()
    S = np.repeat(np.asarray(lo, dtype=np.float32)[:, None], M, axis=1)
    assert np.array_equal(c.project(S), np.ones((c.F, M), dtype=np.float32))
    return S


def same_bits(x, y):
    return np.asarray(x).tobytes() == np.asarray(y).tobytes()


def rows(policy, with_nonfinite=False):
    p0, p1, a, g = ce.table(policy)
    if with_nonfinite:
        q0, q1, qa = ce.nonfinite(policy)
        p0, p1, a, g = np.concatenate([p0, q0]), np.concatenate([p1, q1]), np.concatenate([a, qa]), np.concatenate([g, np.full(len(q0), "nonfinite")])
    return p0, p1, a, g


def params_everywhere(c, p0, p1, policy):
    """the precondition: policy_params returns the crafted preferences' parameters at EVERY state -> (x0, x1) float32 (mu, sd | alpha, beta)"""
    M = len(p0)
    x0, x1 = c.policy_params(rand_states(c, M, 5))
    for S in (rand_states(c, M, 6), ones_state(c, M)):
        y0, y1 = c.policy_params(S)
        assert same_bits(x0, y0) and same_bits(x1, y1), "the parameters depend on the state"
    if policy == G:                                     # mu IS the crafted preference (-0.0 comes back as the sum 0 + -0 = +0: equal, not the same bits)
        zero = p0 == 0
        assert same_bits(x0[~zero], p0[~zero]) and np.all(x0[zero] == 0), "mu is not the crafted preference"
    return x0, x1


def hold(name, figure, bound):
    print("\nEDGE %s: %.4g (bar %.4g)" % (name, figure, bound))
    assert figure <= bound, (name, figure, bound)


def worst(u, skip=None):
    u = np.asarray(u, dtype=np.float64)
    return float(np.max(u[~skip] if skip is not None else u)) if u.size else 0.0


def stage_a(policy, p0, p1, x0, x1, tag):
    if policy == G:
        hold("%s sd rel. to sd" % tag, worst(ce.rel_self(x1, ce.sd64(p1))), ce.sd_bar())
    else:
        al, be = bn.beta_params(p0.astype(np.float64), p1.astype(np.float64))
        with np.errstate(invalid="ignore"):
            hold("%s alpha rel. to alpha" % tag, worst(ce.rel_self(x0, al)), ce.PARAM_BAR)
            hold("%s beta rel. to beta" % tag, worst(ce.rel_self(x1, be)), ce.PARAM_BAR)


def hold_b(policy, quantity, u, tag, n_table):
    """a stage-B figure over the table's rows but the declared ones (u may carry the non-finite rows behind the table's)"""
    skip = np.zeros(len(u), dtype=bool)
    skip[:n_table] = ce.declared_mask(policy, quantity)
    hold("%s %s %s [2^-24 cond]" % (tag, PID[policy], quantity), worst(u, skip), ce.bar(policy, quantity))


def beta_samples(x, alpha, beta, gid, t, purpose, tag):
    want, margin = bn.beta_sample(SEED, gid, t, purpose, alpha.astype(np.float64), beta.astype(np.float64))
    out = margin < ce.BETA_MARGIN
    print("\nEDGE %s beta sample: %d of %d left out" % (tag, int(out.sum()), len(out)))
    assert out.mean() <= ce.BETA_LEFT_OUT, (tag, out.mean())
    hold("%s beta sample |x - x64|" % tag, worst(np.abs(x.astype(np.float64) - want), out), ce.BETA_SAMPLE_BAR)


def gauss_samples(x, mu, sd, gid, t, purpose, tag):
    z, rad = ce.normal_parts(SEED, gid, t, purpose)
    hold("%s gaussian sample [2^-24 cond]" % tag, worst(ce.units(x, *ce.gauss_sample_b(mu, sd, z, rad))), ce.bar(G, "sample"))


# ------------------------------------------------------------------------------------------------------------------------- read-only legs
@pytest.mark.parametrize("order", [1, 2, 5])
@pytest.mark.parametrize("policy", [G, B], ids=["gaussian", "beta"])
def test_read_only_calls(policy, order):
    p0, p1, a, g = rows(policy, with_nonfinite=True)
    n_table, M = len(ce.table(policy)[0]), len(p0)
    tag = "read-only order %d" % order
    with ctx(NAC_G if policy == G else ILSTD_B, order, M) as c:
        craft(c, p0, p1)
        before = (c.checksum(), c.step_count)
        x0, x1 = params_everywhere(c, p0, p1, policy)
        stage_a(policy, p0, p1, x0, x1, tag)
        S = rand_states(c, M, 7)
        mode, pdf = c.policy_mode(S), c.policy_pdf(S, a)
        assert same_bits(mode, c.policy_mode(S)) and same_bits(pdf, c.policy_pdf(S, a)), "two calls, two answers"
        y0, y1 = c.policy_params(S)
        assert same_bits(x0, y0) and same_bits(x1, y1)
        smp = [c.policy_sample(S) for _ in range(2)]
        assert (c.checksum(), c.step_count) == before, "a read-only call changed the ctx"
    gid = OFFSET + np.arange(M)
    if policy == G:
        assert same_bits(mode, x0), "the mode is the mean"
        u = ce.stage_b(G, p0, p1, a, dict(mu=x0, sd=x1, pdf=pdf))
        hold_b(G, "pdf", u["pdf"], tag, n_table)
        for t in range(2):
            gauss_samples(smp[t], x0, x1, gid, t, bn.BLK_API, "%s call %d" % (tag, t))
    else:
        u = ce.stage_b(B, p0, p1, a, dict(alpha=x0, beta=x1, pdf=pdf, mode=mode))
        hold_b(B, "pdf", u["pdf"], tag, n_table)
        hold_b(B, "mode", u["mode"], tag, n_table)
        for t in range(2):                                                                   # (the finite rows: the sampler's loop is not defined on NaN)
            assert np.all((smp[t][:n_table] >= ce.LO32) & (smp[t][:n_table] <= ce.HI32))
            beta_samples(smp[t][:n_table], x0[:n_table], x1[:n_table], gid[:n_table], t, bn.BLK_API, "%s call %d" % (tag, t))


# ------------------------------------------------------------------------------------------------------------------------- coefficient legs
NAMES = {G: ("cm", "cs"), B: ("ca", "cb")}


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("policy", [G, B], ids=["gaussian", "beta"])
def test_nac_q_is_the_coefficient(policy, order):
    """Q = fma(c_0, <w_0, phi>, fma(c_1, <w_1, phi>, <w_2, phi>)) with w a unit vector in block b at phi = 1 is c_b -- or NaN where the other
    coefficient, which meets a zero, is not finite"""
    p0, p1, a, g = rows(policy)
    N = len(p0)
    tag = "nac-q order %d" % order
    with ctx(NAC_G if policy == G else NAC_B, order, N) as c:
        craft(c, p0, p1)
        x0, x1 = params_everywhere(c, p0, p1, policy)
        S = ones_state(c, N)
        got = {}
        for b, name in enumerate(NAMES[policy]):
            w = np.zeros((3 * c.F, 1), dtype=np.float32)
            w[b * c.F + (c.F - 1 if b else 0)] = 1.0
            for i in range(N):
                c.set_weights(w, i)
            got[name] = c.q_evaluate_f32(S, a)
    ref = ce.gauss_b(x0, x1, p1, a) if policy == G else ce.beta_b(x0, x1, p0, p1, a)
    for name, other in (NAMES[policy], NAMES[policy][::-1]):
        with np.errstate(invalid="ignore"):
            nan = np.abs(ref[other][0]) > ce.FLT_MAX                                         # 0 * inf
        assert np.all(np.isnan(got[name][nan])), (tag, name, "0 * an infinite coefficient")
        print("\nEDGE %s %s %s: %d of %d rows are NaN by rule (the other coefficient is infinite), held by the handle legs of 33 / 35 / 21" % (tag, PID[policy], name, int(nan.sum()), N))
        u = ce.units(got[name], *ref[name])
        hold("%s %s %s [2^-24 cond]" % (tag, PID[policy], name), worst(u, nan | ce.declared_mask(policy, name)), ce.bar(policy, name))


HANDLE = [("cacla", CACLA_G, G), ("tdac-gaussian", TDAC_G, G), ("tdac-beta", TDAC_B, B), ("ilstd-ac-beta", ILSTD_B, B)]


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name,agent,policy", HANDLE, ids=[h[0] for h in HANDLE])
def test_handle_moves_the_zero_rows_to_the_coefficient(name, agent, policy, order):
    p0, p1, a, g = rows(policy)
    N = len(p0)
    M = N - 37                                                                               # a partial batch: the last learners are not touched
    tag = "handle %s order %d" % (name, order)
    cacla, ilstd_ac = name == "cacla", name == "ilstd-ac-beta"
    alpha, r = (1.0, 2.0) if cacla else (0.5, 2.0)
    with ctx(agent, order, N, lr=0.0, alpha=alpha) as c:
        craft(c, p0, p1)
        x0, x1 = params_everywhere(c, p0, p1, policy)
        F = c.F
        S = ones_state(c, M)
        rew, term = np.full(M, r, dtype=np.float32), np.ones(M, dtype=np.uint8)
        if cacla:                                                                            # r < 0 = V: the gate is closed, whatever the coefficients
            td = c.handle(S, a[:M], -rew, S, term)
            assert same_bits(td, -rew)
            for i in range(N):
                assert same_bits(c.get_policy_weights(i), ce.columns(F, p0[i], p1[i])), (tag, "a closed gate moved the columns", i)
        td = c.handle(S, a[:M], rew, S, term)
        cols = np.stack([c.get_policy_weights(i) for i in range(N)])
        w = np.stack([c.get_weights(i) for i in range(N)])
    # the critic: w = 0 and lr = 0 (iLSTD: its step size), so V stays 0 and the error is r
    assert same_bits(td, rew) and not w.any() and not np.signbit(w).any(), (tag, "w and td are the critic's: w = 0, td = r")
    for i in range(M, N):
        assert same_bits(cols[i], ce.columns(F, p0[i], p1[i])), (tag, "a learner past the batch moved", i)
    for k in range(1, F - 1):
        assert same_bits(cols[:M, k], cols[:M, 0]), (tag, "the zero rows differ among themselves", k)
    ref = ce.gauss_b(x0, x1, p1, a) if policy == G else ce.beta_b(x0, x1, p0, p1, a)
    # e.  35: alpha (r - V(s')) = 1 exactly.  21: f32(alpha c) of the f64 iLSTD restatement (beta_numpy.tdac_beta_rule's two lines), 1 as well.
    # CACLA: fl32(a - mu) * 1, taken in f64 here: one relative rounding of e and one of the product e * c beside c's own, so
    # cond' = |e| (cond + 2 |c|) and floor' = 2^-149 + |e| floor
    if cacla:
        e = a.astype(np.float64) - x0.astype(np.float64)
    elif ilstd_ac:
        one = np.ones(F)
        _, theta2, _, _ = ilstd(*ilstd_init(F), one, one, r, True, 0.95, 0.0, ILSTD_B["n_steps"], literal=False)
        e = np.full(N, float(np.float32(alpha * critic_target(theta2, one, one, r, True, 0.95))))
        assert e[0] == 1.0
    else:
        e = np.ones(N)
    for b, q in enumerate(NAMES[policy]):
        want, cond, floor = ref[q]
        with np.errstate(invalid="ignore", over="ignore"):
            want_e, cond_e = e * want, np.abs(e) * (cond + (2.0 * np.abs(want) if cacla else 0.0))
            floor_e = ce.SUB + np.abs(e) * floor                                             # (c is an fp32 value before it meets e)
        u = ce.units(cols[:M, 0, b], want_e[:M], cond_e[:M], floor_e[:M])
        hold("%s %s [2^-24 cond]" % (tag, q), worst(u, ce.declared_mask(policy, q)[:M]), ce.bar(policy, q))
        # the constant row: p + e c, rounded once -- the right sign, and within one ulp of the preference's size
        p, move = (p0, p1)[b][:M].astype(np.float64), cols[:M, 0, b].astype(np.float64)
        got = cols[:M, F - 1, b].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            ok = np.isfinite(move) & np.isfinite(p + move)
            ulp = np.spacing(np.maximum(np.abs(p), np.abs(got)).astype(np.float32)).astype(np.float64)
            err, along = np.abs(got - (p + move)), (got - p) * move
        assert np.all(err[ok] <= ulp[ok]), (tag, q, "the constant row")
        assert np.all(along[ok] >= 0), (tag, q, "the constant row moved against the coefficient")


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("policy", [G, B], ids=["gaussian", "beta"])
def test_nac_handle_moves_w_by_the_coefficients(policy, order):
    """SARSA::handle of NAC's critic (the step function of k_handle_nac_*, its own copy of the policy code): from w = 0 on a terminal transition at the
    all-ones state, delta = r - Q = r and w' = fl32(lr r) psi = (c_0, c_1, 1) for lr = 0.5, r = 2 -- row by row, one rounding behind each coefficient.
    The policy's columns do not move, and the learners past the batch keep their bytes"""
    p0, p1, a, g = rows(policy)
    N = len(p0)
    M = N - 37
    tag = "nac-handle order %d" % order
    with ctx(NAC_G if policy == G else NAC_B, order, N, lr=0.5, alpha=0.1) as c:
        craft(c, p0, p1)
        x0, x1 = params_everywhere(c, p0, p1, policy)
        F = c.F
        S = ones_state(c, M)
        rew = np.full(M, 2.0, dtype=np.float32)
        td = c.handle(S, a[:M], rew, S, np.ones(M, dtype=np.uint8))
        w = np.stack([c.get_weights(i)[:, 0] for i in range(N)])
        for i in range(N):
            assert same_bits(c.get_policy_weights(i), ce.columns(F, p0[i], p1[i])), (tag, "the critic moved the policy", i)
    assert not w[M:].any() and not np.signbit(w[M:]).any(), (tag, "a learner past the batch moved")
    ref = ce.gauss_b(x0, x1, p1, a) if policy == G else ce.beta_b(x0, x1, p0, p1, a)
    with np.errstate(invalid="ignore"):
        nan = (np.abs(ref[NAMES[policy][0]][0]) > ce.FLT_MAX) | (np.abs(ref[NAMES[policy][1]][0]) > ce.FLT_MAX)       # Q = 0 * inf: delta is NaN, and so is w'
    nan = nan[:M]
    print("\nEDGE %s %s: %d of %d rows are NaN by rule (a coefficient is infinite: Q = 0 * inf), held by the handle legs of 33 / 35 / 21" % (tag, PID[policy], int(nan.sum()), M))
    assert np.all(np.isnan(td[nan])) and same_bits(td[~nan], rew[~nan]), (tag, "delta = r - Q with Q = <0, psi>")
    assert np.all(w[:M, 2 * F:][~nan] == 1.0)
    for b, q in enumerate(NAMES[policy]):
        blk = w[:M, b * F:(b + 1) * F]
        for k in range(1, F):
            assert same_bits(blk[:, k], blk[:, 0]), (tag, "the rows of a block differ among themselves", k)
        u = ce.units(blk[:, 0], *(x[:M] if np.ndim(x) else x for x in ref[q]))
        hold("%s %s %s [2^-24 cond]" % (tag, PID[policy], q), worst(u, nan | ce.declared_mask(policy, q)[:M]), ce.bar(policy, q))


# ------------------------------------------------------------------------------------------------------------------------- driver-loop legs
DRIVE = [("nac-gaussian", NAC_G, G), ("nac-beta", NAC_B, B), ("ilstd-ac-beta", ILSTD_B, B), ("cacla", CACLA_G, G), ("tdac-gaussian", TDAC_G, G), ("tdac-beta", TDAC_B, B)]


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name,agent,policy", DRIVE, ids=[d[0] for d in DRIVE])
def test_driver_loop_samples(name, agent, policy, order):
    keep = ce.finite_coefficients(policy)
    p0, p1 = (x[keep] for x in ce.table(policy)[:2])
    N = len(p0)
    assert N >= 20
    tag = "driver-loop %s order %d" % (name, order)
    gid = OFFSET + np.arange(N)
    with ctx(agent, order, N, lr=0.0, alpha=0.0) as c:
        craft(c, p0, p1)
        x0, x1 = params_everywhere(c, p0, p1, policy)
        cols = [c.get_policy_weights(i) for i in range(N)]
        w = [c.get_weights(i) for i in range(N)]
        t0 = c.step_count
        check = functools.partial(gauss_samples if policy == G else beta_samples, **{("mu" if policy == G else "alpha"): x0, ("sd" if policy == G else "beta"): x1})
        c.reset()
        check(c.actions.copy(), gid=gid, t=t0, purpose=bn.BLK_INIT, tag=tag + " reset")
        c.train(1)
        check(c.actions.copy(), gid=gid, t=t0, purpose=bn.BLK_STEP, tag=tag + " step 0")
        c.train(2)
        check(c.actions.copy(), gid=gid, t=t0 + 2, purpose=bn.BLK_STEP, tag=tag + " step 2")
        assert c.step_count == t0 + 3 and np.all(c.episode_steps == 3), (tag, "an episode ended")
        for i in range(N):
            assert same_bits(c.get_policy_weights(i), cols[i]) and same_bits(c.get_weights(i), w[i]), (tag, "something was learned with alpha = lr = 0", i)


# ------------------------------------------------------------------------------------------------------------------------- the Philox extremes
def test_gauss_normal_at_the_philox_extremes():
    """one n_envs = 1 ctx per listed (seed, id), env_offset = id: its FIRST policy_sample(states) draws the listed words (BLK_API at t = 0).  The crafted
    rows cycle over the first and the last row of the `floor` and the `general` group"""
    with open(GOLDEN) as f:
        hits = json.load(f)["hits"]
    p0, p1, _, g = ce.table(G)
    picks = [int(np.flatnonzero(g == grp)[k]) for grp in ("floor", "general") for k in (0, -1)]
    worst_u, worst_z = 0.0, 0.0
    for n, h in enumerate(hits):
        j = picks[n % len(picks)]
        gid = np.array([h["id"]])
        with ctx(NAC_G, 1, 1, seed=h["seed"], env_offset=h["id"]) as c:
            c.set_policy_weights(ce.columns(c.F, p0[j], p1[j]), 0)
            S = rand_states(c, 1, 3)
            mu, sd = c.policy_params(S)
            assert c.step_count == 0
            x = c.policy_sample(S)
        w = bn.philox_block(h["seed"], gid, 0, bn.BLK_API + 256)
        assert [int(v) for v in w[0]] == h["words"], (h, "the fixture's words")
        z, rad = gn.gauss_normal_parts(h["seed"], gid, 0, bn.BLK_API)
        u = float(ce.units(x, *ce.gauss_sample_b(mu, sd, z, rad))[0])
        dz = abs(float(x[0]) - float(mu[0])) / float(sd[0])
        print("EDGE philox %s seed %d id %d row %d: %.4g units, |a - mu| / sd = %.6g" % (h["class"], h["seed"], h["id"], j, u, dz))
        worst_u, worst_z = max(worst_u, u), max(worst_z, dz)
    hold("philox extremes gaussian sample [2^-24 cond]", worst_u, ce.bar(G, "sample"))
    hold("philox extremes |a - mu| / sd", worst_z, gn.Z_MAX * (1.0 + 2.0 ** -20))
