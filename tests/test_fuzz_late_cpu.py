"""The campaigns tests/fuzz_episodic.py and tests/fuzz_beta.py without a GPU: their samplers draw only what rsrl_hip_create admits, the shares
their GPU slices may leave out (tests/test_gpu_fuzz.py's committed seed and case count) hold in the f64 restatements alone, and the references
they hold the device to agree with their f64 forms."""
import numpy as np
import pytest

from tests import beta_numpy as bn
from tests import fuzz_beta as fb
from tests import fuzz_episodic as fe
from tests import nac_numpy as nn
from tests.agent_contract import create_rc
from tests.gmc_numpy import gradient_mc, td_chain
from tests.lstd_batch_numpy import residual
from tests.lstd_numpy import ilstd, near_tie_band

EINVAL, EHIP = -1, -2
EPS32, EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)
SEED, CASES = fe.SUITE_SEED, fe.SUITE_CASES


@pytest.mark.parametrize("mod", [fe, fb], ids=["episodic", "beta"])
def test_the_samplers_draw_only_admitted_configurations(mod):
    """2 000 draws of each sampler: rsrl_hip_create admits every one (EHIP -- no device -- here, a ctx with a GPU), and every value of every
    axis the issue lists is drawn"""
    rng = np.random.default_rng(0)
    seen = {}
    for idx in range(2000):
        kw = mod.sample(rng, idx)
        rc, msg = create_rc({}, **dict(kw, n_envs=min(kw["n_envs"], 4), env_offset=min(kw["env_offset"], (1 << 32) - 1 - 4)))
        assert rc == 0 or (rc == EHIP and "device" in msg), (kw, rc, msg)
        assert rc != EINVAL
        for k, v in kw.items():
            if k not in ("seed", "lr", "alpha"):
                seen.setdefault(k, set()).add(v)
        seen.setdefault("ids", set()).add(kw["env_offset"] + kw["n_envs"])
    assert seen["n_envs"] == {1, 3, 5, 63, 64, 65, 130, 257} and seen["gamma"] == {0.0, 0.9, 0.99, 1.0} and seen["steps_per_launch"] == {0, 1, 5, 64}
    assert {0, 64, 1000003, (1 << 31) - 65} <= seen["env_offset"] and (1 << 32) - 1 in seen["ids"]
    if mod is fe:
        assert seen["algo"] == {23, 25, 26} and {(d, o) for d in seen["domain"] for o in seen["order"]} >= set(fe.REG)
        assert seen["max_episode_steps"] == {1, 2, 7, 25, 200} and seen["lam"] == {0.0, 0.5, 0.8, 1.0}
    else:
        assert seen["algo"] == {21, 28} and seen["order"] == {1, 2, 3, 4, 5} and seen["max_episode_steps"] == {0, 1, 7, 23, 200}
        assert seen["n_steps"] == {1, 2, 3, 4, 7, 100}


def test_the_parts_of_a_configuration_the_samplers_fix_are_refused_otherwise():
    """(the admission the samplers rely on: a record agent without a cap and NAC's period 0 are EINVAL, so EHIP above does mean admitted)"""
    rng = np.random.default_rng(1)
    kw = fe.sample(rng, 0)
    assert create_rc({}, **dict(kw, n_envs=4, env_offset=0, max_episode_steps=0))[0] == EINVAL
    kw = fb.sample(rng, 1)
    assert kw["algo"] == 28 and create_rc({}, **dict(kw, n_envs=4, env_offset=0, n_steps=0))[0] == EINVAL


@pytest.mark.parametrize("algo", [25, 26])
def test_no_suite_case_of_the_lstd_agents_diverges_in_the_restatement(orc, algo):
    """the committed slice (SEED, CASES cases per agent): the f64 accumulators of every replayed learner of every batch leg stay finite -- at most
    2 % of the cases may be counted `diverged`, none of 24"""
    diverged = replayed = 0
    for idx in range(CASES):
        rng = fe.case_rng(SEED, idx, (algo,))
        kw = fe.sample(rng, idx, (algo,))
        io = fe.batch_inputs(rng, kw)
        bad = False
        for i in io["rep"]:
            if io["L"][i]:
                st, td = fe.lstd_replay(kw, io, i)
                bad |= not (fe.finite_state(st) and np.isfinite(td).all())
                replayed += 1
        diverged += bad
    assert replayed >= 2 * CASES and diverged <= 0.02 * CASES, (diverged, replayed)


def _beta_left_out(orc, algo):
    """(replayed learner-rounds, those the restatement leaves out) over the committed slice of one Beta agent, from the host inputs alone: the
    oracle's f64 features stand in for the device's projection"""
    left = replayed = 0
    for idx in range(CASES):
        rng = fb.case_rng(SEED, idx, (algo,))
        kw = fb.sample(rng, idx, (algo,))
        io = fb.f64_inputs(rng, kw)
        W = io["W"].astype(np.float64)
        cur = {i: list(io["init"][i]) for _, _, _, _, _, _, rep in io["rounds"] for i in rep} if algo == 21 else None
        for t, (frm, a, rew, nxt, term, M, rep) in enumerate(io["rounds"]):
            assert 1 <= M <= kw["n_envs"] and all(0 <= i < M for i in rep) and a.min() >= 0.0 and a.max() <= 1.0
            if algo == 28:
                for i in rep:
                    replayed += 1
                    left += fb.left_out_nac(kw, W[i], fb.features(kw, nxt[:, i]), i, t, bool(term[i]))[1]
            else:
                for i in [i for i in cur if i < M]:
                    mus = []
                    _, *cur[i] = ilstd(*cur[i], fb.features(kw, frm[:, i]), fb.features(kw, nxt[:, i]), float(rew[i]), bool(term[i]), kw["gamma"], kw["lr"],
                                       kw["n_steps"], literal=False, rounds=mus)
                    if i in rep:
                        replayed += 1
                        left += any(near_tie_band(m) for m in mus)
    return replayed, left


@pytest.mark.parametrize("algo", [21, 28])
def test_the_suite_slices_of_the_beta_agents_leave_out_at_most_five_percent(orc, algo):
    replayed, left = _beta_left_out(orc, algo)
    print("replayed %d, left out %d" % (replayed, left))
    assert replayed >= 2 * CASES and left <= fb.LEFT_OUT_CAP * replayed, (left, replayed)


def test_the_beta_samplers_columns_and_actions_reach_every_branch():
    rng = np.random.default_rng(5)
    W = fb.columns(rng, 65, 16)
    const = W[np.arange(65) % 4 != 3, 15, :]
    assert not W[np.arange(65) % 4 != 3, :15].any() and np.abs(W[np.arange(65) % 4 == 3]).sum(axis=1).max() <= 3.0 + 1e-5
    pairs = {(int(x >= 10) + 2 * int(x <= -20), int(y >= 10) + 2 * int(y <= -20)) for x, y in const}
    assert pairs == {(p, q) for p in (0, 1, 2) for q in (0, 1, 2)}                       # (0: inside (-17, 10), 1: >= 10, 2: <= -20)
    assert ((const > -17.0) | (const <= -20.0)).all() and np.abs(const).max() <= 30.0
    a = np.concatenate([fb.edge_actions(rng, 257) for _ in range(8)])
    assert a.dtype == np.float32 and a.min() == 0.0 and a.max() == 1.0
    for edge in (np.float32(bn.LO), np.float32(bn.HI), np.nextafter(np.float32(0), np.float32(1)), np.nextafter(np.float32(1), np.float32(0))):
        assert (a == edge).any(), edge
    assert ((a > 0.01) & (a < 0.99)).sum() > len(a) // 3


def test_td_chain_in_device_order_agrees_with_gradient_mc_in_f64(orc):
    """the reference of GradientMC's batch leg against the literal f64 restatement, on the first committed case with a batch of >= 5 rows.
    Per visit the f32 chain rounds F products and sums for the prediction, the return, and two operations per weight; its features are f32
    polynomials a few ulps from the f64 cosines: 8 F eps32 per visit, relative to 1 + max |w| + max |return|, summed over the visits (the
    update contracts: lr |phi|^2 <= 0.2)"""
    for idx in range(CASES):
        rng = fe.case_rng(SEED, idx, (23,))
        kw = fe.sample(rng, idx, (23,))
        io = fe.batch_inputs(rng, kw)
        if io["T"] >= 5:
            break
    i = io["rep"][-1]
    n, F = int(io["L"][i]), io["F"]
    assert n == io["T"] >= 5
    ag = orc.make_agent(domain=kw["domain"], order=kw["order"], algo=orc.TD, policy=orc.RANDOM, gamma=kw["gamma"], lr=kw["lr"])
    w32 = io["W"][i].copy()
    _, rets32 = td_chain(orc, ag, w32, io["S"][:n, :, i], io["R"][:n, i], kw["gamma"], "f32d")
    phis = [orc.fourier_project(kw["domain"], kw["order"], io["S"][k, :, i]) for k in range(n)]
    w64, _, rets64 = gradient_mc(io["W"][i], phis, io["R"][:n, i].astype(np.float64), kw["gamma"], kw["lr"])
    scale = 1.0 + np.abs(w64).max() + np.abs(rets64).max()
    assert np.abs(rets32 - rets64).max() <= 2 * n * EPS32 * scale
    assert np.abs(w32 - w64).max() <= 8 * F * n * EPS32 * scale, (np.abs(w32 - w64).max(), 8 * F * n * EPS32 * scale)
    assert np.abs(w64 - io["W"][i]).max() > 8 * F * n * EPS32 * scale                     # (the batch moved w by more than the bound)


@pytest.mark.parametrize("algo", [25, 26])
def test_the_index_order_lstd_restatement_agrees_with_numpy(orc, algo):
    """tests/lstd_batch_numpy.handle (Python floats, the device's operation order) against the same rule in vectorised numpy, on the first
    committed case with >= 3 rows: A, b, z within the GPU bound's 16 F T eps (both are f64 sums of the same terms in different orders),
    theta by the residual of its own A and b"""
    for idx in range(CASES):
        rng = fe.case_rng(SEED, idx, (algo,))
        kw = fe.sample(rng, idx, (algo,))
        io = fe.batch_inputs(rng, kw)
        if io["T"] >= 3 and not io["planted"]:
            break
    i = io["rep"][-1]
    n, F, gamma = int(io["L"][i]), io["F"], kw["gamma"]
    assert n == io["T"] >= 3
    st, td = fe.lstd_replay(kw, io, i)
    theta, A, b, z, _ = [np.array(x, dtype=np.float64) if not isinstance(x, int) else x for x in io["init"][i]]
    rows = [(orc.fourier_project(kw["domain"], kw["order"], io["S"][k, :, i]), orc.fourier_project(kw["domain"], kw["order"], io["S2"][k, :, i]),
             float(io["R"][k, i]), bool(io["Tm"][k, i])) for k in range(n)]
    want_td = [r - ps @ theta if tm else r + gamma * (pn @ theta) - ps @ theta for ps, pn, r, tm in rows]
    if algo == 25:
        for ps, pn, r, tm in rows:
            b = b + r * ps
            A = A + np.outer(ps, ps if tm else ps - gamma * pn)
    else:
        for ps, pn, r, tm in reversed(rows):
            z = kw["lam"] * gamma * z + ps
            b = b + r * z
            A = A + np.outer(z, ps if tm else ps - gamma * pn)
            if tm:
                z = np.zeros(F)
        assert np.abs(np.array(st["z"]) - z).max() <= 16 * F * n * EPS64 * (1 + np.abs(z).max())
    tol = 16 * F * n * EPS64
    assert np.abs(np.array(st["A"]) - A).max() <= tol * (1 + np.abs(A).max()) and np.abs(np.array(st["b"]) - b).max() <= tol * (1 + np.abs(b).max())
    assert np.abs(np.array(td) - np.array(want_td)).max() <= tol * (1 + np.abs(want_td).max())
    assert st["singular"] == io["init"][i][4] and residual(st["A"], st["b"], st["theta"]) <= F * EPS64


def test_nac_handle_f32_agrees_with_nac_handle_in_f64():
    """the bit-for-bit reference of nac_update against the f64 form on the first committed NAC case: the norm is a sum of 2F rounded squares and a
    rounded square root, the step one division and one fused multiply-add per element -- (2F + 8) eps32 relative to 1 + max |W'| (the step is
    at most alpha)"""
    rng = fb.case_rng(SEED, 0, (28,))
    kw = fb.sample(rng, 0, (28,))
    io = fb.f64_inputs(rng, kw)
    F = io["F"]
    for i in range(min(kw["n_envs"], 8)):
        got, norm = nn.nac_handle_f32(io["w_update"][i], io["W"][i], kw["alpha"])
        want, wnorm = nn.nac_handle(io["w_update"][i], io["W"][i], kw["alpha"])
        assert abs(float(norm) - wnorm) <= (2 * F + 8) * EPS32 * wnorm, (i, norm, wnorm)
        assert np.abs(got - want).max() <= (2 * F + 8) * EPS32 * (1 + np.abs(want).max()), i
    norms = [float(nn.nac_handle_f32(io["w_update"][j], io["W"][j], kw["alpha"])[1]) for j in range(min(kw["n_envs"], 3))]
    assert norms[0] == float(np.float32(1e-3))                                             # the learner a relative 1e-7 .. 1e-4 below the floor
