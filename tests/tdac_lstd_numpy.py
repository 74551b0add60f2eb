"""ActorCritic::tdac with the iLSTD critic (RSRL_ILSTD_ACTOR_CRITIC) restated in numpy, in the order of examples/tdac.rs: iLSTD::handle in f64
(tests/lstd_numpy.ilstd, the device's form of the mu update), then TDCritic's target from the UPDATED f64 theta, then the Gibbs actor's step
(tests/ac_numpy.actor_step, the rule tests/tdac_numpy.py applies) scaled by alpha * c rounded ONCE to f32.  Shared by the CPU and GPU tests."""
import numpy as np

from tests.ac_numpy import actor_step
from tests.lstd_numpy import dot, ilstd


def critic_target(theta, phi_s, phi_n, r, term, gamma):
    """TDCritic::target: r - V(s') on a terminal transition (V of the terminal state itself), else r + gamma V(s') - V(s); V = phi . theta summed in
    index order"""
    v_s, v_n = dot(phi_s, theta), dot(phi_n, theta)
    return r - v_n if term else r + gamma * v_n - v_s


def tdac_lstd_rule(theta, A, mu, Th, phi_s, phi_n, a, r, term, gamma, lr, n_updates, alpha, tau, rounds=None, literal=False):
    """one transition -> (iLSTD's diagnostic, theta', A', mu', the actor's theta').  lr is iLSTD's alpha (the critic's rate), alpha ActorCritic's.
    phi_s / phi_n are the f64 features; the actor reads the same ones (the device's f32 features differ from them by the feature error the actor's
    bound allows for).  rounds: receives mu at the start of every solve round"""
    diag, theta2, A2, mu2 = ilstd(theta, A, mu, phi_s, phi_n, r, term, gamma, lr, n_updates, literal=literal, rounds=rounds)
    c = critic_target(theta2, phi_s, phi_n, r, term, gamma)
    e = float(np.float32(alpha * c))                          # the one rounding out of f64
    return diag, theta2, A2, mu2, actor_step(np.asarray(Th, dtype=np.float64), np.asarray(phi_s, dtype=np.float64), a, e, tau)


def n_actions(orc, domain):
    return 2 if domain == orc.CART_POLE else 3


def handle_case(orc, domain, order, N=64, rounds=3, gamma=0.95, lr=0.05, n_updates=3, alpha=0.3, tau=1.0):
    """the GPU handle test's inputs and what the rule makes of them, computed once per configuration on the CPU: a well-conditioned random state per
    learner (tests/test_gpu_lstd.py's: A near I), a random actor, `rounds` rounds of transitions stepped by the oracle's device-order domain (a
    quarter more of them flagged terminal).  -> dict(init = [(theta, A, mu, Th f32)], rounds = [(from [D][N], a, r, to [D][N], term)],
    diag [rounds][N], first = the actor after round 1, final = [(theta, A, mu, Th)], skipped [N]: a solve round's |mu| lay within 1e-9 of
    argmaxima's 1e-7 tie band (tests/lstd_numpy.near_tie_band) -- a rounding may move a j in or out of the set)"""
    from tests.lstd_numpy import near_tie_band
    rng = np.random.default_rng(domain * 100 + order * 10 + 21)
    lo, hi = orc.domain_bounds(domain)
    D, F, A = len(lo), (order + 1) ** len(lo), n_actions(orc, domain)
    init = []
    for _ in range(N):
        M = rng.normal(0.0, 1.0, size=(F, F))
        init.append((rng.normal(0.0, 0.5, size=F), np.eye(F) + 0.1 * M / np.sqrt(F), rng.normal(0.0, 1.0, size=F),
                     rng.normal(0.0, 0.3, size=(F, A)).astype(np.float32)))
    cur = [[t, m, u, th.astype(np.float64)] for t, m, u, th in init]
    out_rounds, diag, first, skipped = [], np.zeros((rounds, N)), None, np.zeros(N, dtype=bool)
    for k in range(rounds):
        frm = rng.uniform(lo, hi, size=(N, D)).T.astype(np.float32)
        a = rng.integers(0, A, size=N).astype(np.int32)
        nxt, rew, term = np.zeros_like(frm), np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.uint8)
        for i in range(N):
            ns, r, t = orc.domain_step(domain, frm[:, i], int(a[i]), prec="f32d")
            nxt[:, i], rew[i], term[i] = np.asarray(ns, dtype=np.float32), np.float32(r), bool(t)
        term = (term.astype(bool) | (rng.random(N) < 0.25)).astype(np.uint8)
        out_rounds.append((frm, a, rew, nxt, term))
        for i in range(N):
            phi_s, phi_n = orc.fourier_project(domain, order, frm[:, i]), orc.fourier_project(domain, order, nxt[:, i])
            mus = []
            diag[k, i], *cur[i] = tdac_lstd_rule(*cur[i], phi_s, phi_n, int(a[i]), float(rew[i]), bool(term[i]), gamma, lr, n_updates, alpha, tau, rounds=mus)
            skipped[i] |= any(near_tie_band(m) for m in mus)
        if k == 0:
            first = [c[3].copy() for c in cur]
    return dict(init=init, rounds=out_rounds, diag=diag, first=first, final=[tuple(c) for c in cur], skipped=skipped, F=F, A=A,
                params=dict(gamma=gamma, lr=lr, n_steps=n_updates, alpha=alpha, tau=tau))
