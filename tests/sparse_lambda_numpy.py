"""SARSA(lambda) / Q(lambda) over ONE shared tile-coded table with the reference's UNBOUNDED trace, restated in f64 numpy: the synchronous mini-batch
rule of rsrl_amd/csrc/kernels_sparse_lambda.hpp with a DENSE (F, A) trace per learner (traces.rs:188-240 over params/sparse.rs:13-97 grows without limit;
the device cuts a learner's list at 512 entries, 512 / T per tiling, by writing over the smallest |v|).  Next to the trace runs the bound B on what the cap
can cost, computed from the dense trace alone.  Shared by the CPU and GPU tests.

The bound, for one (learner, tiling).  All three rules are z <- clip?(rate * z + g), g >= 0: monotone, and a contraction by `rate` in L1.  Read the capped
list as a dense vector in which evicted entries are 0; then 0 <= z_dev <= z_ref elementwise, and D = ||z_ref - z_dev||_1 obeys D' <= rate * D + m with m the
evicted value.  A full sub-list holds CAP distinct keys other than the step's new key, each <= z_ref at its key, so m <= the CAP-th largest decayed z_ref
value of the tiling among the keys other than the new one.  Hence B' = rate * B + kth (an eviction charged at EVERY step), B = 0 after a terminal transition
or a Watkins cut (both sides are emptied), and D <= B."""
import numpy as np

SPARSE_CAP = 512          # kSparseCap: entries per learner, SPARSE_CAP / T per tiling


def trace_rate(gamma, lam, alpha, rule):
    """the decay of the three rules (traces.rs:198, :215, :236); rule: 0 accumulate, 1 saturate, 2 dutch"""
    return gamma * lam * (1.0 - alpha) if rule == 2 else gamma * lam


def fp32_slack(z_ref, rate):
    """what an fp32 trace entry may differ from the f64 one by: one rounding of `rate` and one per fma, over an entry's mass-weighted age of at most
    1 / (1 - rate), times 2"""
    return 2.0 * 2.0 ** -23 / (1.0 - rate) * np.maximum(1.0, z_ref)


class DenseTraces:
    """N learners' dense traces Z (N, F, A) and the bound B (N, T), advanced from a tape: update() per handled transition, then reset() where it was terminal"""

    def __init__(self, N, T, F, A, rate, rule):
        self.N, self.T, self.F, self.A, self.rate, self.rule = N, T, F, A, float(rate), rule
        self.cells, self.cap = F // T, SPARSE_CAP // T
        self.S = self.cells * A                                   # entries of one tiling's slice
        self.Z = np.zeros((N, F, A))
        self.B = np.zeros((N, T))
        self.live = np.zeros((N, T), dtype=np.int64)              # non-zero entries per tiling (an f64 entry does not decay to 0 within these horizons)
        self._n, self._t = np.ogrid[:N, :T]

    def update(self, idx, action, cut=None):
        """idx (N, T): the tile indices of the from-states; action (N,); cut (N,) bool: Watkins's cut, the trace is emptied first (q_lambda.rs:62-66)"""
        if cut is not None and cut.any():
            self.Z[cut] = 0.0
            self.B[cut] = 0.0
            self.live[cut] = 0
        self.Z *= self.rate
        Zt = self.Z.reshape(self.N, self.T, self.S)               # (a view: tiling t owns rows [t * cells, (t + 1) * cells))
        key = (idx - np.arange(self.T) * self.cells) * self.A + np.asarray(action)[:, None]
        held = Zt[self._n, self._t, key]
        kth = 0.0
        if self.S > self.cap:
            if (self.live - (held != 0) >= self.cap).any():       # (else fewer than CAP other keys are held: the CAP-th largest is 0)
                Zt[self._n, self._t, key] = 0.0                   # among the keys other than the new one
                kth = np.partition(Zt, self.S - self.cap, axis=-1)[..., self.S - self.cap]
        self.B = self.rate * self.B + kth
        self.live += held == 0
        v = held + 1.0
        if self.rule == 1:
            v = np.clip(v, -1.0, 1.0)                             # (every other entry is in [0, 1] already)
        Zt[self._n, self._t, key] = v

    def reset(self, terminal):
        terminal = np.asarray(terminal, dtype=bool)
        self.Z[terminal] = 0.0
        self.B[terminal] = 0.0
        self.live[terminal] = 0

    def tilings(self, z=None):
        """(N, T, S): the traces (or any (N, F, A) array) tiling by tiling"""
        return (self.Z if z is None else np.asarray(z)).reshape(self.N, self.T, self.S)

    def slack(self):
        """(N, T): the L1 fp32 slack of a tiling, the sum of fp32_slack over its non-zero entries"""
        Zt = self.tilings()                                        # (max(1, z) = 1 + max(0, z - 1), summed over the non-zero entries)
        over = np.maximum(Zt - 1.0, 0.0).sum(-1) if self.rule != 1 else 0.0
        return fp32_slack(0.0, self.rate) * (self.live + over)


class DenseLambdaTeacher:
    """the driver loop in f64 on the oracle's primitives and draws, successor states rounded to fp32 (as orc_run_teacher does): step() is one batch-step.
    kw: make_agent's (domain, n_tilings, tiles_per_dim, algo, policy, epsilon, tau, gamma, lam, trace, alpha, max_episode_steps)"""

    def __init__(self, orc, N, seed, **kw):
        self.orc, self.N, self.seed = orc, N, seed
        self.ag = orc.make_agent(**dict(kw, basis=orc.TILE, shared_w=True, seed=seed))
        self.domain, self.policy, self.sarsa = kw["domain"], kw["policy"], kw["algo"] == orc.SARSA_LAMBDA
        assert kw["algo"] in (orc.SARSA_LAMBDA, orc.Q_LAMBDA)
        self.eps, self.tau, self.gamma, self.alpha = kw.get("epsilon", 0.1), kw.get("tau", 1.0), kw["gamma"], kw["alpha"]
        self.cap_steps = kw.get("max_episode_steps", 1000)
        self.T, self.F, self.A = self.ag.basis.n_tilings, orc.n_features(self.ag), self.ag.n_actions
        self.rate = trace_rate(self.gamma, kw["lam"], self.alpha, kw.get("trace", 0))
        self.tr = DenseTraces(N, self.T, self.F, self.A, self.rate, kw.get("trace", 0))
        self.W = np.zeros((self.F, self.A))
        self.k = 0
        self.s = np.stack([self._f32(orc.domain_reset(self.domain, "f64")) for _ in range(N)])
        self.idx = np.stack([orc.tile_indices(self.ag, s) for s in self.s])
        self.ep = np.zeros(N, dtype=np.int64)
        self.a = np.array([self._sample(np.zeros(self.A), i, orc.BLK_INIT) for i in range(N)], dtype=np.int32)

    @staticmethod
    def _f32(s):
        return np.asarray(s, dtype=np.float32).astype(np.float64)

    def _sample(self, q, i, block):
        return self.orc.policy_sample(self.policy, q, self.orc.draw(self.seed, i, self.k, block), eps=self.eps, tau=self.tau)

    def _q(self, idx):
        q = np.zeros((len(idx), self.A))
        for t in range(self.T):                                    # (the oracle's order: tiling by tiling)
            q += self.W[idx[:, t]]
        return q

    def step(self, want_slack=False):
        """-> dict: the tape frm (N, D), action, reward, to, terminal (uint8) and td; cut (N,) bool; margin, qmax (N,): the gap between the best and the
        second-best Q(s, .) and the best itself (what a Watkins cut is decided by), untouched (N,) bool: every weight under s is
        still exactly 0 (a tie both sides give to the first action); z_l1 (N,), B (N, T), slack (N, T; on request): the traces the table update used"""
        orc, N = self.orc, self.N
        frm, act = self.s.copy(), self.a.copy()
        to, rew, term = np.empty_like(frm), np.empty(N), np.zeros(N, dtype=np.uint8)
        idn = np.empty_like(self.idx)
        for i in range(N):
            ns, rew[i], tm = orc.domain_step(self.domain, frm[i], act[i], "f64")
            to[i], term[i] = self._f32(ns), tm
            idn[i] = orc.tile_indices(self.ag, to[i])
        self.ep += 1
        trunc = (term == 0) & (self.cap_steps > 0) & (self.ep >= self.cap_steps)
        qs, qn = self._q(self.idx), self._q(idn)
        n = np.arange(N)
        top = np.sort(qs, axis=1)
        cut = None if self.sarsa else np.array([orc.argmax_first(q) for q in qs]) != act    # (utils.rs:23-34: a later action wins by more than 1e-7 only)
        boot = np.zeros(N)                                         # Q(s', a'): the agent's own draw (SARSA) or the maximum (Q)
        for i in np.flatnonzero(term == 0):
            boot[i] = qn[i, self._sample(qn[i], i, orc.BLK_INNER)] if self.sarsa else qn[i].max()
        td = np.where(term != 0, rew - qs[n, act], rew + self.gamma * boot - qs[n, act])
        self.tr.update(self.idx, act, cut)
        out = dict(frm=frm, action=act, reward=rew, to=to.copy(), terminal=term, td=td, cut=np.zeros(N, dtype=bool) if cut is None else cut,
                   margin=top[:, -1] - top[:, -2], qmax=top[:, -1], untouched=(self.W[self.idx] == 0).all((1, 2)),
                   z_l1=self.tr.Z.sum((1, 2)), B=self.tr.B.copy(), slack=self.tr.slack() if want_slack else None)
        dW = np.zeros_like(self.W)
        for i in range(N):                                         # (the oracle's order: learner by learner)
            dW += (self.alpha * td[i]) * self.tr.Z[i]
        self.W += dW
        self.tr.reset(term)
        for i in range(N):
            if term[i] or trunc[i]:
                to[i] = self._f32(orc.domain_reset(self.domain, "f64"))         # (the tape holds a copy)
                idn[i] = orc.tile_indices(self.ag, to[i])
                self.ep[i] = 0
        q = self._q(idn)
        for i in range(N):
            self.a[i] = self._sample(q[i], i, orc.BLK_STEP)
        self.s, self.idx = to, idn
        self.k += 1
        return out


class CutWatch:
    """which learners' traces a Q(lambda) comparison leaves out: a Watkins cut the reference decides by a margin under 1e-5 (1 + |Q|) can fall the other way in
    fp32, so from such a step the learner is left out until both sides empty its trace again (a terminal transition, or a cut decided by a clear margin).
    Exact ties over untouched weights do not count: both sides take argmax_first."""

    def __init__(self, N):
        self.out = np.zeros(N, dtype=bool)
        self.left_out = self.steps = 0

    def step(self, o):
        """o: DenseLambdaTeacher.step()'s dict -> the learners left out after this step"""
        low = (o["margin"] < 1e-5 * (1.0 + np.abs(o["qmax"]))) & ~o["untouched"]
        self.out &= ~(o["cut"] & ~low)
        self.out |= low
        self.out &= o["terminal"] == 0
        self.left_out += int(self.out.sum()); self.steps += len(self.out)
        return self.out

    @property
    def fraction(self):
        return self.left_out / max(1, self.steps)


def follow_tape(orc, ag, tr, t, cut=None):
    """advance DenseTraces `tr` by one batch-step of a tape t (frm, action, terminal): what the reference's trace holds after the same transitions"""
    idx = np.stack([orc.tile_indices(ag, s) for s in t["frm"]])
    tr.update(idx, t["action"], cut)
    tr.reset(t["terminal"])


def deficit(tr, z_dev):
    """z_dev (N, F, A): the capped lists as dense matrices -> (D (N, T) = ||z_ref - z_dev||_1 per tiling, z_dev - z_ref (N, T, S))"""
    diff = tr.tilings(np.asarray(z_dev, dtype=np.float64)) - tr.tilings()
    return np.abs(diff).sum(-1), diff
