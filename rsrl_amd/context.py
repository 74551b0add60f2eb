"""`Context`: one (domain, basis, algo, policy, N, W-mode) instance on one MI355X -- a thin numpy-facing
wrapper over the C ABI (include/rsrl_hip.h).  All compute happens in librsrl_hip.so's HIP kernels."""
import ctypes as C

import numpy as np

from . import _abi

MOUNTAIN_CAR, CART_POLE, ACROBOT, HIV_TREATMENT = 0, 1, 2, 3
CONTINUOUS_MOUNTAIN_CAR = 4                     # mountain_car/continuous.rs: one f32 action in [-1, 1] (Context.continuous; ILSTD_ACTOR_CRITIC, NAC and CONTINUOUS_TD_ACTOR_CRITIC with BETA; NAC, CACLA and CONTINUOUS_TD_ACTOR_CRITIC with GAUSSIAN)
CLIFF_WALK = 5                                  # cliff_walk.rs, CliffWalk::default() (height 5, width 12): states (x, y) as exact integers in f32, 4 actions (N, E, S, W); with basis TABLE only
FOURIER, TILE_CODING = 0, 1
TABLE = 2                                       # fa/tabular/dense.rs, Table<Array2<f64>>: 60 rows (row = x * 5 + y) of 4 entries, with CLIFF_WALK only; weights (60, 4); lr scales the error (lr = 1: the reference's rule)
QLEARNING, SARSA, EXPECTED_SARSA, SARSA_LAMBDA, Q_LAMBDA, PAL, GREEDY_GQ, TD, TD_LAMBDA, Q_SIGMA = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
ACTOR_CRITIC, Q_ACTOR_CRITIC = 10, 11          # ActorCritic (control/ac.rs) with a Gibbs actor and a SARSA critic: a2c.rs's closure / QCritic
TD_ACTOR_CRITIC = 13                           # ActorCritic::tdac: the Gibbs actor with TDCritic over a TD(0) V (12 is no algo)
REINFORCE, BASELINE_REINFORCE = 15, 16         # (14 is no algo) control/mc: REINFORCE<Gibbs>, BaselineREINFORCE<B, Gibbs> (Handler<&Batch>: handle_batch)
RECURSIVE_LSTD, ILSTD = 18, 19                  # (17 is no algo) prediction/lstd: RecursiveLSTD, iLSTD (f64 theta and F x F matrix: get/set_lstd_state)
ILSTD_ACTOR_CRITIC = 21                        # (20 is no algo) ActorCritic::tdac over iLSTD, tdac.rs's agent: lr = iLSTD's alpha, n_steps = its n_updates, alpha = the actor's
GRADIENT_MC = 23                               # (22 is no algo) prediction/mc.rs: GradientMC (Handler<&Trajectory>: handle_batch; episode_record)
LSTD, LSTD_LAMBDA = 25, 26                      # (24 is no algo) prediction/lstd: LSTD, LSTDLambda (Handler<&Batch> on whole transitions: handle_transitions; lstd_solve; get/set_lstd_batch_state)
NAC = 28                                        # (27 is no algo) control/nac.rs with the BETA (nac_beta.rs) or the GAUSSIAN policy (nac.rs) and a SARSA critic over the stable compatible basis on CONTINUOUS_MOUNTAIN_CAR: n_weight_rows = 3 F; q_evaluate_f32; nac_update
GTD2, TDC = 30, 31                              # (29 is no algo) prediction/td: GTD2, TDC -- gradient TD with a second weight column (get/set_td_weights, (F, 1)); lr scales theta's moves, lr_td w's
CACLA = 33                                      # (32 is no algo) control/cacla.rs over the GAUSSIAN policy with a TD(0) critic on CONTINUOUS_MOUNTAIN_CAR: lr = TD's rate, alpha = CACLA's; q_evaluate -> V(s); handle = eval.handle then CACLA::handle
CONTINUOUS_TD_ACTOR_CRITIC = 35                 # (34 is no algo) ActorCritic::tdac (control/ac.rs) with a TD(0) critic over the GAUSSIAN or the BETA policy on CONTINUOUS_MOUNTAIN_CAR: lr = TD's rate, alpha = ActorCritic's; q_evaluate -> V(s); handle = eval.handle then ActorCritic::handle; the domain sees a (GAUSSIAN) or 2a - 1 (BETA)
TRACE_ACCUMULATE, TRACE_SATURATE, TRACE_DUTCH = 0, 1, 2
GREEDY, EPSILON_GREEDY, SOFTMAX, RANDOM = 0, 1, 2, 3
BETA = 4                                        # policies/beta.rs over two Softplus-composed scalar LFAs: ILSTD_ACTOR_CRITIC on CONTINUOUS_MOUNTAIN_CAR
GIBBS_NAC = 37                                  # (36 is no algo) control/nac.rs over the Gibbs policy (nac_softmax.rs: policy=SOFTMAX) and a SARSA critic over the stable compatible basis on the discrete domains: n_weight_rows = (A + 1) F; q_evaluate -> (A, M); handle = critic.handle; nac_update; n_steps = the actor's period
LAMBDA_LSPE = 39                                # (38 and 40 are no algos) prediction/lstd: LambdaLSPE (LSTD_LAMBDA's calls; get/set_lstd_batch_state carry z[0] = delta, z[1] = rows)
GAUSSIAN = 6                                    # (5 is no policy) policies/gaussian: the mean a scalar LFA, the stddev a Softplus-composed one: NAC (nac.rs) and CACLA on CONTINUOUS_MOUNTAIN_CAR
W_PER_ENV, W_SHARED = 0, 1
W_F32, W_BF16 = 0, 1
EXCHANGE_RCCL, EXCHANGE_PEER, EXCHANGE_AUTO = 0, 1, 2
PEER_HANDLE_BYTES = 128


def _p(a):
    """numpy array / raw device pointer (int) / None -> void*"""
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    return a.ctypes.data_as(C.c_void_p)


def _in(a, dtype, shape=None):
    if a is None or isinstance(a, int):
        return a
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def can_access_peer(device, peer_device):
    """True if `device` reads and writes `peer_device`'s memory directly (what the one-hop peer exchange needs of every pair of ranks)"""
    rc = _abi.lib().rsrl_hip_can_access_peer(int(device), int(peer_device))
    if rc < 0:
        _abi.check(rc)
    return rc == 1


def device_identity(device):
    """which PHYSICAL device ordinal `device` is (PCI domain : bus : device): the same number in every process of the node, whatever
    HIP_VISIBLE_DEVICES each runs under"""
    out = C.c_uint64()
    _abi.check(_abi.lib().rsrl_hip_device_identity(int(device), C.byref(out)))
    return int(out.value)


def device_count():
    """visible HIP devices (raises RsrlHipError when the runtime finds none)"""
    n = _abi.lib().rsrl_hip_device_count()
    if n < 0:
        _abi.check(n)
    return n


class Context:
    """One object graph of the reference on one GPU, times `n_envs` independent environments in lock-step:

        env    = MountainCar | CartPole | Acrobot | HIVTreatment | CliffWalk ::default()        (domain)
        basis  = Fourier::from_space(order, ..).with_bias() | TileCoding           (basis, order | n_tilings, tiles_per_dim)
                 | Table::zeros((60, 4)) for CliffWalk                             (basis=TABLE: the one-step agents on a tabular Q)
        q_func = make_shared(LFA::vector(basis, SGD(lr), n_actions))               (lr; weight_mode: one per env or one shared)
        policy = Greedy | EpsilonGreedy(epsilon) | Softmax(tau) | Random           (policy, epsilon, tau)
        agent  = QLearning{gamma} | SARSA | ExpectedSARSA{alpha} | PAL{alpha}      (algo, gamma, alpha)
                 | SARSALambda / QLambda {trace(gamma, lam), alpha}                (lam, trace)
                 | GreedyGQ {fa_td = LFA(SGD(lr_td))} | TD | TDLambda              (lr_td; TD/TDLambda need policy=RANDOM)
                 | GTD2 {fa_theta, fa_w} | TDC {q_func, td_est}                     (lr: theta's moves, lr_td: w's; policy=RANDOM)
                 | QSigma {alpha, gamma, sigma, n_steps}                            (sigma, n_steps)
                 SARSA / ExpectedSARSA / SARSALambda own a policy of their own       (agent_policy, agent_epsilon, agent_tau;
                                                                                     None = the behaviour policy object)

    (rsrl/examples/q_learning.rs:19-32 and the other examples).  `seed` keys the per-env Philox streams by GLOBAL env id
    (`env_offset` + local index), so a sharded run reproduces the unsharded one bit for bit.  `steps_per_launch`: fuse
    depth of `train` (0 = library default: 4096 for the register-resident loops, 256 otherwise; 1 = one batch-step per launch).  Arrays are SoA: states `(D, M)`, actions `(M,)`; weights
    `(F, n_out)` row-major like the reference's `Parameterised::weights()`.  Every method raises `RsrlHipError` with the
    ABI's message on failure; there is no CPU fallback."""

    def __init__(self, domain=MOUNTAIN_CAR, basis=FOURIER, order=5, n_tilings=8, tiles_per_dim=8,
                 algo=QLEARNING, policy=GREEDY, weight_mode=W_PER_ENV, weight_dtype=W_F32,
                 n_envs=1, env_offset=0, seed=0, gamma=0.9, lr=0.001, alpha=1.0, epsilon=0.1, tau=1.0,
                 max_episode_steps=0, steps_per_launch=0, device=0, stream=None, lam=0.0, trace=TRACE_ACCUMULATE, lr_td=0.0,
                 agent_policy=None, agent_epsilon=0.1, agent_tau=1.0, exchange=EXCHANGE_AUTO, sigma=0.0, n_steps=1, peer_timeout_ms=0,
                 epsilon_decay=1.0, epsilon_min=0.0):
        self._L = _abi.lib()
        cfg = _abi.Config()
        _abi.check(self._L.rsrl_hip_config_init(C.byref(cfg)))
        cfg.device, cfg.domain, cfg.basis, cfg.order = device, domain, basis, order
        cfg.n_tilings, cfg.tiles_per_dim = n_tilings, tiles_per_dim
        cfg.algo, cfg.policy, cfg.weight_mode, cfg.weight_dtype = algo, policy, weight_mode, weight_dtype
        cfg.max_episode_steps, cfg.n_envs, cfg.env_offset, cfg.seed = max_episode_steps, n_envs, env_offset, seed
        cfg.gamma, cfg.lr, cfg.alpha, cfg.epsilon, cfg.tau = gamma, lr, alpha, epsilon, tau
        cfg.steps_per_launch = steps_per_launch
        cfg.lam, cfg.trace, cfg.lr_td = lam, trace, lr_td
        cfg.stream = stream
        # the policy owned by the agent (SARSA's inner draw, ExpectedSARSA's expectation); None = the behaviour policy itself
        cfg.agent_policy = -1 if agent_policy is None else int(agent_policy)
        cfg.agent_epsilon, cfg.agent_tau, cfg.exchange = agent_epsilon, agent_tau, exchange
        cfg.sigma, cfg.n_steps = sigma, n_steps                   # QSigma{sigma, Backup::new(n_steps)}
        cfg.peer_timeout_ms = int(peer_timeout_ms)                # bound of the in-kernel waits of the shared-W exchange (0 = default)
        # the reference drivers' schedule `agent.policy.epsilon *= 0.995` once per episode of a learner (examples/sarsa_lambda.rs:68)
        cfg.epsilon_decay, cfg.epsilon_min = float(epsilon_decay), float(epsilon_min)
        self.cfg = cfg
        self._h = C.c_void_p()
        _abi.check(self._L.rsrl_hip_create(C.byref(cfg), C.byref(self._h)))
        self.N = int(n_envs)
        self.D = self._L.rsrl_hip_state_dim(self._h)
        self.A = self._L.rsrl_hip_n_actions(self._h)
        self.n_out = self._L.rsrl_hip_n_outputs(self._h)      # weight columns: A, or 1 for TD / TDLambda
        self.F = self._L.rsrl_hip_n_features(self._h)
        self.n_weight_rows = self._L.rsrl_hip_n_weight_rows(self._h)      # rows of the weight matrix: F, or NAC's 3 F / GIBBS_NAC's (A + 1) F (SCB::n_features)
        self._q_rows = self.A if algo == GIBBS_NAC else self.n_out          # (q_evaluate's array shape: GIBBS_NAC's critic has one weight column and a value per action)
        self.n_policy_out = self._L.rsrl_hip_n_policy_outputs(self._h)      # columns of the policy's own weights: A (Gibbs), 2 (BETA, GAUSSIAN), 0 (the policy reads Q)
        self._policy_cols = self.n_policy_out or self.A                     # (the accessors' array shape; an agent without policy weights is refused by the library)
        self._td_cols = 1 if algo in (GTD2, TDC) else self.A                # (get/set_td_weights' array shape: GreedyGQ's fa_td has A columns)
        self.continuous = domain == CONTINUOUS_MOUNTAIN_CAR                 # actions are f32 values (the *_f32 entry points), not int32 indices
        self.shared = weight_mode == W_SHARED

    # ---- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._L.rsrl_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        _abi.check(self._L.rsrl_hip_sync(self._h))

    # ---- spaces
    def state_bounds(self):
        lo, hi = (C.c_double * self.D)(), (C.c_double * self.D)()
        _abi.check(self._L.rsrl_hip_state_bounds(self._h, lo, hi))
        return np.array(lo[:]), np.array(hi[:])

    def action_bounds(self):
        """action_space() bounds of a continuous domain -> (lo, hi); RsrlHipError on the domains whose actions are indices"""
        lo, hi = C.c_double(), C.c_double()
        _abi.check(self._L.rsrl_hip_action_bounds(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def _act(self):
        """(dtype, entry-point suffix) of the ctx's actions"""
        return (np.float32, "_f32") if self.continuous else (np.int32, "")

    # ---- env state
    def reset(self):
        _abi.check(self._L.rsrl_hip_reset(self._h))

    @property
    def states(self):
        out = np.empty((self.D, self.N), dtype=np.float32)
        _abi.check(self._L.rsrl_hip_get_states(self._h, _p(out)))
        return out

    @states.setter
    def states(self, v):
        _abi.check(self._L.rsrl_hip_set_states(self._h, _p(_in(v, np.float32, (self.D, self.N)))))

    def get_hidden_states(self):
        """HIVTreatment's hidden states [T1, T1*, T2, T2*, V, E], f64 (6, N); RsrlHipError on the other domains"""
        out = np.empty((6, self.N), dtype=np.float64)
        _abi.check(self._L.rsrl_hip_get_hidden_states(self._h, _p(out)))
        return out

    def set_hidden_states(self, y):
        """set HIVTreatment's hidden states, f64 (6, N); the observations (`states`) follow"""
        _abi.check(self._L.rsrl_hip_set_hidden_states(self._h, _p(_in(y, np.float64, (6, self.N)))))

    @property
    def actions(self):
        """the learners' pending actions (N,): int32 indices, or f32 values on a continuous domain"""
        dt, sfx = self._act()
        out = np.empty(self.N, dtype=dt)
        _abi.check(getattr(self._L, "rsrl_hip_get_actions" + sfx)(self._h, _p(out)))
        return out

    @actions.setter
    def actions(self, v):
        dt, sfx = self._act()
        _abi.check(getattr(self._L, "rsrl_hip_set_actions" + sfx)(self._h, _p(_in(v, dt, (self.N,)))))

    @property
    def episode_steps(self):
        """steps every learner's current episode has taken (ABI 8)"""
        out = np.empty(self.N, dtype=np.uint32)
        _abi.check(self._L.rsrl_hip_get_episode_steps(self._h, _p(out)))
        return out

    @episode_steps.setter
    def episode_steps(self, v):
        _abi.check(self._L.rsrl_hip_set_episode_steps(self._h, _p(_in(v, np.uint32, (self.N,)))))

    @property
    def episode_record(self):
        """GRADIENT_MC's (LSTD's, LSTD_LAMBDA's) open episodes -> (states (cap, D, N), rewards (cap, N)), cap = max_episode_steps: learner i's record is rows
        0 .. episode_steps[i]-1 of its column (row k: transition k's `from` and reward), NaN past that; RsrlHipError on the other agents"""
        cap = int(self.cfg.max_episode_steps)
        s, r = np.empty((cap, self.D, self.N), dtype=np.float32), np.empty((cap, self.N), dtype=np.float32)
        _abi.check(self._L.rsrl_hip_get_episode_record(self._h, _p(s), _p(r)))
        return s, r

    @episode_record.setter
    def episode_record(self, v):
        cap = int(self.cfg.max_episode_steps)
        s, r = v
        _abi.check(self._L.rsrl_hip_set_episode_record(self._h, _p(_in(s, np.float32, (cap, self.D, self.N))), _p(_in(r, np.float32, (cap, self.N)))))

    @property
    def q_carry(self):
        """Q(s,.) as the register-family loops carry it from launch to launch, (A, N) -- None while nothing is carried (ABI 8)"""
        out = np.empty((self.A, self.N), dtype=np.float32)
        valid = C.c_int32(0)
        _abi.check(self._L.rsrl_hip_get_q_carry(self._h, _p(out), C.byref(valid)))
        return out if valid.value else None

    @q_carry.setter
    def q_carry(self, v):
        _abi.check(self._L.rsrl_hip_set_q_carry(self._h, _p(_in(v, np.float32, (self.A, self.N)))))

    def domain_step(self, actions=None):
        """Domain::transition for every env -> (from, next, reward, terminal)"""
        frm = np.empty((self.D, self.N), dtype=np.float32)
        nxt = np.empty((self.D, self.N), dtype=np.float32)
        rew = np.empty(self.N, dtype=np.float32)
        term = np.empty(self.N, dtype=np.uint8)
        dt, sfx = self._act()
        _abi.check(getattr(self._L, "rsrl_hip_domain_step" + sfx)(self._h, _p(_in(actions, dt, (self.N,))), _p(frm), _p(nxt), _p(rew), _p(term)))
        return frm, nxt, rew, term

    def domain_reset(self, mask=None):
        _abi.check(self._L.rsrl_hip_domain_reset(self._h, _p(_in(mask, np.uint8, (self.N,)))))

    # ---- Q function
    def _batch(self, states):
        states = _in(states, np.float32)
        if states.ndim != 2 or states.shape[0] != self.D:
            raise ValueError(f"states must be [D={self.D}][M]")
        return states, states.shape[1]

    def q_evaluate(self, states):
        states, M = self._batch(states)
        out = np.empty((self._q_rows, M), dtype=np.float32)
        _abi.check(self._L.rsrl_hip_q_evaluate(self._h, _p(states), M, _p(out)))
        return out

    def q_evaluate_f32(self, states, actions):
        """NAC's critic, Function<(S, A)>: Q(s_i, a_i) = <w_i, psi(s_i, a_i)> against learner i's w and columns -> (M,) f32"""
        states, M = self._batch(states)
        out = np.empty(M, dtype=np.float32)
        _abi.check(self._L.rsrl_hip_q_evaluate_f32(self._h, _p(states), _p(_in(actions, np.float32, (M,))), M, _p(out)))
        return out

    def nac_update(self, mask=None):
        """NAC::handle(()) for the learners of mask ((N,) uint8, None: every learner) -> Response.norm (N,) f32, 0 for a learner left out"""
        out = np.empty(self.N, dtype=np.float32)
        _abi.check(self._L.rsrl_hip_nac_update(self._h, None if mask is None else _p(_in(mask, np.uint8, (self.N,))), _p(out)))
        return out

    def q_find_max(self, states):
        states, M = self._batch(states)
        idx, val = np.empty(M, dtype=np.int32), np.empty(M, dtype=np.float32)
        _abi.check(self._L.rsrl_hip_q_find_max(self._h, _p(states), M, _p(idx), _p(val)))
        return idx, val

    def q_find_min(self, states):
        """Enumerable::find_min (core.rs:86-94): (index, value), ties -> last index"""
        states, M = self._batch(states)
        idx, val = np.empty(M, dtype=np.int32), np.empty(M, dtype=np.float32)
        _abi.check(self._L.rsrl_hip_q_find_min(self._h, _p(states), M, _p(idx), _p(val)))
        return idx, val

    def q_expected_value(self, states, probs):
        """Enumerable::expected_value (core.rs:107-116): sum_a Q(s, a) * probs[a]; probs (A, M)"""
        states, M = self._batch(states)
        out = np.empty(M, dtype=np.float32)
        _abi.check(self._L.rsrl_hip_q_expected_value(self._h, _p(states), M, _p(_in(probs, np.float32, (self.A, M))), _p(out)))
        return out

    def project(self, states):
        states, M = self._batch(states)
        out = np.empty((self.F, M), dtype=np.float32)
        _abi.check(self._L.rsrl_hip_project(self._h, _p(states), M, _p(out)))
        return out

    def tile_indices(self, states):
        states, M = self._batch(states)
        out = np.empty((self.cfg.n_tilings, M), dtype=np.int32)
        _abi.check(self._L.rsrl_hip_tile_indices(self._h, _p(states), M, _p(out)))
        return out

    # ---- agent / policy
    def handle(self, from_states, actions, rewards, to_states, terminal):
        from_states, M = self._batch(from_states)
        to_states, _ = self._batch(to_states)
        td = np.empty(M, dtype=np.float32)
        dt, sfx = self._act()
        _abi.check(getattr(self._L, "rsrl_hip_handle" + sfx)(self._h, _p(from_states), _p(_in(actions, dt, (M,))),
                                                             _p(_in(rewards, np.float32, (M,))), _p(to_states),
                                                             _p(_in(terminal, np.uint8, (M,))), M, _p(td)))
        return td

    def handle_transitions(self, from_states, rewards, to_states, terminal, lengths, td=False, actions=None, T=None):
        """Handler<&Batch>::handle of LSTD / LSTD_LAMBDA for every learner: from_states / to_states (T, D, N), rewards (T, N), terminal (T, N) uint8,
        lengths (N,) -- learner i's batch is rows 0 .. lengths[i]-1 of its column (0: no call, the learner keeps its bytes); actions are not read.
        td=True: also the diagnostic r + gamma V(s') - V(s) at each handled row, (T, N) (NaN where nothing was handled).  One batch-step.  Arrays
        may be raw device pointers (int): then T is given, and `td` may be the device pointer the diagnostic is written to"""
        T = int(np.shape(rewards)[0]) if T is None else int(T)
        out = td if isinstance(td, int) and not isinstance(td, bool) else (np.full((T, self.N), np.nan, dtype=np.float32) if td else None)
        _abi.check(self._L.rsrl_hip_handle_transitions(self._h, T, _p(_in(from_states, np.float32, (T, self.D, self.N))), _p(_in(actions, np.int32, (T, self.N))),
                                                       _p(_in(rewards, np.float32, (T, self.N))), _p(_in(to_states, np.float32, (T, self.D, self.N))),
                                                       _p(_in(terminal, np.uint8, (T, self.N))), _p(_in(lengths, np.uint32, (self.N,))), _p(out)))
        return out

    def handle_batch(self, states, actions=None, rewards=None, lengths=None, returns=False, T=None):
        """Handler<&Batch>::handle of REINFORCE / BASELINE_REINFORCE for every learner: states (T, D, N), actions / rewards (T, N), lengths (N,) --
        learner i's batch is rows 0 .. lengths[i]-1 of its column.  returns=True: also the running return g at each handled transition, (T, N)
        (NaN where nothing was handled).  One batch-step, as handle.
        GRADIENT_MC: Handler<&Trajectory>::handle -- row k is transition k's `from` and reward, visited last to first; actions may be None (they
        are not read), and the returns are the backward sums.  Arrays may be raw device pointers (int): then T is given, and `returns` may be the
        device pointer the returns are written to"""
        if rewards is None or lengths is None:
            raise ValueError("handle_batch needs rewards and lengths")
        T = int(np.shape(rewards)[0]) if T is None else int(T)
        ret = returns if isinstance(returns, int) and not isinstance(returns, bool) else (np.full((T, self.N), np.nan, dtype=np.float32) if returns else None)
        _abi.check(self._L.rsrl_hip_handle_batch(self._h, T, _p(_in(states, np.float32, (T, self.D, self.N))), _p(_in(actions, np.int32, (T, self.N))),
                                                 _p(_in(rewards, np.float32, (T, self.N))), _p(_in(lengths, np.uint32, (self.N,))), _p(ret)))
        return ret

    def policy_sample(self, states=None):
        """Policy::sample.  states = None: the ctx's OWN envs (env.emit().state()) -- the driver loop's behaviour sample of the current batch-step
        (what rsrl_hip_train draws); the actions also become the ctx's pending ones"""
        dt, sfx = self._act()
        sample = getattr(self._L, "rsrl_hip_policy_sample" + sfx)
        if states is None:
            out = np.empty(self.N, dtype=dt)
            _abi.check(sample(self._h, None, self.N, _p(out)))
            return out
        states, M = self._batch(states)
        out = np.empty(M, dtype=dt)
        _abi.check(sample(self._h, _p(states), M, _p(out)))
        return out

    def policy_mode(self, states):
        dt, sfx = self._act()
        states, M = self._batch(states)
        out = np.empty(M, dtype=dt)
        _abi.check(getattr(self._L, "rsrl_hip_policy_mode" + sfx)(self._h, _p(states), M, _p(out)))
        return out

    def policy_params(self, states):
        """BETA's pub compute_alpha / compute_beta -> (alpha (M,), beta (M,)), GAUSSIAN's compute_mean / compute_stddev -> (mu (M,), sd (M,)):
        state i against learner i's columns"""
        states, M = self._batch(states)
        a, b = np.empty(M, dtype=np.float32), np.empty(M, dtype=np.float32)
        _abi.check(self._L.rsrl_hip_policy_params(self._h, _p(states), M, _p(a), _p(b)))
        return a, b

    def policy_pdf(self, states, actions):
        """BETA's Function<(S, A)>: the density of actions (M,) f32, each clamped to [2^-24, 1 - 2^-24]; GAUSSIAN's: of the actions as given"""
        states, M = self._batch(states)
        out = np.empty(M, dtype=np.float32)
        _abi.check(self._L.rsrl_hip_policy_pdf(self._h, _p(states), _p(_in(actions, np.float32, (M,))), M, _p(out)))
        return out

    def policy_probs(self, states):
        states, M = self._batch(states)
        out = np.empty((self.A, M), dtype=np.float32)
        _abi.check(self._L.rsrl_hip_policy_probs(self._h, _p(states), M, _p(out)))
        return out

    def policy_prob(self, states, actions):
        """Function<(S, A)> of the policy: P(a | s) (Softmax: the raw Q(s, a), softmax.rs:84-92)"""
        states, M = self._batch(states)
        out = np.empty(M, dtype=np.float32)
        _abi.check(self._L.rsrl_hip_policy_prob(self._h, _p(states), _p(_in(actions, np.int32, (M,))), M, _p(out)))
        return out

    def set_epsilon(self, eps):
        _abi.check(self._L.rsrl_hip_set_epsilon(self._h, float(eps)))

    @property
    def epsilons(self):
        """every learner's current EpsilonGreedy.epsilon (N,): its own field under `epsilon_decay`, else N copies of the ctx's"""
        out = np.empty(self.N, dtype=np.float32)
        _abi.check(self._L.rsrl_hip_get_epsilons(self._h, _p(out)))
        return out

    # ---- Parameterised
    def get_weights(self, env_index=0):
        out = np.empty((self.n_weight_rows, self.n_out), dtype=np.float32)
        _abi.check(self._L.rsrl_hip_get_weights(self._h, int(env_index), _p(out)))
        return out

    def set_weights(self, w, env_index=0):
        _abi.check(self._L.rsrl_hip_set_weights(self._h, int(env_index), _p(_in(w, np.float32, (self.n_weight_rows, self.n_out)))))

    def get_traces(self, env_index=0):
        out = np.empty((self.F, self.n_out), dtype=np.float32)
        _abi.check(self._L.rsrl_hip_get_traces(self._h, int(env_index), _p(out)))
        return out

    def set_traces(self, z, env_index=0):
        _abi.check(self._L.rsrl_hip_set_traces(self._h, int(env_index), _p(_in(z, np.float32, (self.F, self.n_out)))))

    def get_td_weights(self, env_index=0):
        """GreedyGQ.fa_td's weights of one learner (greedy_gq.rs:52), (F, A); GTD2.fa_w's / TDC.td_est's second weight column, (F, 1)"""
        out = np.empty((self.F, self._td_cols), dtype=np.float32)
        _abi.check(self._L.rsrl_hip_get_td_weights(self._h, int(env_index), _p(out)))
        return out

    def set_td_weights(self, v, env_index=0):
        _abi.check(self._L.rsrl_hip_set_td_weights(self._h, int(env_index), _p(_in(v, np.float32, (self.F, self._td_cols)))))

    def get_policy_weights(self, env_index=0):
        """ActorCritic.policy's weights theta of one learner (the Gibbs actor, ac.rs:61), f32 (F, A) -- also for TD_ACTOR_CRITIC, whose
        get_weights is V's (F, 1) -- and BETA's two columns (F, 2), alpha's then beta's; RsrlHipError on the other agents"""
        out = np.empty((self.F, self._policy_cols), dtype=np.float32)
        _abi.check(self._L.rsrl_hip_get_policy_weights(self._h, int(env_index), _p(out)))
        return out

    def set_policy_weights(self, theta, env_index=0):
        _abi.check(self._L.rsrl_hip_set_policy_weights(self._h, int(env_index), _p(_in(theta, np.float32, (self.F, self._policy_cols)))))

    def get_behaviour_weights(self, env_index=0):
        """REINFORCE's behaviour snapshot theta_b of one learner: its policy weights when the open episode began, f32 (F, A)"""
        out = np.empty((self.F, self.A), dtype=np.float32)
        _abi.check(self._L.rsrl_hip_get_behaviour_weights(self._h, int(env_index), _p(out)))
        return out

    def set_behaviour_weights(self, theta_b, env_index=0):
        _abi.check(self._L.rsrl_hip_set_behaviour_weights(self._h, int(env_index), _p(_in(theta_b, np.float32, (self.F, self.A)))))

    @property
    def return_carry(self):
        """REINFORCE's running return g of every learner's open episode, f32 (N,)"""
        out = np.empty(self.N, dtype=np.float32)
        _abi.check(self._L.rsrl_hip_get_return_carry(self._h, _p(out)))
        return out

    @return_carry.setter
    def return_carry(self, g):
        _abi.check(self._L.rsrl_hip_set_return_carry(self._h, _p(_in(g, np.float32, (self.N,)))))

    def get_lstd_state(self, env_index=0):
        """RecursiveLSTD / iLSTD / the iLSTD ActorCritic: one learner's exact f64 state -> (theta (F,), the matrix (F, F): C / A, mu (F,) for iLSTD else None)"""
        theta, mat = np.empty(self.F, dtype=np.float64), np.empty((self.F, self.F), dtype=np.float64)
        mu = np.empty(self.F, dtype=np.float64) if self.cfg.algo in (ILSTD, ILSTD_ACTOR_CRITIC) else None
        _abi.check(self._L.rsrl_hip_get_lstd_state(self._h, int(env_index), _p(theta), _p(mat), _p(mu)))
        return theta, mat, mu

    def get_lstd_batch_state(self, env_index=0):
        """LSTD / LSTDLambda / LambdaLSPE: one learner's exact f64 state -> (theta (F,), A (F, F), b (F,), z (F,) for LSTDLambda, (delta, rows, 0 ...)
        for LambdaLSPE, else None, singular_solves)"""
        theta, A, b = np.empty(self.F, dtype=np.float64), np.empty((self.F, self.F), dtype=np.float64), np.empty(self.F, dtype=np.float64)
        z = np.empty(self.F, dtype=np.float64) if self.cfg.algo in (LSTD_LAMBDA, LAMBDA_LSPE) else None
        sing = np.zeros(1, dtype=np.uint32)
        _abi.check(self._L.rsrl_hip_get_lstd_batch_state(self._h, int(env_index), _p(theta), _p(A), _p(b), _p(z), _p(sing)))
        return theta, A, b, z, int(sing[0])

    def set_lstd_batch_state(self, theta, A, b, z=None, singular_solves=0, env_index=0):
        """LSTD / LSTDLambda / LambdaLSPE: install one learner's f64 state exactly (z: LSTDLambda's trace, LambdaLSPE's z[0] = delta and z[1] = rows --
        an integer in 0 .. F; None leaves it as it is)"""
        sing = np.array([singular_solves], dtype=np.uint32)
        _abi.check(self._L.rsrl_hip_set_lstd_batch_state(self._h, int(env_index), _p(_in(theta, np.float64, (self.F,))), _p(_in(A, np.float64, (self.F, self.F))),
                                                         _p(_in(b, np.float64, (self.F,))), _p(None if z is None else _in(z, np.float64, (self.F,))), _p(sing)))

    def lstd_solve(self):
        """LSTD / LSTDLambda: the agents' public solve() for every learner -- theta <- A.solve(b) in the library's fixed operation order; an abandoned
        solve (no pivot above 0) keeps theta and counts in singular_solves.  LambdaLSPE: its solve() as handle ends with it (deferred below F rows; the
        relaxed step; A, b, delta and rows zeroed on success)"""
        _abi.check(self._L.rsrl_hip_lstd_solve(self._h))

    def set_lstd_state(self, theta, mat, mu=None, env_index=0):
        """RecursiveLSTD / iLSTD: install one learner's f64 state exactly (mu: iLSTD only; None leaves it as it is)"""
        _abi.check(self._L.rsrl_hip_set_lstd_state(self._h, int(env_index), _p(_in(theta, np.float64, (self.F,))), _p(_in(mat, np.float64, (self.F, self.F))),
                                                   _p(None if mu is None else _in(mu, np.float64, (self.F,)))))

    def save_weights(self, path):
        _abi.check(self._L.rsrl_hip_save_weights(self._h, str(path).encode()))

    def load_weights(self, path):
        _abi.check(self._L.rsrl_hip_load_weights(self._h, str(path).encode()))

    def set_weights_all(self, w):
        _abi.check(self._L.rsrl_hip_set_weights_all(self._h, _p(_in(w, np.float32, (self.n_weight_rows, self.n_out)))))

    # ---- driver loop
    def train(self, n_steps, want_stats=True):
        st = _abi.Stats()
        _abi.check(self._L.rsrl_hip_train(self._h, int(n_steps), C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    @property
    def step_count(self):
        return int(self._L.rsrl_hip_step_count(self._h))

    @property
    def pending_steps(self):
        """batch-steps accepted by train() but not enqueued yet (launch coalescing on a ctx-owned stream)"""
        return int(self._L.rsrl_hip_pending_steps(self._h))

    def _rollout_rows(self, step_limit):
        """rows of a rollout's state output: step_limit, or -- step_limit 0 / None = Domain::rollout(.., None), bounded by the ctx's
        max_episode_steps -- max_episode_steps + 1"""
        return int(step_limit) if step_limit else int(self.cfg.max_episode_steps) + 1

    def rollout_greedy(self, step_limit):
        n_states = np.empty(self.N, dtype=np.uint32)
        tot = np.empty(self.N, dtype=np.float32)
        _abi.check(self._L.rsrl_hip_rollout_greedy(self._h, int(step_limit or 0), _p(n_states), _p(tot)))
        return n_states, tot

    def rollout_trajectory(self, step_limit, M=None):
        """Domain::rollout with the Trajectory (lib.rs:334-409) of learners 0..M-1 -> dict(n_states, total_reward, states
        (step_limit, D, M), actions / rewards (step_limit - 1, M), terminal (M,)); rows past n_states are zero"""
        M = self.N if M is None else int(M)
        L = self._rollout_rows(step_limit)
        out = dict(n_states=np.empty(M, dtype=np.uint32), total_reward=np.empty(M, dtype=np.float32),
                   states=np.zeros((L, self.D, M), dtype=np.float32), actions=np.zeros((max(L - 1, 0), M), dtype=np.int32),
                   rewards=np.zeros((max(L - 1, 0), M), dtype=np.float32), terminal=np.empty(M, dtype=np.uint8))
        _abi.check(self._L.rsrl_hip_rollout_trajectory(self._h, int(step_limit or 0), M, _p(out["n_states"]), _p(out["total_reward"]), _p(out["states"]),
                                                       _p(out["actions"]) if L > 1 else None, _p(out["rewards"]) if L > 1 else None,
                                                       _p(out["terminal"])))
        return out

    def rollout_policy(self, policy, step_limit, M=None, epsilon=0.1, tau=1.0):
        """Domain::rollout with the closure s -> policy.sample(rng, s) for ANY of the four policies over the ctx's Q function
        (lib.rs:448-479 takes any FnMut(&S) -> A) -> the same dict as rollout_trajectory"""
        M = self.N if M is None else int(M)
        L = self._rollout_rows(step_limit)
        out = dict(n_states=np.empty(M, dtype=np.uint32), total_reward=np.empty(M, dtype=np.float32),
                   states=np.zeros((L, self.D, M), dtype=np.float32), actions=np.zeros((max(L - 1, 0), M), dtype=np.int32),
                   rewards=np.zeros((max(L - 1, 0), M), dtype=np.float32), terminal=np.empty(M, dtype=np.uint8))
        _abi.check(self._L.rsrl_hip_rollout_policy(self._h, int(policy), float(epsilon), float(tau), int(step_limit or 0), M, _p(out["n_states"]),
                                                   _p(out["total_reward"]), _p(out["states"]), _p(out["actions"]) if L > 1 else None,
                                                   _p(out["rewards"]) if L > 1 else None, _p(out["terminal"])))
        return out

    def checksum(self):
        """(weights(+traces), env state) 64-bit checksums computed on the device"""
        out = (C.c_uint64 * 2)()
        _abi.check(self._L.rsrl_hip_checksum(self._h, out))
        return int(out[0]), int(out[1])

    def fx_saturations(self):
        """terms the shared-W fixed-point sums had to clamp so far on this device (0 in a healthy run)"""
        n = C.c_uint64()
        _abi.check(self._L.rsrl_hip_fx_saturations(self._h, C.byref(n)))
        return int(n.value)

    # ---- multi-GPU (shared weights): RCCL communicator, one process per GPU
    @staticmethod
    def comm_unique_id():
        """ncclUniqueId (128 bytes) -- call on rank 0 and distribute through the control plane"""
        buf = (C.c_uint8 * 128)()
        _abi.check(_abi.lib().rsrl_hip_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, id_bytes, world_size, rank):
        buf = (C.c_uint8 * 128)(*id_bytes)
        _abi.check(self._L.rsrl_hip_comm_init(self._h, buf, int(world_size), int(rank)))

    # ---- multi-GPU (shared weights): one-hop peer-write exchange (exchange=EXCHANGE_PEER)
    def peer_export(self, world_size):
        """this rank's receive buffer described in a 128-byte handle -- all-gather the handles through the control plane"""
        buf = (C.c_uint8 * PEER_HANDLE_BYTES)()
        _abi.check(self._L.rsrl_hip_peer_export(self._h, int(world_size), buf))
        return bytes(buf)

    def peer_connect(self, handles, rank):
        """handles: the world_size handles in rank order"""
        blob = b"".join(handles)
        buf = (C.c_uint8 * len(blob))(*blob)
        _abi.check(self._L.rsrl_hip_peer_connect(self._h, buf, len(handles), int(rank)))

    @staticmethod
    def group_create(ctxs):
        """all ranks in this process (rank = position in `ctxs`): attach the exchange the ctxs were configured with"""
        arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
        _abi.check(_abi.lib().rsrl_hip_group_create(arr, len(ctxs)))

    @staticmethod
    def group_train(ctxs, n_steps):
        """one thread stepping every rank of a group made by group_create (required for RCCL groups of more than one rank:
        each batch-step's all-reduces are issued for all ranks inside one ncclGroupStart / End)"""
        arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
        _abi.check(_abi.lib().rsrl_hip_group_train(arr, len(ctxs), int(n_steps)))

    def comm_info(self):
        """(world_size, rank, exchange) as the attached exchange reports them; exchange -1 = none"""
        w, r, e = C.c_int(), C.c_int(), C.c_int()
        _abi.check(self._L.rsrl_hip_comm_info(self._h, C.byref(w), C.byref(r), C.byref(e)))
        return w.value, r.value, e.value

    # ---- measurement
    def timing_enable(self, on=True):
        _abi.check(self._L.rsrl_hip_timing_enable(self._h, int(bool(on))))

    def timing_read(self):
        ms, n, name = C.c_double(), C.c_uint64(), C.c_char_p()
        _abi.check(self._L.rsrl_hip_timing_read(self._h, C.byref(ms), C.byref(n), C.byref(name)))
        return ms.value, int(n.value), (name.value or b"").decode()
