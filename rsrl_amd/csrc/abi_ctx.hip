// abi_ctx.hip -- the ctx's life cycle and plain state: create / destroy (the constructors of examples/q_learning.rs:19-32), configuration checks,
// the env state accessors, reset, the timing hooks.
#include "ctx.hpp"

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_last_error = buf;
    // the HIP runtime keeps the last failure of ANY call of this thread until somebody asks for it: asked for here WHEN THE FAILURE REPORTED IS A HIP ONE, so
    // that it is not found again by the next launch check (KCHECK) of a healthy ctx.  A pure argument / state error (EINVAL, ESTATE) leaves it alone: a launch
    // error not yet checked must not be lost behind an unrelated report; rsrl_hip_destroy and the clean-up paths clear it themselves.
    if (code == RSRL_HIP_EHIP || code == RSRL_HIP_ENOMEM) (void)hipGetLastError();
    return code;
}

// every environment switch the library reads: once, when the ctx is created -- except RSRL_NO_COALESCE, which rsrl_hip_train asks
// at every call (bench.py turns it on and off around calls of a live ctx)
static Switches read_switches() {
    Switches sw;
    sw.no_graph = getenv("RSRL_NO_GRAPH") != nullptr;
    sw.no_persist = getenv("RSRL_NO_PERSIST") != nullptr;
    sw.no_trait_defer = getenv("RSRL_NO_TRAIT_DEFER") != nullptr;
    sw.k1_feature_major = getenv("RSRL_K1_FEATURE_MAJOR") != nullptr;
    if (const char* e = getenv("RSRL_K1_QUAD")) sw.k1_quad = e[0] != '0' ? 1 : 0;
    if (const char* e = getenv("RSRL_SPARSE_CHUNK")) { const int v = atoi(e); sw.sparse_chunk = v > 0 && v < 16 ? 16 : v; }
    if (const char* e = getenv("RSRL_PEER_TIMEOUT_MS")) sw.peer_timeout_ms = atol(e);
    if (const char* e = getenv("RSRL_WAVE_PK")) sw.no_wave_pk = e[0] == '0';
    if (const char* e = getenv("RSRL_REG_PRODUCER")) sw.no_reg_producer = e[0] == '0';
    if (const char* e = getenv("RSRL_TABLE_MEM")) sw.table_mem = e[0] != '0' ? 1 : 0;
    return sw;
}
bool no_coalesce_switch() { return getenv("RSRL_NO_COALESCE") != nullptr; }

// the kernel family of a validated configuration (ctx.hpp AgentFamily), first match in the order of the enum.  w_elems: the ctx's weight count.
// A decision, so a function; what a family IS stands in ctx.hpp's kFamily, the other place (with launch_agent) a new family is entered
static AgentFamily classify(const rsrl_hip_config& cfg, size_t w_elems) {
    using F = AgentFamily;
    const bool fourier = cfg.basis == RSRL_FOURIER, tile = cfg.basis == RSRL_TILE_CODING;
    const bool wave = is_wave(cfg), reg = is_reg_fourier(cfg);
    const int al = cfg.algo;
    if (cfg.domain == RSRL_HIV_TREATMENT) return F::Hiv;
    if (cfg.domain == RSRL_CLIFF_WALK) return F::CliffTable;
    if (is_ac(al)) return F::AcReg;                         // (before the one-step agents: carries_q is false, no trait fast path)
    if (is_tdac(al)) return F::TdAcReg;                     // (before the prediction agents: W is V's one column, but the policy is the actor's)
    if (is_reinforce(al)) return F::ReinforceReg;
    if (is_lstd(al)) return F::LstdReg;
    if (is_tdac_lstd(al)) return cfg.domain == RSRL_CONTINUOUS_MOUNTAIN_CAR ? F::TdAcBetaReg : F::TdAcLstdReg;
    if (is_gmc(al)) return F::GmcReg;
    if (is_lstd_batch(al)) return F::LstdBatchReg;
    if (is_nac(al)) return cfg.policy == RSRL_GAUSSIAN ? F::NacGaussReg : F::NacBetaReg;
    if (is_gibbs_nac(al)) return F::GibbsNacReg;            // (before the prediction agents: W is one column, but the policy is the actor's)
    if (is_gtd(al)) return F::GtdReg;
    if (is_cacla(al)) return F::CaclaGaussReg;
    if (is_tdac_cont(al)) return cfg.policy == RSRL_GAUSSIAN ? F::TdAcGaussReg : F::TdAcBetaTdReg;
    if (cfg.weight_mode == RSRL_W_SHARED) return fourier ? F::SharedDense : (is_sparse_lambda(cfg) ? F::SharedSparseLambda : F::SharedTile);
    if (wave && is_wave_aux_algo(al)) return F::WaveAux;
    if (is_pred(al)) return tile ? F::TdTile : (reg ? F::TdReg : F::TdGeneric);
    if (al == RSRL_Q_SIGMA) return wave ? F::WaveQSigma : (reg ? F::QSigmaReg : F::QSigmaGeneric);
    if (al == RSRL_GREEDY_GQ) return reg ? F::GqReg : F::GqGeneric;
    if (is_lambda(al)) return tile ? F::LambdaTile : (wave ? F::WaveLambda : (reg ? F::LambdaReg : F::LambdaGeneric));
    if (wave) return F::WaveControl;
    // single-step streaming kernel: needs the whole W addressable through one 32-bit buffer descriptor
    if (reg) return cfg.steps_per_launch == 1 && (uint64_t)w_elems * 4ull < (1ull << 32) ? F::RegStep : F::RegFused;
    return F::Generic;
}
// what rsrl_hip_timing_read names after a driver-loop launch of the family (the persistent kernel and the trait-granular kernels name themselves)
static const char* train_kernel_name(const rsrl_hip_ctx* c) {
    // (the two families whose kernel the configuration refines; every other name is the family's row of kFamily)
    if (c->family == AgentFamily::WaveControl && c->cfg.weight_dtype == RSRL_W_BF16 && !c->sw.no_wave_pk) return "k_train_wave_pk";
    if (c->family == AgentFamily::RegStep && c->w_ls != 1) return c->k1_quad ? "k_step_reg_q4" : "k_step_reg_lm";
    if (c->family == AgentFamily::LstdBatchReg && c->cfg.algo == RSRL_LAMBDA_LSPE) return "k_train_lspe";
    if (c->family == AgentFamily::CliffTable && c->sw.table_mem == 1) return "k_table_train_mem";      // (by launch depth otherwise: launch_agent names it)
    return family_row(c).kernel;
}
// one statistics slot per thread block of the family's driver-loop kernel
static size_t stat_slots(Slots geometry, int64_t N, int F) {
    switch (geometry) {
    case Slots::Block: return grid_for(N);
    case Slots::Block64: return (size_t)((N + 63) / 64);
    case Slots::WaveBlock: return wave_grid_for(N);
    case Slots::Learner: return (size_t)N;
    case Slots::LstdGroup: return (size_t)((N * lstd_group_lanes(F) + kBlock - 1) / kBlock);      // k_train_lstd: G lanes per learner
    }
    return 0;
}
// THE owner of the device buffers create_impl allocates: allocated, zero-filled on the ctx's stream if asked, and recorded for rsrl_hip_destroy -- the
// MEMBER, not its value: rsrl_hip_load_weights switches W, Z, sp_keys and sp_vals to shadow copies and frees the old ones itself
template <class T>
static int ctx_alloc(rsrl_hip_ctx* c, T** member, size_t bytes, bool zero = false) {
    if (bytes == 0) { *member = nullptr; return RSRL_HIP_OK; }      // (a continuous ctx's [A][N] arrays: A = 0)
    HIP_TRY(hipMalloc((void**)member, bytes));
    c->owned.push_back((void**)member);
    if (zero) HIP_TRY(hipMemsetAsync(*member, 0, bytes, c->stream));
    return RSRL_HIP_OK;
}

RSRL_API_BEGIN

int rsrl_hip_abi_version(void) { return RSRL_HIP_ABI_VERSION; }
int rsrl_hip_device_count(void) {
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    return n;
}
const char* rsrl_hip_last_error(void) { return g_last_error.c_str(); }

int rsrl_hip_config_init(rsrl_hip_config* cfg) {
    if (!cfg) return fail(RSRL_HIP_EINVAL, "null cfg");
    memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->domain = RSRL_MOUNTAIN_CAR; cfg->basis = RSRL_FOURIER; cfg->order = 5;
    cfg->n_tilings = 8; cfg->tiles_per_dim = 8;
    cfg->algo = RSRL_QLEARNING; cfg->policy = RSRL_GREEDY;
    cfg->weight_mode = RSRL_W_PER_ENV; cfg->weight_dtype = RSRL_W_F32;
    cfg->n_envs = 1; cfg->seed = 0;
    cfg->gamma = 0.9; cfg->lr = 0.001; cfg->alpha = 1.0; cfg->epsilon = 0.1; cfg->tau = 1.0;
    cfg->max_episode_steps = 0; cfg->steps_per_launch = 0;
    cfg->trace = RSRL_TRACE_ACCUMULATE; cfg->lambda = 0.0; cfg->lr_td = 0.0;
    cfg->agent_policy = -1; cfg->agent_epsilon = 0.1; cfg->agent_tau = 1.0; cfg->exchange = RSRL_EXCHANGE_AUTO;
    cfg->sigma = 0.0; cfg->n_steps = 1;
    cfg->epsilon_decay = 1.0; cfg->epsilon_min = 0.0;
    return RSRL_HIP_OK;
}

int rsrl_hip_destroy(rsrl_hip_ctx* c) {
    if (!c) return RSRL_HIP_OK;
    // (a ctx whose creation failed on its device ordinal is torn down through here too: the failure of this call must not stay behind as the thread's
    //  last HIP error -- tests/fuzz_abi.py found it reported by the next ctx's first launch check)
    if (hipSetDevice(c->cfg.device) != hipSuccess) (void)hipGetLastError();
    if (c->tp.stage) (void)trait_flush(c);       // trait calls accepted but not launched: the caller's arrays are still written
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& ev : c->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (c->step_graph_exec) (void)hipGraphExecDestroy(c->step_graph_exec);
    if (c->step_graph) (void)hipGraphDestroy(c->step_graph);
    for (void** member : c->owned) if (*member) (void)hipFree(*member);      // everything create_impl allocated (ctx_alloc)
    // what has a lifetime of its own: the staging slots, the pinned statistics, the communicator, the peer exchange's and the persistent kernel's buffers
    // (abi_group.hip, ensure_persist_buffers)
    for (auto& s : c->scratch) if (s.p) (void)hipFree(s.p);
    if (c->h_stats) (void)hipHostFree(c->h_stats);
    if (c->comm) (void)ncclCommDestroy(c->comm);
    for (size_t r = 0; r < c->peer_ptrs.size(); ++r) if (c->peer_opened[r] && c->peer_ptrs[r]) (void)hipIpcCloseMemHandle(c->peer_ptrs[r]);
    if (c->peer_recv) (void)hipFree(c->peer_recv);
    if (c->d_peer_ptrs) (void)hipFree(c->d_peer_ptrs);
    if (c->px_A) (void)hipFree(c->px_A);
    if (c->px_B && c->px_B_owned) (void)hipFree(c->px_B);
    if (c->d_px_Bptrs) (void)hipFree(c->d_px_Bptrs);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    (void)hipGetLastError();                     // (whatever a release above may have failed with is not the next ctx's business)
    delete c;
    return RSRL_HIP_OK;
}

// The agents that exist only on the register-family Fourier orders with per-learner f32 weights (train_ac.hip, train_tdac.hip, train_reinforce.hip,
// train_lstd.hip, train_tdac_lstd.hip, train_gmc.hip, train_lstd_batch.hip, train_lspe.hip, train_gtd.hip): the policy is the agent's own -- the Gibbs actor / policy, or the prediction agents' Random behaviour -- and the
// critic shares it; iLSTD's n_updates travel as config.n_steps.  `storage`: register-family order, per-learner f32 weights, no epsilon schedule
static int check_reg_only(const rsrl_hip_config& cfg, const AlgoRow& a, bool storage) {
    if (!storage || cfg.policy != a.reg_policy || cfg.agent_policy != -1)
        return fail(RSRL_HIP_EINVAL, "%s supports per-learner f32 weights on the register-family Fourier orders (MountainCar 1-5, CartPole 1, Acrobot 1) "
                                     "with policy = %s%s, agent_policy = -1%s and no epsilon schedule (got domain %d, basis %d, order %d, weight mode %d, "
                                     "dtype %d, policy %d, agent_policy %d, epsilon_decay %g)",
                    a.name, a.reg_policy == RSRL_SOFTMAX ? "Softmax" : "Random", a.policy_words, a.shares_words,
                    cfg.domain, cfg.basis, cfg.order, cfg.weight_mode, cfg.weight_dtype, cfg.policy, cfg.agent_policy, cfg.epsilon_decay);
    if (a.n_updates && (cfg.n_steps < 1 || cfg.n_steps > 32))
        return fail(RSRL_HIP_EINVAL, "%s: n_steps (%sn_updates, the rounds of solve() per transition) must be in [1, 32], got %d", a.name, a.n_updates, cfg.n_steps);
    if (a.agent == Agent::GibbsNac && (cfg.n_steps < 1 || cfg.n_steps > 65536))
        return fail(RSRL_HIP_EINVAL, "%s: n_steps (the actor's period: NAC::handle(()) runs at every n_steps-th step of an episode, nac_softmax.rs) must be "
                                     "in [1, 65536], got %d", a.name, cfg.n_steps);
    // GradientMC, LSTD, LSTDLambda and LambdaLSPE keep every learner's open episode on the device, max_episode_steps rows of it
    if ((a.agent == Agent::Gmc || a.agent == Agent::LstdBatch) && cfg.max_episode_steps < 1)
        return fail(RSRL_HIP_EINVAL, "%s: max_episode_steps must be >= 1 -- the device records every learner's open episode, and an unbounded episode "
                                     "(max_episode_steps = 0) has no record size", a.name);
    if (cfg.algo == RSRL_LAMBDA_LSPE && !std::isfinite(cfg.alpha))
        return fail(RSRL_HIP_EINVAL, "%s: alpha (the relaxation theta <- (1 - alpha) theta + alpha x of solve(), lambda_lspe.rs:55-56) must be finite, got %g", a.name, cfg.alpha);
    return RSRL_HIP_OK;
}

// (state dimension, action count) of MountainCar, CartPole, Acrobot, HIVTreatment, ContinuousMountainCar (0: the action set is not enumerable), CliffWalk
static const int kDomainShape[6][2] = {{2, 3}, {4, 2}, {4, 3}, {6, 4}, {2, 0}, {2, 4}};

// ContinuousMountainCar and the continuous policies (cont_policy.hpp; train_tdac_beta.hip, train_nac.hip, train_cont.hip):
// the domain exists for them only and they for it, Beta under the iLSTD ActorCritic, NAC and the continuous TD ActorCritic, Gaussian under NAC, CACLA
// and the continuous TD ActorCritic -- and NAC, CACLA and the continuous TD ActorCritic for them only
static int check_continuous(const rsrl_hip_config& cfg, const AlgoRow& a, bool storage) {
    const bool nac = cfg.algo == RSRL_NAC, cacla = cfg.algo == RSRL_CACLA, tdac = cfg.algo == RSRL_CONTINUOUS_TD_ACTOR_CRITIC;
    const bool pair = (cfg.policy == RSRL_BETA && (cfg.algo == RSRL_ILSTD_ACTOR_CRITIC || nac || tdac)) || (cfg.policy == RSRL_GAUSSIAN && (nac || cacla || tdac));
    if (cfg.domain != RSRL_CONTINUOUS_MOUNTAIN_CAR || !pair || !storage || cfg.agent_policy != -1)
        return fail(RSRL_HIP_EINVAL, "ContinuousMountainCar (RSRL_CONTINUOUS_MOUNTAIN_CAR), the Beta policy (RSRL_BETA), the Gaussian policy (RSRL_GAUSSIAN), "
                                     "NAC (RSRL_NAC), CACLA (RSRL_CACLA) and the continuous TD ActorCritic (RSRL_CONTINUOUS_TD_ACTOR_CRITIC) support the iLSTD "
                                     "ActorCritic (RSRL_ILSTD_ACTOR_CRITIC) with policy = Beta, NAC and the continuous TD ActorCritic with policy = Beta or "
                                     "Gaussian and CACLA with policy = Gaussian on ContinuousMountainCar, Fourier orders 1-5, per-learner f32 "
                                     "weights, agent_policy = -1 and no epsilon schedule -- and nothing else (got domain %d, basis %d, order %d, algo %d, weight "
                                     "mode %d, dtype %d, policy %d, agent_policy %d, epsilon_decay %g)",
                    cfg.domain, cfg.basis, cfg.order, cfg.algo, cfg.weight_mode, cfg.weight_dtype, cfg.policy, cfg.agent_policy, cfg.epsilon_decay);
    if (nac) {
        if (cfg.n_steps < 1 || cfg.n_steps > 65536)
            return fail(RSRL_HIP_EINVAL, "%s: n_steps (the actor's period: NAC::handle(()) runs at every n_steps-th step of an episode, 100 in nac_beta.rs and nac.rs) must be "
                                         "in [1, 65536], got %d", a.name, cfg.n_steps);
        return RSRL_HIP_OK;
    }
    if (cacla || tdac) return RSRL_HIP_OK;      // (n_steps is not read)
    if (cfg.n_steps < 1 || cfg.n_steps > 32)
        return fail(RSRL_HIP_EINVAL, "%s: n_steps (%sn_updates, the rounds of solve() per transition) must be in [1, 32], got %d", a.name, a.n_updates, cfg.n_steps);
    return RSRL_HIP_OK;
}

// admission: every rule that needs no device (a refused configuration is EINVAL on any machine, with or without a GPU).  create_impl checks
// two more once the device is known: peer_timeout_ms, and the slice of a shared tile table with sparse traces.  The second section states
// which kernels exist, one block per agent group; the register-family-only agents (check_reg_only) and HIVTreatment are whole rules of their own.
static int check_config(const rsrl_hip_config& cfg) {
    // ---- field ranges
    if (cfg.domain < RSRL_MOUNTAIN_CAR || cfg.domain > RSRL_CLIFF_WALK) return fail(RSRL_HIP_EINVAL, "unknown domain %d", cfg.domain);
    const int D = kDomainShape[cfg.domain][0], A = kDomainShape[cfg.domain][1];
    if (cfg.n_envs < 1) return fail(RSRL_HIP_EINVAL, "n_envs must be >= 1");
    if (cfg.n_envs + cfg.env_offset > (int64_t)0xffffffffLL || cfg.env_offset < 0) return fail(RSRL_HIP_EINVAL, "global env ids must fit 32 bits");
    if (cfg.algo < 0 || cfg.algo > kLastAlgo || !kAlgo[cfg.algo].name) return fail(RSRL_HIP_EINVAL, "unknown algo %d", cfg.algo);
    if (cfg.policy < 0 || (cfg.policy > RSRL_BETA && cfg.policy != RSRL_GAUSSIAN)) return fail(RSRL_HIP_EINVAL, "unknown policy %d", cfg.policy);      // (5 is no policy)
    // Softmax::new panics for |tau| < 1e-7 (policies/softmax.rs:63-66)
    if (cfg.policy == RSRL_SOFTMAX && std::fabs(cfg.tau) < 1e-7) return fail(RSRL_HIP_EINVAL, "Tau parameter in Softmax must be non-zero.");
    // the reference admits any non-zero tau; the kernels evaluate the max-shifted form exp((q - max q) / tau), whose exponents are >= 0 for tau < 0
    if (cfg.policy == RSRL_SOFTMAX && cfg.tau < 0.0) return fail(RSRL_HIP_EINVAL, NEGATIVE_TAU_MSG, "tau", cfg.tau);
    if (cfg.weight_dtype != RSRL_W_F32 && cfg.weight_dtype != RSRL_W_BF16) return fail(RSRL_HIP_EINVAL, "unknown weight dtype %d", cfg.weight_dtype);
    if (cfg.agent_policy < -1 || cfg.agent_policy > RSRL_RANDOM) return fail(RSRL_HIP_EINVAL, "unknown agent policy %d", cfg.agent_policy);
    if (cfg.agent_policy == RSRL_SOFTMAX && std::fabs(cfg.agent_tau) < 1e-7) return fail(RSRL_HIP_EINVAL, "Tau parameter in Softmax must be non-zero.");
    if (cfg.agent_policy == RSRL_SOFTMAX && cfg.agent_tau < 0.0) return fail(RSRL_HIP_EINVAL, NEGATIVE_TAU_MSG, "agent_tau", cfg.agent_tau);
    if (cfg.agent_policy == RSRL_EPSILON_GREEDY && !(cfg.agent_epsilon >= 0.0 && cfg.agent_epsilon <= 1.0))
        return fail(RSRL_HIP_EINVAL, "agent_epsilon must be in [0,1]");
    if (cfg.exchange != RSRL_EXCHANGE_RCCL && cfg.exchange != RSRL_EXCHANGE_PEER && cfg.exchange != RSRL_EXCHANGE_AUTO) return fail(RSRL_HIP_EINVAL, "unknown exchange %d", cfg.exchange);
    const bool shared = cfg.weight_mode == RSRL_W_SHARED, per_env = cfg.weight_mode == RSRL_W_PER_ENV;
    if (cfg.basis == RSRL_FOURIER) {
        if (cfg.order < 1 || cfg.order > 7) return fail(RSRL_HIP_EINVAL, "Fourier order must be in [1, 7]");
    } else if (cfg.basis == RSRL_TILE_CODING) {
        if (cfg.tiles_per_dim < 1 || cfg.tiles_per_dim > 64) return fail(RSRL_HIP_EINVAL, "tiles_per_dim must be in [1, 64]");
        int64_t cells = 1; for (int i = 0; i < D; ++i) cells *= cfg.tiles_per_dim;
        if (cells > (int64_t)1 << 30 || cells * cfg.n_tilings > (int64_t)1 << 30) return fail(RSRL_HIP_EINVAL, "tile table too large");
        // (a shared table is gathered through one 32-bit buffer descriptor)
        if (shared && cells * cfg.n_tilings * A * 4 >= (int64_t)1 << 31) return fail(RSRL_HIP_EINVAL, "a shared tile table must be smaller than 2 GiB");
    } else if (cfg.basis != RSRL_TABLE) {      // (the table reads none of order, n_tilings, tiles_per_dim)
        return fail(RSRL_HIP_EINVAL, "unknown basis %d", cfg.basis);
    }
    if (cfg.algo == RSRL_TD_LAMBDA || is_lambda(cfg.algo)) {
        if (cfg.trace < 0 || cfg.trace > RSRL_TRACE_DUTCH) return fail(RSRL_HIP_EINVAL, "unknown trace rule %d", cfg.trace);
        if (!(cfg.lambda >= 0.0 && cfg.lambda <= 1.0)) return fail(RSRL_HIP_EINVAL, "lambda must be in [0, 1]");
    }
    if (cfg.algo == RSRL_Q_SIGMA) {
        if (!(cfg.sigma >= 0.0 && cfg.sigma <= 1.0)) return fail(RSRL_HIP_EINVAL, "sigma must be in [0, 1]");
        if (cfg.n_steps < 1 || cfg.n_steps > 32) return fail(RSRL_HIP_EINVAL, "n_steps must be in [1, 32]");
    }
    if ((cfg.algo == RSRL_GREEDY_GQ || is_gtd(cfg.algo)) && !(cfg.lr_td >= 0.0)) return fail(RSRL_HIP_EINVAL, "lr_td must be >= 0");
    if (!(cfg.epsilon_decay > 0.0 && cfg.epsilon_decay <= 1.0)) return fail(RSRL_HIP_EINVAL, "epsilon_decay must be in (0, 1] (1 = no schedule)");
    if (!(cfg.epsilon_min >= 0.0 && cfg.epsilon_min <= 1.0)) return fail(RSRL_HIP_EINVAL, "epsilon_min must be in [0, 1]");

    // ---- which kernels exist
    const int al = cfg.algo;
    const bool tile = cfg.basis == RSRL_TILE_CODING, reg = is_reg_fourier(cfg), wave = is_wave(cfg);
    const bool f32 = cfg.weight_dtype == RSRL_W_F32, esched = cfg.epsilon_decay != 1.0;
    const bool one_step = kAlgo[al].agent == Agent::OneStep;
    // train_table.hip: CliffWalk exists for the tabular Q only and the table for it only -- a rule of its own, in front of every agent's: whatever else the
    // configuration names, the refusal names CliffWalk
    if (cfg.domain == RSRL_CLIFF_WALK || cfg.basis == RSRL_TABLE) {
        if (cfg.domain != RSRL_CLIFF_WALK || cfg.basis != RSRL_TABLE || !one_step || !per_env || !f32 || esched || cfg.policy > RSRL_RANDOM)
            return fail(RSRL_HIP_EINVAL, "CliffWalk (RSRL_CLIFF_WALK) and the tabular Q (RSRL_TABLE) support each other only, with QLearning, SARSA, ExpectedSARSA "
                                         "and PAL under the Greedy, EpsilonGreedy, Softmax and Random policies, per-learner f32 tables and no epsilon schedule: "
                                         "this combination is unknown to the library (got domain %d, basis %d, algo %d, policy %d, weight mode %d, dtype %d, "
                                         "epsilon_decay %g)",
                        cfg.domain, cfg.basis, al, cfg.policy, cfg.weight_mode, cfg.weight_dtype, cfg.epsilon_decay);
        return RSRL_HIP_OK;
    }
    // (NAC over the Gibbs policy names itself in every refusal, the continuous domain's and policies' included)
    if (is_gibbs_nac(al)) return check_reg_only(cfg, kAlgo[al], reg && per_env && f32 && !esched);
    if (cfg.domain == RSRL_CONTINUOUS_MOUNTAIN_CAR || cfg.policy == RSRL_BETA || cfg.policy == RSRL_GAUSSIAN || al == RSRL_NAC || al == RSRL_CACLA || al == RSRL_CONTINUOUS_TD_ACTOR_CRITIC)
        return check_continuous(cfg, kAlgo[al], is_cmc_fourier(cfg) && per_env && f32 && !esched);
    if (kAlgo[al].reg_policy >= 0) return check_reg_only(cfg, kAlgo[al], reg && per_env && f32 && !esched);
    if (cfg.domain == RSRL_HIV_TREATMENT) {
        // train_hiv.hip: the one-step agents over the Fourier basis of order 1-3, per-learner f32 weights, one epsilon for the ctx
        if (!one_step || tile || cfg.order > 3 || !per_env || !f32 || esched)
            return fail(RSRL_HIP_EINVAL, "HIVTreatment supports QLearning, SARSA, ExpectedSARSA and PAL on the Fourier basis of order 1-3 with per-learner "
                                         "f32 weights and no epsilon schedule (got algo %d, basis %d, order %d, weight mode %d, dtype %d, epsilon_decay %g)",
                        al, cfg.basis, cfg.order, cfg.weight_mode, cfg.weight_dtype, cfg.epsilon_decay);
        return RSRL_HIP_OK;
    }
    // the weight storage: one shared approximator on the register-family orders or tile coding; bf16 on the order-7 wave family
    if (shared && wave) return fail(RSRL_HIP_EINVAL, "shared weights are not available for the order-7 wave family yet");
    if (shared && !tile && !reg)
        return fail(RSRL_HIP_EINVAL, "shared weights need a register-family Fourier order (MountainCar 1-5, CartPole/Acrobot 1) or tile coding");
    if (!f32 && !wave) return fail(RSRL_HIP_EINVAL, "bf16 weights are available for Fourier order 7 on CartPole / Acrobot only");
    if (!model_supported(cfg))
        return fail(RSRL_HIP_EINVAL, "basis %d (order %d / %d tilings) on domain %d has no kernel yet", cfg.basis, cfg.order, cfg.n_tilings, cfg.domain);
    // the agents
    if (is_pred(al)) {
        if (!per_env) return fail(RSRL_HIP_EINVAL, "the prediction agents (TD, TDLambda) need per-learner weights on a Fourier basis or on tile coding");
        if (cfg.policy != RSRL_RANDOM) return fail(RSRL_HIP_EINVAL, "prediction agents have no Q function: the behaviour policy must be RSRL_RANDOM");
    }
    if (al == RSRL_GREEDY_GQ && !per_env) return fail(RSRL_HIP_EINVAL, "GreedyGQ needs per-learner weights");
    if (al == RSRL_Q_SIGMA && !per_env) return fail(RSRL_HIP_EINVAL, "QSigma needs per-learner weights");
    // SARSALambda / QLambda: dense per-learner traces on any basis (the wave family: f32, or bf16 + stochastic rounding), or sparse per-learner
    // traces over ONE shared tile table (traces.rs:5-12 over params/sparse.rs; its tilings 4, 8 or 16 as every tile model's)
    if (is_lambda(al) && !per_env && !is_sparse_lambda(cfg))
        return fail(RSRL_HIP_EINVAL, "the eligibility-trace agents need per-learner weights on a Fourier basis "
                                     "or on tile coding (per-learner tables, or one shared table with sparse per-learner traces)");
    // the per-learner epsilon schedule: k_train_reg<.., ESCHED>, k_train_lambda, k_train_mem, k_train_wave / k_train_wave_pk <.., ESCHED>, k_wave_lambda
    if (esched && !(cfg.policy == RSRL_EPSILON_GREEDY && per_env && cfg.steps_per_launch != 1 && (one_step || (is_lambda(al) && (reg || wave)))))
        return fail(RSRL_HIP_EINVAL, "epsilon_decay (the per-learner epsilon schedule) needs policy = EpsilonGreedy, per-learner weights, steps_per_launch != 1 and "
                                     "a one-step agent or SARSALambda / QLambda on a register-family or order-7 wave-family Fourier basis, or a one-step agent on "
                                     "tile coding / a generic Fourier order");
    return RSRL_HIP_OK;
}

static int create_impl(const rsrl_hip_config* cfg, rsrl_hip_ctx* c) {
    TRY(check_config(*cfg));
    c->cfg = *cfg;
    c->D = kDomainShape[cfg->domain][0]; c->A = kDomainShape[cfg->domain][1];
    c->F = 1;
    for (int i = 0; i < c->D; ++i) c->F *= cfg->basis == RSRL_FOURIER ? cfg->order + 1 : cfg->tiles_per_dim;
    if (cfg->basis == RSRL_TILE_CODING) c->F *= cfg->n_tilings;
    if (cfg->basis == RSRL_TABLE) c->F = Domain<5>::kCells;      // one row per cell
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(RSRL_HIP_EHIP, "no HIP device");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(RSRL_HIP_EINVAL, "device %d out of range (%d devices)", cfg->device, ndev);
    HIP_TRY(hipSetDevice(cfg->device));
    { int cus = 0; HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device)); if (cus > 0) { c->n_simd = 4 * cus; c->n_cu = cus; } }
    if (cfg->peer_timeout_ms < 0) return fail(RSRL_HIP_EINVAL, "peer_timeout_ms must be >= 0");
    c->sw = read_switches();
    if (cfg->peer_timeout_ms > 0) c->peer_timeout = (uint64_t)cfg->peer_timeout_ms * 100000ull;
    else if (c->sw.peer_timeout_ms > 0) c->peer_timeout = (uint64_t)c->sw.peer_timeout_ms * 100000ull;
    if (cfg->stream) { c->stream = (hipStream_t)cfg->stream; c->own_stream = false; }
    else { HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    const int64_t N = cfg->n_envs;
    const bool shared = cfg->weight_mode == RSRL_W_SHARED;
    c->w_stride = shared ? 1 : N;
    const AlgoRow& agent = kAlgo[cfg->algo];
    c->Aw = agent.v ? 1 : c->A;
    c->Ap = (cfg->policy == RSRL_BETA || cfg->policy == RSRL_GAUSSIAN) ? 2 : (agent.reg_policy == RSRL_SOFTMAX ? c->A : 0);
    // (SCB::n_features: the score's blocks -- two columns, or the Gibbs policy's A -- and the basis itself)
    c->Fw = is_nac(cfg->algo) ? 3 * c->F : (is_gibbs_nac(cfg->algo) ? (c->A + 1) * c->F : c->F);
    c->w_elems = (size_t)c->Aw * c->Fw * (size_t)(shared ? 1 : N);
    c->family = classify(*cfg, c->w_elems);
    // a ctx that steps one batch-step per launch streams W every step: learner-major rows (W[N][A][F]) let k_step_reg_lm
    // write back only the touched column (RSRL_K1_FEATURE_MAJOR=1 keeps the feature-major layout, for A/B runs).  NOT the default layout: the fused loop runs on it
    // bit for bit, but its strided load / store of W costs 71 against 26 us per 20-step launch and 1.3 % of the coalesced rate (round 6, measured)
    if (c->family == AgentFamily::RegStep && (c->A * c->F) % 4 == 0 && c->F % 4 == 0 && !c->sw.k1_feature_major) {
        c->w_stride = 1;
        c->w_ls = (int64_t)c->A * c->F;
        // four lanes per learner (k_step_reg_q4) pays once there is more than one round of one-lane waves to overlap: measured
        // 19.8 vs 21.3 us per launch at 131 072 learners, 32.7 vs 38.0 at 262 144, but 9.8 vs 9.0 at 65 536 (RSRL_K1_QUAD=1 / 0 forces)
        c->k1_quad = c->A <= 3 && (c->sw.k1_quad >= 0 ? c->sw.k1_quad == 1 : N >= 131072);
    }
    // the fused loop with a producer wave per SIMD (kernels_reg_pw.hpp): only while the grid is at most one block per CU -- there a SIMD would hold ONE
    // learner wave, and the partner fills its idle issue slots.  Above it k_train_reg already runs two learner waves per SIMD.  The schedule-free loop
    // only; RSRL_REG_PRODUCER=0 keeps k_train_reg (A/B, same bits)
    if (c->family == AgentFamily::RegFused && !c->sw.no_reg_producer && cfg->epsilon_decay == 1.0 && N <= (int64_t)kBlock * c->n_cu) {
        int lds = 0;
        HIP_TRY(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg->device));
        c->reg_producer = train_reg_pw_serves(cfg->domain, cfg->order, cfg->algo, lds);
    }
    c->train_kernel = train_kernel_name(c);
    c->dw_elems = (size_t)c->Aw * c->F;
    c->n_stat_slots = stat_slots(c->k1_quad ? Slots::Block64 : family_row(c).slots, N, c->F);
    TRY(ctx_alloc(c, &c->state, sizeof(float) * c->D * (size_t)N));
    TRY(ctx_alloc(c, &c->action, sizeof(int32_t) * (size_t)N));
    if (is_continuous(c)) TRY(ctx_alloc(c, &c->action_f, sizeof(float) * (size_t)N, true));
    TRY(ctx_alloc(c, &c->ep_step, sizeof(uint32_t) * (size_t)N));
    c->w_bytes = c->w_elems * (cfg->weight_dtype == RSRL_W_BF16 ? 2 : 4);
    TRY(ctx_alloc(c, &c->W, c->w_bytes));
    TRY(ctx_alloc(c, &c->dW, sizeof(float) * c->dw_elems));
    TRY(ctx_alloc(c, &c->qcache, sizeof(float) * c->A * (size_t)N));
    if (cfg->domain == RSRL_HIV_TREATMENT) TRY(ctx_alloc(c, &c->hiv_y, sizeof(double) * 6 * (size_t)N));      // (set by the domain reset of create)
    // the trait-granular fast path: learner-major per-learner f32 weights on a basis / agent kernels_trait.hpp is instantiated for, one epsilon for the ctx
    if (c->w_ls != 1 && cfg->weight_dtype == RSRL_W_F32 && cfg->epsilon_decay == 1.0 && trait_lm_available(cfg->domain, cfg->order, cfg->algo)) {
        TRY(ctx_alloc(c, &c->tq_key, sizeof(float) * c->D * (size_t)N));
        TRY(ctx_alloc(c, &c->tq_q, sizeof(float) * c->A * (size_t)N));
    }
    if (cfg->algo == RSRL_Q_SIGMA) {                                                  // Backup::new: empty
        TRY(ctx_alloc(c, &c->qs_buf, sizeof(float) * (size_t)(c->D + 5) * (size_t)cfg->n_steps * (size_t)N, true));
        TRY(ctx_alloc(c, &c->qs_head, sizeof(uint32_t) * (size_t)N, true));
        TRY(ctx_alloc(c, &c->qs_len, sizeof(uint32_t) * (size_t)N, true));
    }
    if (cfg->epsilon_decay != 1.0) {
        TRY(ctx_alloc(c, &c->eps, sizeof(float) * (size_t)N));
        hipLaunchKernelGGL(k_fill_f32, dim3(grid_for(N)), dim3(kBlock), 0, c->stream, c->eps, N, (float)cfg->epsilon);
        KCHECK();
    }
    if (c->family == AgentFamily::SharedSparseLambda) {
        const int64_t slice = (int64_t)(c->F / cfg->n_tilings) * c->A;
        if (slice > 65536) return fail(RSRL_HIP_EINVAL, "SARSALambda / QLambda over a shared tile table: one tiling's slice (cells * actions = %lld entries) must not "
                                                        "exceed 65 536 (16-bit slice-relative keys between the step and the trace kernel)", (long long)slice);
        TRY(ctx_alloc(c, &c->sp_len, sizeof(uint32_t) * (size_t)cfg->n_tilings * (size_t)N, true));        // Trace::zeros: empty lists
        // (the lists are written only below their lengths; what lies beyond is never read as an entry, but a checkpoint copies whole rows)
        TRY(ctx_alloc(c, &c->sp_keys, sizeof(uint16_t) * (size_t)kSparseCap * (size_t)N, true));
        TRY(ctx_alloc(c, &c->sp_vals, sizeof(float) * (size_t)kSparseCap * (size_t)N, true));
        c->sp_lds = slice * 8 <= 128 * 1024;
        if (c->sp_lds && slice * 8 > 64 * 1024) c->sp_lds = sparse_trace_scatter_allow_lds(cfg->n_tilings, (int)(slice * 8));      // more dynamic LDS than a kernel gets by default
    } else if (agent.aux != Aux::None) {
        // Trace::zeros; the policy's theta (LFA::vector zero-initialises): of W's shape, or A columns next to V's one
        c->z_bytes = (agent.aux == Aux::Policy ? (size_t)c->Ap * c->F * (size_t)N : c->w_elems) * 4;
        TRY(ctx_alloc(c, &c->Z, c->z_bytes, true));
    }
    if (agent.episode) {      // REINFORCE: theta_b of theta's shape, zero as it is; g = 0
        TRY(ctx_alloc(c, &c->Zb, c->z_bytes, true));
        TRY(ctx_alloc(c, &c->ret_g, sizeof(float) * (size_t)N, true));
    }
    if (agent.lstd) {
        // theta = 0; RecursiveLSTD: C = 1e-5 I; iLSTD (the iLSTD ActorCritic's critic too): A = I, mu = 0 (recursive_lstd.rs:24-33, ilstd.rs:27-40)
        const size_t nv = (size_t)c->F * (size_t)N, nm = nv * (size_t)c->F;
        TRY(ctx_alloc(c, &c->lstd_theta, sizeof(double) * nv, true));
        TRY(ctx_alloc(c, &c->lstd_mat, sizeof(double) * nm));
        // LSTD / LSTDLambda: A = 1e-6 I, b = 0 (in lstd_mu's place), z = 0, no abandoned solve (lstd.rs:23-37, lstd_lambda.rs:25-41)
        const bool batch = is_lstd_batch(cfg->algo);
        launch_lstd_fill_eye(c->stream, c->lstd_mat, (int64_t)nm, c->F, batch ? 1e-6 : (cfg->algo == RSRL_RECURSIVE_LSTD ? 1e-5 : 1.0));
        KCHECK();
        if (cfg->algo != RSRL_RECURSIVE_LSTD) TRY(ctx_alloc(c, &c->lstd_mu, sizeof(double) * nv, true));
        if (cfg->algo == RSRL_LSTD_LAMBDA) TRY(ctx_alloc(c, &c->lstd_z, sizeof(double) * nv, true));
        if (cfg->algo == RSRL_LAMBDA_LSPE) {
            // LambdaLSPE: delta = 0 (lambda_lspe.rs:41) and the row count F -- the identity's F rows make the first system full rank
            const std::vector<double> pair = [&] { std::vector<double> v(2 * (size_t)N, 0.0); for (size_t i = 0; i < (size_t)N; ++i) v[2 * i + 1] = (double)c->F; return v; }();
            TRY(ctx_alloc(c, &c->lstd_z, sizeof(double) * pair.size()));
            HIP_TRY(hipMemcpyAsync(c->lstd_z, pair.data(), sizeof(double) * pair.size(), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        if (batch) TRY(ctx_alloc(c, &c->lstd_sing, sizeof(uint32_t) * (size_t)N, true));
    }
    if (keeps_record(cfg->algo)) {
        // the open episodes (empty: ep_step = 0 below).  Not zero-filled: nothing at or past a learner's ep_step is ever read (get_episode_record shows NaN)
        const uint64_t rows = (uint64_t)cfg->max_episode_steps * (uint64_t)N;      // (<= 2^64 - 2^33: both factors fit 32 bits)
        if (rows > (uint64_t)1 << 40) return fail(RSRL_HIP_ENOMEM, "the episode record: max_episode_steps * n_envs = %llu rows do not fit any device",
                                                  (unsigned long long)rows);
        TRY(ctx_alloc(c, &c->rec_s, (size_t)(rows * (uint64_t)c->D * sizeof(float))));
        TRY(ctx_alloc(c, &c->rec_r, (size_t)(rows * sizeof(float))));
    }
    if (shared) {
        TRY(ctx_alloc(c, &c->flags, (size_t)N));
        if (c->family == AgentFamily::SharedDense) {
            c->sh_rows = (unsigned)((N + kSharedBlock - 1) / kSharedBlock);
            TRY(ctx_alloc(c, &c->sh_tab, sizeof(long long) * 3 * kTabRep * c->dw_elems));
            HIP_TRY(hipMemset(c->sh_tab, 0, sizeof(long long) * 3 * kTabRep * c->dw_elems));
            TRY(ctx_alloc(c, &c->W2, c->w_bytes));
        }
    }
    TRY(ctx_alloc(c, &c->d_stats, sizeof(DevStats) * c->n_stat_slots));
    TRY(ctx_alloc(c, &c->d_t, sizeof(uint64_t)));
    TRY(ctx_alloc(c, &c->d_dyn, sizeof(DynParams)));
    HIP_TRY(hipHostMalloc((void**)&c->h_stats, sizeof(DevStats) * c->n_stat_slots, hipHostMallocDefault));
    HIP_TRY(hipMemsetAsync(c->W, 0, c->w_bytes, c->stream));                      // LFA::vector zero-initialises
    HIP_TRY(hipMemsetAsync(c->dW, 0, sizeof(float) * c->dw_elems, c->stream));
    // shared tile coding: the mini-batch delta is accumulated in 64-bit fixed point, always.  When one tiling's slice, twice, as
    // 64-bit words fits 128 KiB of LDS the scatter is privatised there and flushed into n_rep copies of the table; otherwise
    // every learner adds its term to ONE copy with device atomics (same integers, same sum).
    if (shared && cfg->basis == RSRL_TILE_CODING) {
        c->tile_slice = (int64_t)(c->F / cfg->n_tilings) * c->A * 16 <= 128 * 1024;
        // four copies of the delta table the scatter blocks flush into (us per batch-step at 262 144 learners: 1: 25.7, 2: 24.7, 4: 24.1, 8: 24.8,
        // 16: 26.4).  The scatter fused into the step kernel measured 28.7-35.0: scripts/ab/round6_pruned_knobs.patch
        const bool privatised = c->sp_keys ? c->sp_lds : c->tile_slice;
        c->n_rep = privatised ? 4 : 1;
        TRY(ctx_alloc(c, &c->dW_rep, sizeof(long long) * c->dw_elems * c->n_rep, true));
        if (c->tile_slice || c->sp_keys) {                               // the scatter is a kernel of its own (k_tile_scatter; k_sparse_trace_scatter)
            TRY(ctx_alloc(c, &c->sc_keys, sizeof(uint16_t) * (size_t)cfg->n_tilings * (size_t)N));
            TRY(ctx_alloc(c, &c->sc_terms, sizeof(float) * (size_t)N));
        }
    }
    if (shared) {
        TRY(ctx_alloc(c, &c->d_peer_err, sizeof(uint32_t), true));
        TRY(ctx_alloc(c, &c->h_fx, sizeof(long long) * c->dw_elems, true));
    }
    HIP_TRY(hipMemsetAsync(c->action, 0, sizeof(int32_t) * (size_t)N, c->stream));
    HIP_TRY(hipMemsetAsync(c->ep_step, 0, sizeof(uint32_t) * (size_t)N, c->stream));
    return RSRL_HIP_OK;
}

int rsrl_hip_domain_reset(rsrl_hip_ctx* c, const uint8_t* mask);

int rsrl_hip_create(const rsrl_hip_config* cfg, rsrl_hip_ctx** out) {
    if (!cfg || !out) return fail(RSRL_HIP_EINVAL, "null argument");
    // struct_size-versioned: a caller built against an older header passes a shorter struct; the fields it does not know
    // keep the defaults of rsrl_hip_config_init
    if (cfg->struct_size < RSRL_HIP_CONFIG_SIZE_V3 || cfg->struct_size > sizeof(rsrl_hip_config))
        return fail(RSRL_HIP_EINVAL, "config struct_size %u not in [%u, %zu] (ABI mismatch)", cfg->struct_size,
                    RSRL_HIP_CONFIG_SIZE_V3, sizeof(rsrl_hip_config));
    rsrl_hip_config full;
    rsrl_hip_config_init(&full);
    memcpy(&full, cfg, cfg->struct_size);
    full.struct_size = (uint32_t)sizeof(full);
    cfg = &full;
    rsrl_hip_ctx* c = new rsrl_hip_ctx();
    int rc = create_impl(cfg, c);
    if (rc == RSRL_HIP_OK) rc = rsrl_hip_domain_reset(c, nullptr);     // envs start at Domain::default()
    if (rc == RSRL_HIP_OK) { hipError_t e = hipStreamSynchronize(c->stream); if (e != hipSuccess) rc = fail(RSRL_HIP_EHIP, "%s", hipGetErrorString(e)); }
    if (rc != RSRL_HIP_OK) { std::string keep = g_last_error; rsrl_hip_destroy(c); g_last_error = keep; *out = nullptr; return rc; }
    *out = c;
    return RSRL_HIP_OK;
}

int rsrl_hip_sync(rsrl_hip_ctx* c) {
    CHECK_CTX(c); FLUSH(c);
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return peer_check(c);
}

int rsrl_hip_state_dim(const rsrl_hip_ctx* c) { return c ? c->D : RSRL_HIP_EINVAL; }
int rsrl_hip_n_actions(const rsrl_hip_ctx* c) { return c ? c->A : RSRL_HIP_EINVAL; }
int rsrl_hip_n_outputs(const rsrl_hip_ctx* c) { return c ? c->Aw : RSRL_HIP_EINVAL; }
int rsrl_hip_n_policy_outputs(const rsrl_hip_ctx* c) { return c ? c->Ap : RSRL_HIP_EINVAL; }
int rsrl_hip_n_features(const rsrl_hip_ctx* c) { return c ? c->F : RSRL_HIP_EINVAL; }
int rsrl_hip_n_weight_rows(const rsrl_hip_ctx* c) { return c ? c->Fw : RSRL_HIP_EINVAL; }
int64_t rsrl_hip_n_envs(const rsrl_hip_ctx* c) { return c ? c->cfg.n_envs : RSRL_HIP_EINVAL; }
uint64_t rsrl_hip_step_count(const rsrl_hip_ctx* c) { return c ? c->t + (uint64_t)c->pending : 0; }
int64_t rsrl_hip_pending_steps(const rsrl_hip_ctx* c) { return c ? c->pending : 0; }

int rsrl_hip_state_bounds(const rsrl_hip_ctx* c, double* lo, double* hi) {
    CHECK_CTX(c);
    if (!lo || !hi) return fail(RSRL_HIP_EINVAL, "null argument");
    for (int i = 0; i < c->D; ++i) {
        switch (c->cfg.domain) {
        case 0: lo[i] = Domain<0>::lo_d(i); hi[i] = Domain<0>::hi_d(i); break;
        case 1: lo[i] = Domain<1>::lo_d(i); hi[i] = Domain<1>::hi_d(i); break;
        case 2: lo[i] = Domain<2>::lo_d(i); hi[i] = Domain<2>::hi_d(i); break;
        case 4: lo[i] = Domain<4>::lo_d(i); hi[i] = Domain<4>::hi_d(i); break;
        case 5: lo[i] = Domain<5>::lo_d(i); hi[i] = Domain<5>::hi_d(i); break;
        default: lo[i] = -5.0; hi[i] = 8.0; break;            // HIVTreatment: LIMITS of every observation component (hiv.rs:34, :137-145)
        }
    }
    return RSRL_HIP_OK;
}

int rsrl_hip_action_bounds(const rsrl_hip_ctx* c, double* lo, double* hi) {
    CHECK_CTX(c);
    if (!lo || !hi) return fail(RSRL_HIP_EINVAL, "null argument");
    if (!is_continuous(c)) return fail(RSRL_HIP_EINVAL, "domain %d has a finite action set (rsrl_hip_n_actions = %d indices): only ContinuousMountainCar has action bounds", c->cfg.domain, c->A);
    *lo = Domain<4>::action_lo(); *hi = Domain<4>::action_hi();
    return RSRL_HIP_OK;
}

void state_limits(const rsrl_hip_ctx* c, float* lo, float* hi) {
    double l[8], h[8];
    (void)rsrl_hip_state_bounds(c, l, h);
    // HIVTreatment: an observation outside its bounds is no observation (set_states inverts it through pow(10, obs))
    if (c->hiv_y) { for (int d = 0; d < c->D; ++d) { lo[d] = (float)l[d]; hi[d] = (float)h[d]; } return; }
    for (int d = 0; d < c->D; ++d) { const double w = 1000.0 * (h[d] - l[d]); lo[d] = (float)(l[d] - w); hi[d] = (float)(h[d] + w); }
}

int rsrl_hip_set_epsilon(rsrl_hip_ctx* c, double eps) {
    CHECK_CTX(c); FLUSH(c);
    if (!(eps >= 0.0 && eps <= 1.0)) return fail(RSRL_HIP_EINVAL, "epsilon must be in [0,1]");   // gen_bool panics otherwise
    c->cfg.epsilon = eps;
    if (c->eps) {                                                       // the field of every learner
        HIP_TRY(hipSetDevice(c->cfg.device));
        hipLaunchKernelGGL(k_fill_f32, dim3(grid_for(c->cfg.n_envs)), dim3(kBlock), 0, c->stream, c->eps, c->cfg.n_envs, (float)eps);
        KCHECK();
    }
    return RSRL_HIP_OK;
}
int rsrl_hip_get_epsilons(rsrl_hip_ctx* c, float* eps_out) {
    CHECK_CTX(c); FLUSH(c); if (!eps_out) return fail(RSRL_HIP_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int64_t N = c->cfg.n_envs;
    if (c->eps) {
        HIP_TRY(hipMemcpyAsync(eps_out, c->eps, sizeof(float) * (size_t)N, hipMemcpyDefault, c->stream));
    } else {
        CallFrame f(c);
        float* d_eps;
        TRY(f.out(eps_out, (size_t)N, &d_eps));
        hipLaunchKernelGGL(k_fill_f32, dim3(grid_for(N)), dim3(kBlock), 0, c->stream, d_eps, N, (float)c->cfg.epsilon);
        KCHECK();
        TRY(f.finish());
    }
    HIP_TRY(hipStreamSynchronize(c->stream));      // (an accessor: synchronous for device memory too)
    return RSRL_HIP_OK;
}

int rsrl_hip_reset(rsrl_hip_ctx* c) {
    CHECK_CTX(c); FLUSH(c);
    c->q_valid = false;
    HIP_TRY(hipSetDevice(c->cfg.device));
    // QSigma: fresh episodes start from an empty n-step backup (as after a terminal transition, q_sigma.rs:154) -- entries of the
    // abandoned trajectories must not be mixed into the first anchor updates of the new ones
    if (c->qs_len) HIP_TRY(hipMemsetAsync(c->qs_len, 0, sizeof(uint32_t) * (size_t)c->cfg.n_envs, c->stream));
    // REINFORCE: every episode starts anew, theta_b <- theta, g <- 0 (the initial sample below reads theta, which theta_b now is)
    if (c->family == AgentFamily::ReinforceReg) { launch_reinforce_restart(c->stream, make_reinforce(c), c->cfg.n_envs, (int64_t)c->F * c->A, nullptr); KCHECK(); }
    const Common k = make_policy_common(c);              // the initial policy.sample (ActorCritic: the actor's theta)
    const BasisGeom g = make_geom(c);
    if (is_continuous(c)) {      // (the agents' state is untouched: the initial sample reads the policy's columns)
        if (!launch_cont_reset(c->cfg.order, cont_policy(c), c->stream, k, c->Z, c->t, c->action_f)) return NO_MODEL(c);
    } else if (c->family == AgentFamily::Hiv) {
        launch_hiv_reset(c->stream, k, g, c->hiv_y, c->t);
    } else if (c->family == AgentFamily::CliffTable) {
        launch_table_reset(c->stream, k, c->t);
    } else if (is_v_only(c->cfg.algo)) {       // (the LSTD agents' state is untouched: the weights are not reset either; GradientMC's records empty with ep_step = 0)
        if (!launch_reset_td(c->cfg.domain, dim3(grid_for(k.n_envs)), dim3(kBlock), c->stream, k, c->t)) return NO_MODEL(c);
    } else if (is_wave_family(c->family)) {
        for_wave(c, [&](auto tag) {
            using T = decltype(tag); using WT = typename T::wt;
            hipLaunchKernelGGL((k_wave_reset<T::domain, WT>), dim3(wave_grid_for(k.n_envs)), dim3(kBlock), 0, c->stream, k, (const WT*)c->W, c->t);
        });
    } else if (!for_model(c, [&](auto tag) {
            using M = typename decltype(tag)::type;
            hipLaunchKernelGGL((k_reset<M>), dim3(grid_for(k.n_envs)), dim3(kBlock), 0, c->stream, k, g, c->t);
        })) return NO_MODEL(c);
    KCHECK();
    return RSRL_HIP_OK;
}

int rsrl_hip_get_states(rsrl_hip_ctx* c, float* states) {
    CHECK_CTX(c); FLUSH(c); if (!states) return fail(RSRL_HIP_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipMemcpyAsync(states, c->state, sizeof(float) * c->D * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return peer_check(c);
}
int rsrl_hip_set_states(rsrl_hip_ctx* c, const float* states) {
    CHECK_CTX(c); FLUSH(c);
    if (!states) return fail(RSRL_HIP_EINVAL, "null argument");
    CallFrame f(c);      // (asked where the array lives; nothing is staged: the copy below is the runtime's own)
    TRY(check_host_states(f, states, (size_t)c->cfg.n_envs));
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (f.device(states)) {
        // same rule as for a host array, checked where the data is; a refused array leaves the ctx untouched
        StateLimits lim; state_limits(c, lim.lo, lim.hi);
        TRY(scratch_reserve(c, 7, sizeof(unsigned)));
        unsigned* d_bad = (unsigned*)c->scratch[7].p;
        unsigned bad = 0;
        HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(unsigned), c->stream));
        hipLaunchKernelGGL(k_check_states, dim3(grid_for(c->cfg.n_envs)), dim3(kBlock), 0, c->stream, states, c->cfg.n_envs, c->D, lim, d_bad);
        KCHECK();
        HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (bad) return fail(RSRL_HIP_EINVAL, "%u component(s) of the device array of states are not finite values within 1000 widths of their dimension's bounds", bad);
    }
    c->q_valid = false;
    HIP_TRY(hipMemcpyAsync(c->state, states, sizeof(float) * c->D * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    if (c->hiv_y) { launch_hiv_emit(c->stream, c->hiv_y, c->state, c->cfg.n_envs, true); KCHECK(); }       // HIVTreatment: hidden state = 10^obs
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
int rsrl_hip_get_hidden_states(rsrl_hip_ctx* c, double* y) {
    CHECK_CTX(c); FLUSH(c); if (!y) return fail(RSRL_HIP_EINVAL, "null argument");
    if (!c->hiv_y) return fail(RSRL_HIP_EINVAL, "domain has no hidden state (domain %d): only HIVTreatment keeps one", c->cfg.domain);
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipMemcpyAsync(y, c->hiv_y, sizeof(double) * 6 * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
int rsrl_hip_set_hidden_states(rsrl_hip_ctx* c, const double* y) {
    CHECK_CTX(c); FLUSH(c); if (!y) return fail(RSRL_HIP_EINVAL, "null argument");
    if (!c->hiv_y) return fail(RSRL_HIP_EINVAL, "domain has no hidden state (domain %d): only HIVTreatment keeps one", c->cfg.domain);
    HIP_TRY(hipSetDevice(c->cfg.device));
    c->q_valid = false;
    HIP_TRY(hipMemcpyAsync(c->hiv_y, y, sizeof(double) * 6 * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    launch_hiv_emit(c->stream, c->hiv_y, c->state, c->cfg.n_envs, false);        // the observations follow
    KCHECK();
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
int rsrl_hip_get_actions(rsrl_hip_ctx* c, int32_t* actions) {
    CHECK_CTX(c); FLUSH(c); if (!actions) return fail(RSRL_HIP_EINVAL, "null argument");
    NEEDS_INDEX_ACTIONS(c, "rsrl_hip_get_actions");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipMemcpyAsync(actions, c->action, sizeof(int32_t) * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
int rsrl_hip_set_actions(rsrl_hip_ctx* c, const int32_t* actions) {
    CHECK_CTX(c); FLUSH(c); if (!actions) return fail(RSRL_HIP_EINVAL, "null argument");
    NEEDS_INDEX_ACTIONS(c, "rsrl_hip_set_actions");
    HIP_TRY(hipSetDevice(c->cfg.device));
    CallFrame f(c);
    TRY(check_host_actions(f, actions, (size_t)c->cfg.n_envs, c->A));
    HIP_TRY(hipMemcpyAsync(c->action, actions, sizeof(int32_t) * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    hipLaunchKernelGGL(k_clamp_actions, dim3(grid_for(c->cfg.n_envs)), dim3(kBlock), 0, c->stream, c->action, c->cfg.n_envs, c->A);
    KCHECK();
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
// the f32 twins (a continuous ctx's pending actions)
int rsrl_hip_get_actions_f32(rsrl_hip_ctx* c, float* actions) {
    CHECK_CTX(c); FLUSH(c); if (!actions) return fail(RSRL_HIP_EINVAL, "null argument");
    NEEDS_F32_ACTIONS(c, "rsrl_hip_get_actions");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipMemcpyAsync(actions, c->action_f, sizeof(float) * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
int rsrl_hip_set_actions_f32(rsrl_hip_ctx* c, const float* actions) {
    CHECK_CTX(c); FLUSH(c); if (!actions) return fail(RSRL_HIP_EINVAL, "null argument");
    NEEDS_F32_ACTIONS(c, "rsrl_hip_set_actions");
    HIP_TRY(hipSetDevice(c->cfg.device));
    CallFrame f(c);
    TRY(check_host_actions_f32(f, actions, (size_t)c->cfg.n_envs, !is_gaussian(c)));      // (a Gaussian sample is any finite f32)
    HIP_TRY(hipMemcpyAsync(c->action_f, actions, sizeof(float) * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    if (!is_gaussian(c)) { launch_cmc_clamp_actions(c->stream, c->action_f, c->cfg.n_envs); KCHECK(); }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}

// ---- ABI 8: the learners' state between two driver calls that is neither weights nor env state (include/rsrl_hip.h)
int rsrl_hip_get_episode_steps(rsrl_hip_ctx* c, uint32_t* steps) {
    CHECK_CTX(c); FLUSH(c); if (!steps) return fail(RSRL_HIP_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipMemcpyAsync(steps, c->ep_step, sizeof(uint32_t) * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return peer_check(c);
}
int rsrl_hip_set_episode_steps(rsrl_hip_ctx* c, const uint32_t* steps) {
    CHECK_CTX(c); FLUSH(c); if (!steps) return fail(RSRL_HIP_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (keeps_record(c->cfg.algo)) {
        // k_train_gmc / k_train_lstd_batch index the learner's record by it: checked before anything is installed (a device array through a host copy)
        const size_t n = (size_t)c->cfg.n_envs;
        std::vector<uint32_t> h(n);
        HIP_TRY(hipMemcpyAsync(h.data(), steps, sizeof(uint32_t) * n, hipMemcpyDefault, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < n; ++i)
            if (h[i] > c->cfg.max_episode_steps)
                return fail(RSRL_HIP_EINVAL, "episode_steps[%zu] = %u is more than max_episode_steps = %u, the rows of the episode record", i, h[i],
                            c->cfg.max_episode_steps);
    }
    HIP_TRY(hipMemcpyAsync(c->ep_step, steps, sizeof(uint32_t) * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
// GradientMC's open episodes (rec_s / rec_r): read with NaN past each learner's episode_steps, installed whole
static const char* const kNoEpisodeRecord = "only GradientMC, LSTD, LSTDLambda and LambdaLSPE (RSRL_GRADIENT_MC, RSRL_LSTD, RSRL_LSTD_LAMBDA, RSRL_LAMBDA_LSPE) keep the learners' open episodes on the device";
int rsrl_hip_get_episode_record(rsrl_hip_ctx* c, float* states, float* rewards) {
    CHECK_CTX(c); FLUSH(c); if (!states || !rewards) return fail(RSRL_HIP_EINVAL, "null argument");
    if (!keeps_record(c->cfg.algo)) return fail(RSRL_HIP_ESTATE, "%s", kNoEpisodeRecord);
    HIP_TRY(hipSetDevice(c->cfg.device));
    const int64_t N = c->cfg.n_envs, cap = (int64_t)c->cfg.max_episode_steps;
    CallFrame f(c);
    float* d_states; float* d_rew;
    TRY(f.out(states, (size_t)cap * (size_t)c->D * (size_t)N, &d_states));
    TRY(f.out(rewards, (size_t)cap * (size_t)N, &d_rew));
    launch_gmc_record_get(c->stream, make_gmc(c), c->ep_step, N, cap, c->D, d_states, d_rew);
    KCHECK();
    TRY(f.finish());
    HIP_TRY(hipStreamSynchronize(c->stream));      // (an accessor: synchronous for device memory too)
    return RSRL_HIP_OK;
}
int rsrl_hip_set_episode_record(rsrl_hip_ctx* c, const float* states, const float* rewards) {
    CHECK_CTX(c); FLUSH(c); if (!states || !rewards) return fail(RSRL_HIP_EINVAL, "null argument");
    if (!keeps_record(c->cfg.algo)) return fail(RSRL_HIP_ESTATE, "%s", kNoEpisodeRecord);
    HIP_TRY(hipSetDevice(c->cfg.device));
    const size_t rows = (size_t)c->cfg.max_episode_steps * (size_t)c->cfg.n_envs;
    HIP_TRY(hipMemcpyAsync(c->rec_s, states, sizeof(float) * rows * (size_t)c->D, hipMemcpyDefault, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rec_r, rewards, sizeof(float) * rows, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
int rsrl_hip_get_q_carry(rsrl_hip_ctx* c, float* q, int32_t* valid) {
    CHECK_CTX(c); FLUSH(c); if (!q || !valid) return fail(RSRL_HIP_EINVAL, "null argument");
    *valid = (carries_q(c) && c->q_valid) ? 1 : 0;
    if (!*valid) return RSRL_HIP_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipMemcpyAsync(q, c->qcache, sizeof(float) * (size_t)c->A * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RSRL_HIP_OK;
}
int rsrl_hip_set_q_carry(rsrl_hip_ctx* c, const float* q) {
    CHECK_CTX(c); FLUSH(c); if (!q) return fail(RSRL_HIP_EINVAL, "null argument");
    if (!carries_q(c)) return fail(RSRL_HIP_EINVAL, "this ctx's kernels evaluate Q(s,.) from the weights every step: there is nothing carried to restore");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipMemcpyAsync(c->qcache, q, sizeof(float) * (size_t)c->A * (size_t)c->cfg.n_envs, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->q_valid = true;
    return RSRL_HIP_OK;
}

int rsrl_hip_timing_enable(rsrl_hip_ctx* c, int enable) {
    CHECK_CTX(c); FLUSH(c);
    c->timing = enable != 0;
    c->events_used = 0;
    return RSRL_HIP_OK;
}
int rsrl_hip_timing_read(rsrl_hip_ctx* c, double* ms_total, uint64_t* launches, const char** kernel_name) {
    CHECK_CTX(c); FLUSH(c);
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    double tot = 0.0;
    for (size_t i = 0; i < c->events_used; ++i) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, c->events[i].first, c->events[i].second));
        tot += ms;
    }
    if (ms_total) *ms_total = tot;
    if (launches) { uint64_t n = 0; for (size_t i = 0; i < c->events_used; ++i) n += c->event_launches[i]; *launches = n; }
    if (kernel_name) *kernel_name = c->kernel_name;
    return RSRL_HIP_OK;
}
RSRL_API_END
