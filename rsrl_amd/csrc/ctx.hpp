// ctx.hpp -- what the translation units of the C ABI (abi_*.hip; include/rsrl_hip.h) share: the ctx, error reporting, the (basis, domain, order) -> model
// dispatch, host / device pointer staging, and the small kernels more than one unit launches.  Internal: nothing here is exported.
//   abi_ctx.hip      create / destroy, configuration, env state accessors, reset, timing hooks
//   abi_trait.hip    the trait-granular entry points: Domain::transition, Function / Enumerable, Policy, Handler::handle (+ the deferred trait loop)
//   abi_weights.hip  Parameterised (weights, traces, fa_td), checkpoints, checksums
//   abi_train.hip    the fused driver loop: launch shapes, step graphs, the persistent shared-W kernel, rollouts
//   abi_group.hip    multi-rank: RCCL communicators, the peer exchange set-up, single-process groups
//   kernels_util.hip, launch_shared.hip   the small kernels / the kernel-template launches more than one of those units needs (one copy of the machine code)
#pragma once
//
// One ctx = one HIP device + one stream + one (domain, basis, algo, policy, N, W-mode)
// instance, i.e. what the reference builds in examples/q_learning.rs:19-32.  There is no
// CPU path in this library: every entry point launches HIP kernels.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <unistd.h>
#include <dlfcn.h>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rsrl_hip.h"
// everything below is internal to the library: only what include/rsrl_hip.h declared (above, default visibility) is exported
#pragma GCC visibility push(hidden)
#define RSRL_API_BEGIN _Pragma("GCC visibility push(default)") extern "C" {
#define RSRL_API_END } _Pragma("GCC visibility pop")
#include "launch.hpp"
#include "models.hpp"
#include "model_list.hpp"
#include "kernels_wave.hpp"
#include "kernels_lambda.hpp"
#include "kernels_gq.hpp"
#include "kernels_td.hpp"
#include "kernels_qsigma.hpp"
#include "kernels_persist.hpp"
#include "kernels_wave_lambda.hpp"
#include "kernels_wave_aux.hpp"
#include "kernels_sparse_lambda.hpp"
#include "kernels_trait.hpp"
#include "kernels_ac.hpp"

using namespace rsrl;

// ---- THE agent table: what the reference's agent of each rsrl_algo is, one row per number.  Admission (check_config), the ctx's buffers (create_impl),
// the accessors and the checkpoint read it; a new agent adds its row here, a line of classify() and a case of launch_agent ("Adding an agent").
enum class Agent : uint8_t { None, OneStep, Lambda, Gq, Pred, QSigma, Ac, TdAc, Reinforce, Lstd, TdAcLstd, Gmc, LstdBatch, Nac, Gtd, Cacla, TdAcCont, GibbsNac };      // the group classify() and the kernels' dispatch know it by
enum class Aux : uint8_t { None, LikeW, Policy };      // the second per-learner matrix Z: none, of W's shape, or the actor's A columns next to a one-column W
struct AlgoRow {
    const char* name = nullptr;      // as the admission messages print it (nullptr: the number is unassigned)
    Agent agent = Agent::None;
    bool v = false;                  // the value function has ONE column (V: ScalarLFA, or the f64 theta) instead of A
    Aux aux = Aux::None;             // Z: traces (Lambda, TDLambda), fa_td's weights (Gq), the policy's theta (the actor-critics, REINFORCE)
    int aux_kind = 0;                // the checkpoint's (abi_weights.hip kCkptKind), unless the configuration decides it (aux_kind_of)
    bool episode = false;            // REINFORCE's open episode: the behaviour snapshot Zb and the running return ret_g
    bool lstd = false;               // the f64 least-squares state (lstd_theta / lstd_mat / lstd_mu) is the value function
    // the agents that exist only on the register-family Fourier orders with per-learner f32 weights (check_reg_only): the policy they require (-1: not
    // one of them), the message's words behind it and behind "agent_policy = -1", and what it calls config.n_steps in front of "n_updates" (nullptr: not read)
    int reg_policy = -1; const char* policy_words = ""; const char* shares_words = ""; const char* n_updates = nullptr;
};
constexpr int kLastAlgo = RSRL_LAMBDA_LSPE;      // the highest assigned number (RSRL_CACLA stays the enum's textually last enumerator)
constexpr AlgoRow kAlgo[kLastAlgo + 1] = {
    /*  0 */ {"QLearning", Agent::OneStep},
    /*  1 */ {"SARSA", Agent::OneStep},
    /*  2 */ {"ExpectedSARSA", Agent::OneStep},
    /*  3 */ {"SARSALambda", Agent::Lambda, false, Aux::LikeW, 1},
    /*  4 */ {"QLambda", Agent::Lambda, false, Aux::LikeW, 1},
    /*  5 */ {"PAL", Agent::OneStep},
    /*  6 */ {"GreedyGQ", Agent::Gq, false, Aux::LikeW, 2},
    /*  7 */ {"TD", Agent::Pred, true},
    /*  8 */ {"TDLambda", Agent::Pred, true, Aux::LikeW, 1},
    /*  9 */ {"QSigma", Agent::QSigma, false, Aux::None, 3},
    /* 10 */ {"ActorCritic", Agent::Ac, false, Aux::LikeW, 5, false, false, RSRL_SOFTMAX, " (the Gibbs actor)", " (the critic shares the actor)"},
    /* 11 */ {"ActorCritic", Agent::Ac, false, Aux::LikeW, 5, false, false, RSRL_SOFTMAX, " (the Gibbs actor)", " (the critic shares the actor)"},
    /* 12 */ {},
    // (the TD / iLSTD ActorCritic: W is V's one column, theta has A)
    /* 13 */ {"the TD ActorCritic (RSRL_TD_ACTOR_CRITIC)", Agent::TdAc, true, Aux::Policy, 6, false, false, RSRL_SOFTMAX, " (the Gibbs actor)"},
    /* 14 */ {},
    // (theta in Z, theta_b in Zb; W is the baseline B -- REINFORCE: allocated, never read)
    /* 15 */ {"REINFORCE (RSRL_REINFORCE)", Agent::Reinforce, false, Aux::LikeW, 7, true, false, RSRL_SOFTMAX, " (the Gibbs policy)"},
    /* 16 */ {"BaselineREINFORCE (RSRL_BASELINE_REINFORCE)", Agent::Reinforce, false, Aux::LikeW, 7, true, false, RSRL_SOFTMAX, " (the Gibbs policy)"},
    /* 17 */ {},
    // (the least-squares agents: W is allocated, one zero column, never read)
    /* 18 */ {"RecursiveLSTD (RSRL_RECURSIVE_LSTD)", Agent::Lstd, true, Aux::None, 8, false, true, RSRL_RANDOM},
    /* 19 */ {"iLSTD (RSRL_ILSTD)", Agent::Lstd, true, Aux::None, 8, false, true, RSRL_RANDOM, "", "", ""},
    /* 20 */ {},
    /* 21 */ {"the iLSTD ActorCritic (RSRL_ILSTD_ACTOR_CRITIC)", Agent::TdAcLstd, true, Aux::Policy, 9, false, true, RSRL_SOFTMAX, " (the Gibbs actor)", "", "the critic's "},
    /* 22 */ {},
    // (W is V's one column, TD's layout; the open episodes live in rec_s / rec_r)
    /* 23 */ {"GradientMC (RSRL_GRADIENT_MC)", Agent::Gmc, true, Aux::None, 0, false, false, RSRL_RANDOM},
    /* 24 */ {},
    // (the batch least-squares agents: W as the LSTD agents'; A in lstd_mat, b in lstd_mu, z / singular_solves of their own, the open episodes in rec_s / rec_r)
    /* 25 */ {"LSTD (RSRL_LSTD)", Agent::LstdBatch, true, Aux::None, 10, false, true, RSRL_RANDOM},
    /* 26 */ {"LSTDLambda (RSRL_LSTD_LAMBDA)", Agent::LstdBatch, true, Aux::None, 10, false, true, RSRL_RANDOM},
    /* 27 */ {},
    // (W is the SCB critic's one column of 3F rows -- weight_rows() --, the Beta or the Gaussian policy's two columns in Z; admitted by check_continuous, not
    // check_reg_only; aux_kind 12 with Beta, 14 with Gaussian: aux_kind_of)
    /* 28 */ {"NAC (RSRL_NAC)", Agent::Nac, true, Aux::Policy, 12},
    /* 29 */ {},
    // (the gradient-TD agents: W is theta's one column, TD's layout; Z is the second column w -- fa_w / td_est --, [F][1])
    /* 30 */ {"GTD2 (RSRL_GTD2)", Agent::Gtd, true, Aux::LikeW, 13, false, false, RSRL_RANDOM},
    /* 31 */ {"TDC (RSRL_TDC)", Agent::Gtd, true, Aux::LikeW, 13, false, false, RSRL_RANDOM},
    /* 32 */ {},
    // (W is the V learner's one column, TD's layout; the Gaussian policy's two columns in Z; admitted by check_continuous, not check_reg_only)
    /* 33 */ {"CACLA (RSRL_CACLA)", Agent::Cacla, true, Aux::Policy, 15},
    /* 34 */ {},
    // (CACLA's layout: W is the V learner's one column, the Gaussian or the Beta policy's two columns in Z; admitted by check_continuous; aux_kind 16 with
    // Beta, 17 with Gaussian: aux_kind_of)
    /* 35 */ {"the continuous TD ActorCritic (RSRL_CONTINUOUS_TD_ACTOR_CRITIC)", Agent::TdAcCont, true, Aux::Policy, 16},
    /* 36 */ {},
    // (W is the SCB critic's one column of (A+1) F rows -- weight_rows() --, the Gibbs policy's theta, A columns, in Z; config.n_steps is the actor's period,
    // checked by check_reg_only itself)
    /* 37 */ {"NAC over the Gibbs policy (RSRL_GIBBS_NAC)", Agent::GibbsNac, true, Aux::Policy, 18, false, false, RSRL_SOFTMAX, " (the Gibbs policy)", " (the critic shares the policy)"},
    /* 38 */ {},
    // (LSTDLambda's row in every column but the checkpoint's: lstd_z holds (delta, rows) per learner instead of the trace)
    /* 39 */ {"LambdaLSPE (RSRL_LAMBDA_LSPE)", Agent::LstdBatch, true, Aux::None, 19, false, true, RSRL_RANDOM},
};
// (readers of the table, for configurations check_config has admitted: the algo is a row with a name)
static inline bool is_lambda(int algo) { return kAlgo[algo].agent == Agent::Lambda; }
static inline bool is_pred(int algo) { return kAlgo[algo].agent == Agent::Pred; }
static inline bool is_ac(int algo) { return kAlgo[algo].agent == Agent::Ac; }
static inline bool is_tdac(int algo) { return kAlgo[algo].agent == Agent::TdAc; }
static inline bool is_reinforce(int algo) { return kAlgo[algo].agent == Agent::Reinforce; }
static inline bool is_lstd(int algo) { return kAlgo[algo].agent == Agent::Lstd; }
static inline bool is_tdac_lstd(int algo) { return kAlgo[algo].agent == Agent::TdAcLstd; }
static inline bool is_gmc(int algo) { return kAlgo[algo].agent == Agent::Gmc; }
static inline bool is_lstd_batch(int algo) { return kAlgo[algo].agent == Agent::LstdBatch; }
// the batch agents' lstd_z, doubles per learner: LSTDLambda's trace z[F]; LambdaLSPE's (delta, rows); LSTD has none
static inline size_t lstd_z_per_learner(int algo, int F) { return algo == RSRL_LSTD_LAMBDA ? (size_t)F : (algo == RSRL_LAMBDA_LSPE ? 2 : 0); }
static inline bool is_nac(int algo) { return kAlgo[algo].agent == Agent::Nac; }
static inline bool is_gtd(int algo) { return kAlgo[algo].agent == Agent::Gtd; }
static inline bool is_cacla(int algo) { return kAlgo[algo].agent == Agent::Cacla; }
static inline bool is_tdac_cont(int algo) { return kAlgo[algo].agent == Agent::TdAcCont; }
static inline bool is_gibbs_nac(int algo) { return kAlgo[algo].agent == Agent::GibbsNac; }
// the agents with NAC::handle(()) (rsrl_hip_nac_update): over the continuous policies, or over the Gibbs policy
static inline bool has_nac_update(int algo) { return is_nac(algo) || is_gibbs_nac(algo); }
// the continuous agents whose value function is a TD(0) V learner in W, TD's layout (rsrl_hip_q_evaluate -> V(s): k_v_evaluate)
static inline bool is_td_v_continuous(int algo) { return is_cacla(algo) || is_tdac_cont(algo); }
// the agents that keep every learner's open episode on the device (rec_s / rec_r, max_episode_steps rows) and sweep it when it ends
static inline bool keeps_record(int algo) { return is_gmc(algo) || is_lstd_batch(algo); }
// the agents whose value function is V alone and whose behaviour is Random: no action values to search, weigh, sample from or roll out with
static inline bool is_v_only(int algo) { return is_pred(algo) || is_lstd(algo) || is_gmc(algo) || is_lstd_batch(algo) || is_gtd(algo); }

// ---- the small kernels more than one unit launches, and the launches of kernel templates two units would otherwise both instantiate: defined ONCE, in
// kernels_util.hip / launch_shared.hip (a kernel's host stub is an ordinary function: another unit launches it through this declaration)
__global__ __launch_bounds__(256) void k_apply_rep(float* __restrict__ W, float* __restrict__ dW, long long* __restrict__ rep, int n_rep, int n, float lsb);
__global__ __launch_bounds__(1024) void k_tile_scatter(const uint16_t* __restrict__ keys, const float* __restrict__ terms, int64_t N, int S, int per_block, long long* __restrict__ dW64, int n_rep, int64_t rep_stride, float inv_lsb);
__global__ __launch_bounds__(256) void k_fx_finalize(long long* __restrict__ fx, float* __restrict__ dW, int n, float lsb);
__global__ void k_clamp_actions(int32_t* __restrict__ a, int64_t n, int A);
__global__ __launch_bounds__(256) void k_peer_push(const float* __restrict__ dW, int n, uint2* const* __restrict__ peers, int world, int rank, uint64_t t, const uint64_t* __restrict__ t_dev, int64_t xdelta);
__global__ __launch_bounds__(256) void k_peer_reduce(float* __restrict__ dW, int n, const uint2* __restrict__ recv, int world, uint64_t t, const uint64_t* __restrict__ t_dev, int64_t xdelta, uint32_t* __restrict__ err, uint64_t timeout);
__global__ __launch_bounds__(kBlock) void k_tab_finalize(const long long* __restrict__ tab, int n, float lr, float* __restrict__ dW, uint64_t t, const uint64_t* __restrict__ t_dev);
__global__ __launch_bounds__(256) void k_tab_exchange_apply(const long long* __restrict__ tab, int n, float lr, uint2* const* __restrict__ peers, const uint2* __restrict__ recv, float* __restrict__ W, int world, int rank, uint64_t t, const uint64_t* __restrict__ t_dev, int64_t xdelta, uint32_t* __restrict__ err, uint64_t timeout);
__global__ void k_fill_f32(float* __restrict__ p, int64_t n, float v);
__global__ void k_set_dyn(DynParams* __restrict__ d, DynParams v);
__global__ void k_set_t(uint64_t* __restrict__ t_dev, uint64_t v);
__global__ void k_advance_t(uint64_t* __restrict__ t_dev, uint64_t d);
__global__ void k_apply_dw(float* __restrict__ W, float* __restrict__ dW, int n);
__global__ void k_weights_get(const float* __restrict__ W, bool tile, int64_t stride, int64_t wi, int F, int A, float* __restrict__ out);
__global__ void k_weights_set(float* __restrict__ W, bool tile, int64_t stride, int64_t wi, int F, int A, const float* __restrict__ in);
__global__ void k_weights_set_all(float* __restrict__ W, bool tile, int64_t N, int64_t stride, int64_t ls, int F, int A, const float* __restrict__ in);
__global__ void k_checksum_lm(const uint32_t* __restrict__ p, int64_t N, int AF, unsigned long long* __restrict__ out);
__global__ void k_checksum(const uint32_t* __restrict__ p, size_t n, size_t index_offset, unsigned long long* __restrict__ out);
struct rsrl_hip_ctx;
// the order-7 wave family's memory-sweep agents (GreedyGQ / TD / TDLambda: k_wave_aux; QSigma: k_wave_qsigma; SARSALambda / QLambda: k_wave_lambda), driver loop
// (io == nullptr: n_steps batch-steps of the ctx's learners) or Handler::handle on io's caller-supplied transitions
void launch_wave_agent(const rsrl_hip_ctx* c, const rsrl::Common& k, uint64_t t, int n_steps, rsrl::DevStats* d_stats, const rsrl::Transitions* io);
// the trace update + LDS scatter of the sparse-trace lambda agents for learners 0 .. n_learners-1 (kernels_sparse_lambda.hpp)
void launch_sparse_trace_scatter(const rsrl_hip_ctx* c, int64_t n_learners, int per_block);
// dynamic LDS beyond the default for that kernel (a tiling's slice of more than 64 KiB): false when the runtime refuses
bool sparse_trace_scatter_allow_lds(int n_tilings, int bytes);

// ------------------------------------------------------------------------------- errors
extern thread_local std::string g_last_error;      // (abi_ctx.hip)

int fail(int code, const char* fmt, ...);           // records the message for rsrl_hip_last_error() and returns `code` (abi_ctx.hip)
// Softmax with tau < 0 (create's tau / agent_tau, the policy rollout's tau); arguments: the field's name, its value
#define NEGATIVE_TAU_MSG "%s = %g: only positive Softmax temperatures are evaluated -- the kernels compute exp((q - max q) / tau), whose exponents are " \
                         ">= 0 for tau < 0 and overflow fp32 once (max q - min q) / |tau| exceeds 88.7 (inf / inf), where the reference's f64 form " \
                         "still returns ordinary probabilities"
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(_e == hipErrorOutOfMemory ? RSRL_HIP_ENOMEM : RSRL_HIP_EHIP, "%s failed: %s (%s:%d)", \
                        #expr, hipGetErrorString(_e), __FILE__, __LINE__);                         \
    } while (0)
#define CHECK_CTX(ctx) do { if (!(ctx)) return fail(RSRL_HIP_EINVAL, "null ctx"); } while (0)

// ------------------------------------------------------------------------------- ctx
struct Scratch { void* p = nullptr; size_t cap = 0; };

// The kernel family that serves a ctx: decided once, by classify() in rsrl_hip_create; the driver loop, handle, reset, the Q operations, rollouts and
// the launch shapes switch on it.  Listed in the order classify() tests them (first match wins).
enum class AgentFamily : uint8_t {
    SharedDense,          // shared W, Fourier: k_shared_step / k_shared_persist
    SharedTile,           // shared W, tile coding: k_shared_ca (+ k_tile_scatter)
    SharedSparseLambda,   // SARSALambda / QLambda over one shared tile table, sparse per-learner traces: k_shared_ca + k_sparse_trace_scatter
    WaveAux,              // order-7 wave family, GreedyGQ / TD / TDLambda: k_wave_aux
    TdTile,               // TD / TDLambda, tile coding: k_td_tile
    TdGeneric,            // ... generic Fourier orders: k_td_mem
    TdReg,                // ... register-family Fourier: k_train_td
    WaveQSigma,           // k_wave_qsigma
    QSigmaReg,            // QSigma, register-family Fourier: k_train_qsigma<FourierModel>
    QSigmaGeneric,        // ... tile coding, generic Fourier orders: k_train_qsigma<M>
    GqReg,                // GreedyGQ, register-family Fourier: k_train_gq
    GqGeneric,            // ... tile coding, generic Fourier orders: k_train_gq_mem
    LambdaTile,           // SARSALambda / QLambda, per-learner tile tables: k_lambda_tile
    WaveLambda,           // k_wave_lambda
    LambdaGeneric,        // ... generic Fourier orders: k_train_lambda_mem4
    LambdaReg,            // ... register-family Fourier: k_train_lambda
    WaveControl,          // order-7 wave family, one-step agents: k_train_wave (f32) / k_train_wave_pk (bf16)
    RegStep,              // register family, one batch-step per launch: k_step_reg / k_step_reg_lm / k_step_reg_q4
    RegFused,             // register family, fused loop: k_train_reg
    Generic,              // one-step agents on tile coding / generic Fourier orders, per-learner weights: k_train_mem
    Hiv,                  // HIVTreatment (f64 hidden state): one-step agents, per-learner weights, Fourier orders 1-3: k_hiv_train (train_hiv.hip)
    AcReg,                // ActorCritic (both critics), register-family Fourier, per-learner f32 weights: k_train_ac (train_ac.hip); theta in Z
    TdAcReg,              // ActorCritic with the TD(0) V critic, same configurations: k_train_tdac (train_tdac.hip); w in W (one column), theta in Z (A columns)
    ReinforceReg,         // REINFORCE / BaselineREINFORCE, same configurations: k_train_reinforce (train_reinforce.hip); B in W, theta in Z, theta_b in Zb, g in ret_g
    LstdReg,              // RecursiveLSTD / iLSTD, register-family Fourier, per-learner state: k_train_lstd (train_lstd.hip); f64 state in lstd_theta / lstd_mat / lstd_mu
    TdAcLstdReg,          // ActorCritic with the iLSTD critic, same configurations as TdAcReg: k_train_tdac_lstd (train_tdac_lstd.hip); iLSTD's f64 state as
                          // LstdReg's, theta in Z (A columns)
    GmcReg,               // GradientMC, same configurations as LstdReg: k_train_gmc (train_gmc.hip); w in W (one column), the open episodes in rec_s / rec_r
    LstdBatchReg,         // LSTD / LSTDLambda, same configurations as GmcReg: k_train_lstd_batch (train_lstd_batch.hip); f64 state in lstd_theta / lstd_mat (A) /
                          // lstd_mu (b) / lstd_z / lstd_sing, the open episodes in rec_s / rec_r.  LambdaLSPE too: k_train_lspe (train_lspe.hip), named by
                          // train_kernel_name; lstd_z is (delta, rows) per learner
    TdAcBetaReg,          // ActorCritic with the iLSTD critic and the Beta policy on ContinuousMountainCar, Fourier orders 1-5: k_train_tdac_beta
                          // (train_tdac_beta.hip); iLSTD's f64 state as LstdReg's, the policy's two columns in Z, f32 actions in action_f
    NacBetaReg,           // NAC with the Beta policy and the SCB SARSA critic on ContinuousMountainCar, Fourier orders 1-5: k_train_nac<ORDER, Beta>, reported as k_train_nac_beta (train_nac.hip),
                          // one thread per learner; the critic's w in W (3F rows, one column), the policy's two columns in Z, f32 actions in action_f
    GtdReg,               // GTD2 / TDC, same configurations as LstdReg: k_train_gtd (train_gtd.hip); theta in W (one column), the second column w in Z
    NacGaussReg,          // NAC with the Gaussian policy, NacBetaReg's configurations and layout: k_train_nac<ORDER, Gaussian>, reported as k_train_nac_gauss (train_nac.hip); the policy's columns
                          // (the mean's, the stddev's) in Z
    CaclaGaussReg,        // CACLA over the Gaussian policy with a TD(0) critic, NacBetaReg's configurations: k_train_td0_cont<ORDER, CaclaRule>, reported as k_train_cacla (train_cont.hip); the V learner's w
                          // in W (one column, F rows), the policy's columns in Z, f32 actions in action_f
    TdAcGaussReg,         // ActorCritic::tdac with a TD(0) critic over the Gaussian policy, CaclaGaussReg's configurations and layout: k_train_tdac_cont
                          // (train_cont.hip)
    TdAcBetaTdReg,        // ... over the Beta policy (the columns alpha's and beta's; the loop hands the domain 2a - 1): k_train_tdac_cont.  (TdAcBetaReg is
                          // the iLSTD critic's family)
    GibbsNacReg,          // NAC over the Gibbs policy with the SCB SARSA critic, AcReg's configurations: k_train_gibbs_nac (train_gibbs_nac.hip); the critic's w in W
                          // ((A+1) F rows, one column), theta in Z (A columns)
    CliffTable,           // CliffWalk over the tabular Q (RSRL_TABLE): one-step agents, per-learner f32 tables W f32[4][60][N]: k_table_train_lds, or
                          // k_table_train_mem for launches below kTableMemBelow batch-steps (train_table.hip)
};
constexpr size_t kAgentFamilies = (size_t)AgentFamily::CliffTable + 1;      // (the enum's last value)
// ---- THE family table: which kernels serve a family and what they can do, one row per AgentFamily value in the enum's order.  classify() (abi_ctx.hip: a
// decision) and launch_agent (abi_train.hip: it instantiates the templates) are the two other places a new family is entered.
enum class Slots : uint8_t { Block, Block64, WaveBlock, Learner, LstdGroup };      // a statistics slot per: kBlock learners, 64 learners (k_train_lambda_mem4; the
                                                                                   // ctx's k1_quad), wave-family block, learner (a block each), kBlock lanes of G per learner
enum class Handle : uint8_t { Model, Wave, Agent };      // rsrl_hip_handle's kernel: k_handle<Model>, k_wave_handle, or the family's own through launch_agent
enum : uint8_t { kWave = 1, kCarriesQ = 2, kPolicyW = 4, kVCritic = 8, kLstd = 16, kBatchLstd = 32 };
struct FamilyRow {
    AgentFamily family;      // (its own index: checked below)
    const char* kernel;      // the driver-loop kernel timing_read names (WaveControl, RegStep: refined by train_kernel_name)
                             // A LABEL, not always a symbol: k_train_cacla, k_train_tdac_cont, k_train_nac_gauss and k_train_nac_beta are the agents' names for
                             // k_train_td0_cont<ORDER, Rule> and k_train_nac<ORDER, P> (kernels_cont.hpp), which is what a profiler's trace shows
    int depth;               // batch-steps per launch while config.steps_per_launch == 0 (the shared families: not read, they step one per launch)
    Slots slots;
    Handle handle;
    uint8_t can;             // kWave: one wavefront per learner (is_wave_family); kCarriesQ: reads Common::qcache; kPolicyW: a Gibbs policy over weights of its
};                           // own, theta in Z; kVCritic: a state-value critic next to the actor; kLstd: the value function is the f64 least-squares state;
                             // kBatchLstd: ... of the batch agents (A, b, z, singular_solves: get/set_lstd_batch_state, not get/set_lstd_state)
// The depths.  Every launch of a register-resident loop loads and stores every learner's weights (60.7 MB at 65 536 MountainCar learners: ~11 us; the
// trace / GreedyGQ / TD ones two matrices) and pays a launch-to-launch gap around its arithmetic (0.77 us per batch-step): 1 024 steps per launch instead
// of 256 is worth +7 % (8.3e10 -> 8.9e10 env-steps/s).  Round 3, under the driver's invocation (20-step calls, coalesced): 1 024 -> 8.96e10,
// 2 048 -> 9.06e10, 4 096 -> 9.12e10, 8 192 -> 9.17e10 env-steps/s; 4 096 is a 2.9 ms launch at 65 536 learners.  The memory-resident and wave-family loops keep 256 (their steps are 15-150x longer).  RecursiveLSTD / iLSTD (and
// the iLSTD ActorCritic, the same f64 step with the actor's f32 work beside it): O(F^2) f64 per learner-step, 0.76 / 1.03 ms per batch-step at 262 144
// MountainCar order-5 learners -- 32 keep a launch in the tens of milliseconds there.  HIVTreatment: one batch-step is 1 000 f64 RK4
// sub-steps per learner, ~1 ms at 65 536 learners -- 16 keep a launch in the tens of milliseconds.  GradientMC starts from TdReg's 4 096: at 65 536
// MountainCar order-3 learners (cap 1 000) the median of seven 8 192-step regions is 1.887 / 1.890 / 1.800 us per batch-step at 1 024 / 4 096 /
// 16 384 steps per launch, inside the regions' own drift (1.14 -> 2.13 us as the learners' episodes fall out of step; profiles/gmc_rate.md).
// CliffWalk's two loops (train_table.hip): k_table_train_lds stages 960 B per learner each way around a launch, k_table_train_mem gathers every row from
// memory.  Measured at 65 536 learners (QLearning, EpsilonGreedy; profiles/cliff_walk_rate.md), us per batch-step: the LDS loop 2.94 / 1.41 / 1.32 at
// 16 / 256 / 4 096 batch-steps per launch, the memory loop 8.00 / 2.91 / 2.52 at 1 / 16 / 256.  kTableDepth: the fastest LDS depth measured.
// kTableMemBelow: launches of FEWER batch-steps take the memory loop -- the curves (1.32 + 26 / d against 2.52 + 5.5 / d) cross at d = 17, and at 16 the
// two medians are 1.2 % apart, inside the memory loop's own range
constexpr int kTableDepth = 4096;
constexpr int kTableMemBelow = 16;
constexpr FamilyRow kFamily[] = {
    {AgentFamily::SharedDense, "k_shared_step", 256, Slots::Block, Handle::Model, 0},
    {AgentFamily::SharedTile, "k_shared_ca", 256, Slots::Block, Handle::Model, 0},
    {AgentFamily::SharedSparseLambda, "k_sparse_trace_scatter", 256, Slots::Learner, Handle::Agent, 0},      // (handle: rsrl_hip_handle's own branch)
    {AgentFamily::WaveAux, "k_wave_aux", 256, Slots::WaveBlock, Handle::Agent, kWave},
    {AgentFamily::TdTile, "k_td_tile", 256, Slots::Learner, Handle::Agent, 0},
    {AgentFamily::TdGeneric, "k_td_mem", 256, Slots::Block, Handle::Agent, 0},
    {AgentFamily::TdReg, "k_train_td", 4096, Slots::Block, Handle::Agent, 0},
    {AgentFamily::WaveQSigma, "k_wave_qsigma", 256, Slots::WaveBlock, Handle::Agent, kWave},
    {AgentFamily::QSigmaReg, "k_train_qsigma", 256, Slots::Block, Handle::Agent, 0},
    {AgentFamily::QSigmaGeneric, "k_train_qsigma", 256, Slots::Block, Handle::Agent, 0},
    {AgentFamily::GqReg, "k_train_gq", 4096, Slots::Block, Handle::Agent, 0},
    {AgentFamily::GqGeneric, "k_train_gq_mem", 256, Slots::Block, Handle::Agent, 0},
    {AgentFamily::LambdaTile, "k_lambda_tile", 256, Slots::Learner, Handle::Agent, 0},
    {AgentFamily::WaveLambda, "k_wave_lambda", 256, Slots::WaveBlock, Handle::Agent, kWave},
    {AgentFamily::LambdaGeneric, "k_train_lambda_mem", 256, Slots::Block64, Handle::Agent, 0},
    {AgentFamily::LambdaReg, "k_train_lambda", 4096, Slots::Block, Handle::Agent, 0},
    {AgentFamily::WaveControl, "k_train_wave", 256, Slots::WaveBlock, Handle::Wave, kWave},
    {AgentFamily::RegStep, "k_step_reg", 4096, Slots::Block, Handle::Model, kCarriesQ},
    {AgentFamily::RegFused, "k_train_reg", 4096, Slots::Block, Handle::Model, kCarriesQ},
    {AgentFamily::Generic, "k_train_mem", 256, Slots::Block, Handle::Model, 0},
    {AgentFamily::Hiv, "k_hiv_train", 16, Slots::Block, Handle::Agent, 0},
    {AgentFamily::AcReg, "k_train_ac", 4096, Slots::Block, Handle::Agent, kPolicyW},
    {AgentFamily::TdAcReg, "k_train_tdac", 4096, Slots::Block, Handle::Agent, kPolicyW | kVCritic},
    {AgentFamily::ReinforceReg, "k_train_reinforce", 4096, Slots::Block, Handle::Agent, kPolicyW},      // (handle: refused, whole batches only)
    {AgentFamily::LstdReg, "k_train_lstd", 32, Slots::LstdGroup, Handle::Agent, kLstd},
    {AgentFamily::TdAcLstdReg, "k_train_tdac_lstd", 32, Slots::LstdGroup, Handle::Agent, kPolicyW | kVCritic | kLstd},
    {AgentFamily::GmcReg, "k_train_gmc", 4096, Slots::Block, Handle::Agent, 0},      // (handle: refused, whole trajectories only)
    {AgentFamily::LstdBatchReg, "k_train_lstd_batch", 256, Slots::LstdGroup, Handle::Agent, kLstd | kBatchLstd},      // (handle: refused, whole batches only)
    {AgentFamily::TdAcBetaReg, "k_train_tdac_beta", 32, Slots::LstdGroup, Handle::Agent, kPolicyW | kVCritic | kLstd},      // (handle: rsrl_hip_handle_f32)
    {AgentFamily::NacBetaReg, "k_train_nac_beta", 256, Slots::Block, Handle::Agent, kPolicyW},      // (handle: rsrl_hip_handle_f32; a step is a long scalar chain: 256 as the memory-resident loops)
    {AgentFamily::GtdReg, "k_train_gtd", 4096, Slots::Block, Handle::Agent, 0},      // (4 096: TdReg's depth, taken over and not measured)
    {AgentFamily::NacGaussReg, "k_train_nac_gauss", 256, Slots::Block, Handle::Agent, kPolicyW},      // (handle: rsrl_hip_handle_f32; NacBetaReg's depth, taken over)
    {AgentFamily::CaclaGaussReg, "k_train_cacla", 4096, Slots::Block, Handle::Agent, kPolicyW | kVCritic},      // (handle: rsrl_hip_handle_f32; measured at 65 536 order-3
                                                                                                               // learners: 0.984 / 0.961 / 0.952 us per batch-step at 256 / 1 024 / 4 096 steps per launch, profiles/cacla_rate.md)
    {AgentFamily::TdAcGaussReg, "k_train_tdac_cont", 4096, Slots::Block, Handle::Agent, kPolicyW | kVCritic},      // (handle: rsrl_hip_handle_f32; measured at 65 536 order-3 learners: 1.02 / 1.00 /
                                                                                                                   // 0.99 us per batch-step at 256 / 1 024 / 4 096 steps per launch, profiles/tdac_cont_rate.md)
    {AgentFamily::TdAcBetaTdReg, "k_train_tdac_cont", 4096, Slots::Block, Handle::Agent, kPolicyW | kVCritic},     // (handle: rsrl_hip_handle_f32; 3.18 / 3.14 / 3.12 us at the same depths: the
                                                                                                                   // Beta sampler's scalar chain dominates, the depth is CaclaGaussReg's all the same)
    {AgentFamily::GibbsNacReg, "k_train_gibbs_nac", 4096, Slots::Block, Handle::Agent, kPolicyW},      // (measured at 65 536 order-3 learners: 1.75 / 1.72 / 1.70 us per batch-step at
                                                                                                       // 256 / 1 024 / 4 096 steps per launch, k_train_ac 1.66 in the same process: profiles/gibbs_nac_rate.md)
    {AgentFamily::CliffTable, "k_table_train_lds", kTableDepth, Slots::Block64, Handle::Agent, 0},      // (one wave per block; the depth and the switch to k_table_train_mem:
                                                                                                        // kTableDepth / kTableMemBelow above, profiles/cliff_walk_rate.md)
};
constexpr bool family_rows_in_order() {
    for (size_t i = 0; i < sizeof(kFamily) / sizeof(kFamily[0]); ++i) if ((size_t)kFamily[i].family != i) return false;
    return true;
}
static_assert(sizeof(kFamily) / sizeof(kFamily[0]) == kAgentFamilies && family_rows_in_order(), "kFamily: one row per AgentFamily value, in the enum's order");
static inline bool is_wave_family(AgentFamily f) { return kFamily[(size_t)f].can & kWave; }

// the environment switches, read once when the ctx is created (abi_ctx.hip read_switches)
struct Switches {
    bool no_graph = false;            // RSRL_NO_GRAPH: plain launches instead of captured step graphs
    bool no_persist = false;          // RSRL_NO_PERSIST: shared dense W steps one launch per batch-step instead of the persistent kernel
    bool no_trait_defer = false;      // RSRL_NO_TRAIT_DEFER: the trait-granular loop launches one kernel per call
    bool k1_feature_major = false;    // RSRL_K1_FEATURE_MAJOR: the single-step kernel keeps the feature-major layout
    int k1_quad = -1;                 // RSRL_K1_QUAD: 0 / 1 forces one / four lanes per learner, -1 = by size
    int sparse_chunk = 0;             // RSRL_SPARSE_CHUNK: learners per block of the sparse-trace scatter (0 = one block per CU)
    long peer_timeout_ms = 0;         // RSRL_PEER_TIMEOUT_MS (0 = unset)
    bool no_wave_pk = false;          // RSRL_WAVE_PK=0: bf16 ctxs of the order-7 wave family on the fp32-register kernel k_train_wave
    bool no_reg_producer = false;     // RSRL_REG_PRODUCER=0: the fused loop keeps generating its own draws (k_train_reg instead of pw::k_train_reg)
    int table_mem = -1;               // RSRL_TABLE_MEM: 1 forces CliffWalk's memory loop (k_table_train_mem), 0 forbids it, -1 = by launch depth (kTableMemBelow)
};

struct rsrl_hip_ctx {
    rsrl_hip_config cfg{};
    AgentFamily family = AgentFamily::Generic;
    const char* train_kernel = "";   // the family's driver-loop kernel, what rsrl_hip_timing_read names after a train launch
    Switches sw;
    int D = 0, A = 0, F = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    float* state = nullptr; int32_t* action = nullptr; uint32_t* ep_step = nullptr;
    float* action_f = nullptr;       // a continuous domain's pending actions f32[N] (ContinuousMountainCar; `action` is then allocated and never read)
    int Ap = 0;                      // columns of the policy's own weights (rsrl_hip_n_policy_outputs): A for the Gibbs actors, 2 for Beta, 0 when the policy reads Q
    float* W = nullptr; float* dW = nullptr;
    int Aw = 0;                      // columns of the weight matrix: A (control) or 1 (prediction: ScalarLFA)
    int Fw = 0;                      // rows of the weight matrix (rsrl_hip_n_weight_rows): F, or NAC's 3F / the Gibbs NAC's (A+1) F (the critic's basis is SCB)
    long long* dW_rep = nullptr; int n_rep = 1;  // shared tile coding: n_rep copies of the fixed-point (64-bit) delta table
    long long* sh_tab = nullptr;     // shared-W dense basis: 3 sets x kTabRep copies of the fixed-point delta table (models.hpp DeltaTab)
    long long* h_fx = nullptr;       // shared W: fixed-point delta table of rsrl_hip_handle (one entry per weight)
    bool tile_slice = false;         // shared tile coding: one tiling's slice (twice, as 64-bit words) fits LDS
    uint16_t* sc_keys = nullptr;     // shared tile coding, separate scatter kernel: slice-relative entries [T][N]
    float* sc_terms = nullptr;       //   and terms lr*e [N] handed from the step kernel to k_tile_scatter
    uint64_t sh_tab_t = 0;           // batch-step counter the table rotation is in phase with (the end of the last shared train call)
    float* W2 = nullptr;             // shared-W dense basis: second weight buffer (k_shared_step reads one, block 0 writes the other)
    int sh_par = 0;                  // which W buffer holds the current weights (0 = W)
    unsigned sh_rows = 0;            // rows per buffer = blocks of k_shared_step
    float* qcache = nullptr;         // [A][N]: Q(s,.) carried between train launches (register family)
    float* qs_buf = nullptr; uint32_t* qs_head = nullptr; uint32_t* qs_len = nullptr;     // QSigma: per-learner n-step backups
    float* eps = nullptr;            // [N] per-learner EpsilonGreedy.epsilon (config.epsilon_decay != 1), else null
    // lambda agents over ONE shared tile table: every learner's sparse trace + the step's mailbox (kernels_sparse_lambda.hpp)
    uint16_t* sp_keys = nullptr; float* sp_vals = nullptr; uint32_t* sp_len = nullptr;    // sparse traces: [N][kSparseCap] slice-relative keys (16 bit) and values, lengths [N][n_tilings]
    bool sp_lds = false;             //   one tiling's slice of the delta table fits LDS (k_sparse_trace_scatter)
    float* Z = nullptr;              // auxiliary matrix f32[A][F][N]: eligibility traces (lambda agents) / fa_td weights (GreedyGQ; GTD2's fa_w, TDC's td_est) / the actor's theta (ActorCritic)
                                     // -- of W's shape, except TdAcReg's / TdAcLstdReg's theta: A columns against W's one (aux_cols)
    float* Zb = nullptr;             // REINFORCE only: the behaviour snapshot theta_b f32[A][F][N] (theta when the open episode began)
    float* ret_g = nullptr;          //   and the open episode's running return g f32[N]
    double* hiv_y = nullptr;         // HIVTreatment only: every learner's hidden state f64[6][N] (`state` holds its observation)
    double* lstd_theta = nullptr;    // RecursiveLSTD / iLSTD / the iLSTD ActorCritic only: theta f64[N][F], the matrix (C / A) f64[N][F][F], iLSTD's mu f64[N][F] (learner-major)
    double* lstd_mat = nullptr;
    double* lstd_mu = nullptr;       //   (LSTD / LSTDLambda: A in lstd_mat, b in lstd_mu)
    double* lstd_z = nullptr;        // LSTDLambda: the trace z f64[N][F]; LambdaLSPE: (delta, rows) f64[N][2] (lstd_z_per_learner)
    uint32_t* lstd_sing = nullptr;   // LSTD / LSTDLambda / LambdaLSPE only: u32[N], the solves abandoned on a zero pivot
    float* rec_s = nullptr;          // GradientMC, LSTD / LSTDLambda only: every learner's open episode, rows 0 .. ep_step[i]-1 of f32[max_episode_steps][D][N] (`from`) and
    float* rec_r = nullptr;          //   f32[max_episode_steps][N] (the reward)
    bool q_valid = false;            // false whenever weights / states were changed from outside the driver loop
    // ---- the trait-granular fast path (kernels_trait.hpp): register-family Fourier basis, per-learner f32 weights, learner-major layout
    float* tq_key = nullptr;         // [D][N]: the state each learner's tq_q entry belongs to (allocated iff the ctx takes the fast path)
    float* tq_q = nullptr;           // [A][N]: the hand-over's Q(key,.) -- its own buffer: qcache is the train loops' carry, which a query must not touch
    bool tq_valid = false;           // tq_q / tq_key hold the hand-over of rsrl_hip_handle (false: the keys are emptied before the next trait kernel)
    // calls of the trait-granular loop accepted but not launched yet (ctx-owned stream, device pointers, the loop's own order):
    //   stage 1 = domain_step, 2 = + handle on exactly that transition, 3 = + domain_reset with the terminal flags as its mask;
    //   policy_sample(NULL) then launches the whole batch-step as ONE kernel; anything else launches the accepted calls one by one first
    struct TraitPend { int stage = 0; const int32_t* act = nullptr; float* from = nullptr; float* to = nullptr; float* rew = nullptr;
                       uint8_t* term = nullptr; float* td = nullptr; uint64_t t_handle = 0; } tp;
    uint8_t* flags = nullptr;        // shared-W: terminal/truncated flags between phase A and phase C
    size_t w_elems = 0; size_t dw_elems = 0; size_t w_bytes = 0; size_t z_bytes = 0;      // (the auxiliary matrix Z -- traces / fa_td weights -- is f32 whatever W's storage)
    int64_t w_stride = 0;            // stride between (action, feature) rows of W
    int64_t w_ls = 1;                // stride between learners (A*F in the learner-major single-step layout, else 1)
    DevStats* d_stats = nullptr; DevStats* h_stats = nullptr;   // one slot per thread block
    size_t n_stat_slots = 0;
    bool k1_quad = false;                      // single-step streaming kernel with four lanes per learner (k_step_reg_q4)
    bool reg_producer = false;                 // RegFused: the loop whose draws come from a partner wave per SIMD (pw::k_train_reg), decided at create
    uint64_t t = 0;          // batch-steps executed (RNG counter)
    int64_t pending = 0;     // batch-steps accepted by rsrl_hip_train but not launched yet (launch coalescing, see rsrl_hip_train)
    uint64_t api_calls = 0;  // RNG counter of rsrl_hip_policy_sample
    uint64_t rollout_calls = 0;   // ... and of rsrl_hip_rollout_policy (one stream of draws per call)
    Scratch scratch[8];
    std::vector<void**> owned;       // the device buffers create_impl allocated (ctx_alloc, abi_ctx.hip), by MEMBER: rsrl_hip_destroy frees what each holds then
    // timing of train launches
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    std::vector<uint32_t> event_launches;      // batch-step launches bracketed by each event pair (a graph replay brackets many)
    size_t events_used = 0;
    // launch-bound inner loops (one batch-step per launch: the streaming kernel, the shared-W phases) replayed as a hipGraph
    uint64_t* d_t = nullptr;                   // device copy of the batch-step counter: graph nodes carry offsets to it
    DynParams* d_dyn = nullptr;                // device copy of the policy parameters graph nodes read (epsilon can change between calls)
    DynParams dyn_uploaded{};                  // what d_dyn holds
    bool dyn_valid = false;
    hipGraph_t step_graph = nullptr;
    hipGraphExec_t step_graph_exec = nullptr;
    Common step_graph_key{};                   // kernel arguments the graph was captured with
    int step_graph_kind = 0;                   // 1 = k_step_reg, 2 = shared-W batch-step
    const char* kernel_name = "";
    // multi-rank shared-W (one process per GPU): the per-batch-step exchange of the weight delta
    ncclComm_t comm = nullptr;                 // RSRL_EXCHANGE_RCCL
    int n_simd = 1024;                         // SIMDs of the device (4 per CU): launches of more waves than that co-schedule waves
    int world_size = 1, rank = 0;
    bool multi = false;                        // an exchange is attached (a communicator of size 1 included: same sequence)
    // RSRL_EXCHANGE_PEER: one-hop peer-write.  recv = this rank's receive buffer, granules {value bits, step tag}
    // [2 (step parity)][world][dw_elems]; peers[r] = rank r's receive buffer mapped into this process (hipIpc), own included
    uint2* peer_recv = nullptr; size_t peer_recv_bytes = 0; int peer_world = 0;
    std::vector<void*> peer_ptrs; std::vector<char> peer_opened;
    uint2** d_peer_ptrs = nullptr;             // device copy of peer_ptrs
    uint32_t* d_peer_err = nullptr;            // set by a block / rank that waited too long for a peer (sticky; shared-W ctxs only)
    uint64_t peer_seq = 0;                     // exchanges performed on peer_recv so far: parity and tags follow it (Common::xdelta)
    uint64_t peer_timeout = 400000000ull;      // bound of every in-kernel wait, ticks of the 100 MHz wall clock (RSRL_PEER_TIMEOUT_MS, default 4000)
    size_t peer_old_bytes = 0;                 // peer_recv = [granules of the per-step exchange kernels | hop-2 buffer of the persistent kernel]
    // persistent shared-W kernel (kernels_persist.hpp): hop-1 buffer A, hop-2 buffer B (own; inside peer_recv in peer mode)
    unsigned long long* px_A = nullptr; unsigned long long* px_B = nullptr; bool px_B_owned = false;
    unsigned long long** d_px_Bptrs = nullptr; // device array [world] of every rank's hop-2 buffer
    uint64_t px_seq = 0;                       // batch-steps exchanged through px_A / px_B so far (tags and parity)
    int n_cu = 256;
    // ---- co-residency of the persistent kernel (every block of the grid -- and of every peer rank -- must be resident at once)
    int persist_occ = -1;                      // blocks of k_shared_persist one CU admits (occupancy query; -1 = not asked yet, 0 = none)
    bool group_persist = false;                // PEER group: the COLLECTIVE decision of rsrl_hip_peer_connect (every rank takes the same path)
    int peer_share = 1;                        // ranks of this ctx's group on ITS device, itself included (rsrl_hip_peer_connect); caps the exchange grids
    bool coop_allowed = true;                  // no rank of this ctx's group shares (process, device) with it: a cooperative launch cannot queue behind a peer's
    bool coop_validated = false;               // one cooperative launch of this ctx's persistent grid has been accepted by the runtime
    bool persist_refused = false;              // ... or refused (single rank: the per-step path takes over for good)
    uint64_t group_token = 0;                  // identifies the peer group (same on every rank); 0 = a lone ctx
    bool st_rccl_group = false;                // member of a single-thread RCCL group of more than one rank: stepped by rsrl_hip_group_train only
};

static Common make_common(const rsrl_hip_ctx* c) {
    Common k{};
    k.n_envs = c->cfg.n_envs; k.env_offset = c->cfg.env_offset; k.seed = c->cfg.seed;
    k.pol.kind = c->cfg.policy;
    double v = c->cfg.epsilon * 16777216.0;
    k.pol.eps_thr = v <= 0.0 ? 0u : (v >= 16777216.0 ? 16777216u : (uint32_t)v);
    k.pol.eps = (float)c->cfg.epsilon; k.pol.tau = (float)c->cfg.tau;
    if (c->cfg.agent_policy < 0) { k.apol = k.pol; k.apol_same = 1; }
    else {
        k.apol.kind = c->cfg.agent_policy;
        v = c->cfg.agent_epsilon * 16777216.0;
        k.apol.eps_thr = v <= 0.0 ? 0u : (v >= 16777216.0 ? 16777216u : (uint32_t)v);
        k.apol.eps = (float)c->cfg.agent_epsilon; k.apol.tau = (float)c->cfg.agent_tau;
        k.apol_same = 0;
    }
    k.alg.kind = c->cfg.algo; k.alg.gamma = (float)c->cfg.gamma; k.alg.lr = (float)c->cfg.lr;
    k.alg.alpha = (float)c->cfg.alpha;
    k.max_episode_steps = c->cfg.max_episode_steps;
    k.state = c->state; k.action = c->action; k.ep_step = c->ep_step; k.W = c->W; k.w_stride = c->w_stride; k.w_ls = c->w_ls; k.shared = c->cfg.weight_mode == RSRL_W_SHARED ? 1 : 0;
    k.qcache = c->qcache; k.q_valid = c->q_valid ? 1 : 0;
    k.eps = c->eps; k.eps_decay = (float)c->cfg.epsilon_decay; k.eps_min = (float)c->cfg.epsilon_min;
    k.xdelta = (int64_t)c->peer_seq - (int64_t)c->t;
    return k;
}

static inline const FamilyRow& family_row(const rsrl_hip_ctx* c) { return kFamily[(size_t)c->family]; }
// the agents with a Gibbs policy over weights of their own (theta in Z): ActorCritic (both critics, TDCritic over TD(0) or iLSTD), REINFORCE (both)
static inline bool has_policy_weights(const rsrl_hip_ctx* c) { return family_row(c).can & kPolicyW; }
// the weights the POLICY side reads: the actor's preferences theta for ActorCritic (the policy is Gibbs over theta, not over Q), W otherwise.
// Policy::sample / mode / probabilities, reset's initial sample and the rollouts run the model kernels on it; the value side keeps make_common
static Common make_policy_common(const rsrl_hip_ctx* c) {
    Common k = make_common(c);
    if (has_policy_weights(c)) k.W = c->Z;      // (the model kernels take the column count from the model: A)
    return k;
}
// a state-value critic next to the actor: the weights are V's one column, theta has A
static inline bool is_v_actor_critic(const rsrl_hip_ctx* c) { return family_row(c).can & kVCritic; }
// columns of the auxiliary matrix Z: W's (Aw), except the TD / iLSTD ActorCritic's theta (A)
static inline int aux_cols(const rsrl_hip_ctx* c) { return kAlgo[c->cfg.algo].aux == Aux::Policy ? c->Ap : c->Aw; }
// a ctx whose actions are f32 values, not indices (ContinuousMountainCar): the *_f32 entry points are its own, their int32 twins ESTATE
static inline bool is_continuous(const rsrl_hip_ctx* c) { return c->cfg.domain == RSRL_CONTINUOUS_MOUNTAIN_CAR; }
// the continuous ctx's policy is the Gaussian (cont_policy.hpp), not Beta: actions any finite f32, no 2a - 1 in NAC's loop (nor in CACLA's)
static inline bool is_gaussian(const rsrl_hip_ctx* c) { return c->cfg.policy == RSRL_GAUSSIAN; }
// the Beta loops that hand the domain 2a - 1 for the agent's action a (nac_beta.rs:63; NAC and the continuous TD ActorCritic): the pending-action
// domain step and the mode rollout apply it.  (The iLSTD ActorCritic's loop, tdac_beta.rs, hands the domain the action itself)
static inline bool maps_beta_action(const rsrl_hip_ctx* c) { return !is_gaussian(c) && (is_nac(c->cfg.algo) || is_tdac_cont(c->cfg.algo)); }
#define NEEDS_INDEX_ACTIONS(c, call) do { if (is_continuous(c)) return fail(RSRL_HIP_ESTATE, "%s carries int32 action indices: this ctx's domain " \
    "(ContinuousMountainCar) has one f32 action -- use %s_f32", call, call); } while (0)
#define NEEDS_F32_ACTIONS(c, call) do { if (!is_continuous(c)) return fail(RSRL_HIP_ESTATE, "%s_f32 carries f32 actions: this ctx's domain has a finite " \
    "action set (int32 indices) -- use %s", call, call); } while (0)
// the domain whose Fourier features the ctx's are (ContinuousMountainCar: MountainCar's), for the kernels that read only features
static inline int feature_domain(const rsrl_hip_ctx* c) { return is_continuous(c) ? RSRL_MOUNTAIN_CAR : c->cfg.domain; }
// the agents whose value function is the f64 least-squares state (lstd_theta / lstd_mat / lstd_mu)
static inline bool has_lstd_state(const rsrl_hip_ctx* c) { return family_row(c).can & kLstd; }
static inline ReinforceState make_reinforce(const rsrl_hip_ctx* c) {
    ReinforceState rs;
    rs.theta = c->Z; rs.theta_b = c->Zb; rs.g = c->ret_g;
    return rs;
}

static inline GmcState make_gmc(const rsrl_hip_ctx* c) {
    GmcState gs;
    gs.rec_s = c->rec_s; gs.rec_r = c->rec_r;
    return gs;
}
static inline bool has_batch_lstd_state(const rsrl_hip_ctx* c) { return family_row(c).can & kBatchLstd; }
static inline LstdBatchState make_lstd_batch(const rsrl_hip_ctx* c) {
    LstdBatchState ls;
    ls.theta = c->lstd_theta; ls.mat = c->lstd_mat; ls.b = c->lstd_mu; ls.z = c->lstd_z; ls.sing = c->lstd_sing;
    ls.rec_s = c->rec_s; ls.rec_r = c->rec_r;
    ls.gamma = c->cfg.gamma; ls.lambda = c->cfg.lambda;
    return ls;
}
static inline LspeState make_lspe(const rsrl_hip_ctx* c) {
    LspeState ls;
    static_cast<LstdBatchState&>(ls) = make_lstd_batch(c);
    ls.alpha = c->cfg.alpha;
    return ls;
}
static inline LstdState make_lstd(const rsrl_hip_ctx* c) {
    LstdState ls;
    ls.theta = c->lstd_theta; ls.mat = c->lstd_mat; ls.mu = c->lstd_mu;
    // (the iLSTD ActorCritic: config.alpha is ActorCritic.alpha, iLSTD's alpha is the critic's rate, config.lr)
    ls.gamma = c->cfg.gamma; ls.alpha = is_tdac_lstd(c->cfg.algo) ? c->cfg.lr : c->cfg.alpha;
    ls.n_updates = kAlgo[c->cfg.algo].n_updates ? c->cfg.n_steps : 0;
    return ls;
}
static inline TdacLstdState make_tdac_lstd(const rsrl_hip_ctx* c) {
    TdacLstdState ts;
    ts.ls = make_lstd(c); ts.theta = c->Z; ts.alpha = c->cfg.alpha;
    return ts;
}

// the thread-per-learner continuous agents (kernels_cont.hpp): the policy's columns and the pending f32 actions; NAC's actor period travels beside it
static inline ContState make_cont(const rsrl_hip_ctx* c) {
    ContState cs;
    cs.pol = c->Z; cs.action = c->action_f;
    return cs;
}
// (RSRL_GIBBS_NAC's too)
static inline uint32_t nac_period(const rsrl_hip_ctx* c) { return (uint32_t)c->cfg.n_steps; }
static inline ContPolicy cont_policy(const rsrl_hip_ctx* c) { return c->cfg.policy == RSRL_GAUSSIAN ? ContPolicy::Gaussian : ContPolicy::Beta; }

static inline TdacBetaState make_tdac_beta(const rsrl_hip_ctx* c) {
    TdacBetaState ts;
    ts.ls = make_lstd(c); ts.w = c->Z; ts.alpha = c->cfg.alpha; ts.action = c->action_f;
    return ts;
}

static LambdaParams make_lambda(const rsrl_hip_ctx* c) {
    LambdaParams lp{};
    lp.Z = c->Z;
    double rate = c->cfg.gamma * c->cfg.lambda;
    if (c->cfg.trace == RSRL_TRACE_DUTCH) rate *= (1.0 - c->cfg.alpha);       // traces.rs:233-239
    lp.rate = (float)rate; lp.alpha = (float)c->cfg.alpha; lp.trace = c->cfg.trace;
    return lp;
}

// GTD2 / TDC: the second weight column and its rate (theta travels as k.W, lr and gamma in k.alg)
static inline GtdState make_gtd(const rsrl_hip_ctx* c) {
    GtdState gs;
    gs.w = c->Z; gs.lr_td = (float)c->cfg.lr_td;
    return gs;
}

static GqParams make_gq(const rsrl_hip_ctx* c) {
    GqParams gp{};
    gp.V = c->Z; gp.lr_td = (float)c->cfg.lr_td;
    return gp;
}

static QsParams make_qs(const rsrl_hip_ctx* c) {
    QsParams qp{};
    qp.buf = c->qs_buf; qp.head = c->qs_head; qp.len = c->qs_len; qp.n_steps = c->cfg.n_steps;
    qp.sigma = (float)c->cfg.sigma; qp.alpha = (float)c->cfg.alpha;
    return qp;
}

static TdParams make_td(const rsrl_hip_ctx* c) {
    TdParams tp{};
    tp.Z = c->Z;
    double rate = c->cfg.gamma * c->cfg.lambda;
    if (c->cfg.trace == RSRL_TRACE_DUTCH) rate *= (1.0 - c->cfg.alpha);
    tp.rate = (float)rate; tp.trace = c->cfg.trace;
    return tp;
}

// SARSALambda / QLambda over one shared tile-coded table: per-learner SPARSE traces (kernels_sparse_lambda.hpp)
static inline bool is_sparse_lambda(const rsrl_hip_config& cfg) {
    return is_lambda(cfg.algo) && cfg.basis == RSRL_TILE_CODING && cfg.weight_mode == RSRL_W_SHARED;
}
// GreedyGQ / TD / TDLambda on the order-7 wave family (kernels_wave_aux.hpp)
static inline bool is_wave_aux_algo(int algo) { return algo == RSRL_GREEDY_GQ || is_pred(algo); }
static WaveAuxParams make_wave_aux(const rsrl_hip_ctx* c) {
    WaveAuxParams ap{};
    ap.mode = c->cfg.algo == RSRL_GREEDY_GQ ? WAUX_GQ : (c->cfg.algo == RSRL_TD ? WAUX_TD : WAUX_TDL);
    ap.aux = c->Z; ap.lr_td = (float)c->cfg.lr_td;
    const TdParams tp = make_td(c);
    ap.rate = tp.rate; ap.trace = tp.trace;
    return ap;
}
template <int DM, class WT> struct WaveTag { static constexpr int domain = DM; using wt = WT; };
template <class Fn>
static bool for_wave(const rsrl_hip_ctx* c, Fn&& fn) {
    const bool bf = c->cfg.weight_dtype == RSRL_W_BF16;
    if (c->cfg.domain == RSRL_CART_POLE) { if (bf) fn(WaveTag<1, bf16_t>{}); else fn(WaveTag<1, float>{}); return true; }
    if (c->cfg.domain == RSRL_ACROBOT) { if (bf) fn(WaveTag<2, bf16_t>{}); else fn(WaveTag<2, float>{}); return true; }
    return false;
}

// resolution of the fixed-point delta tables of shared tile coding: 2^(floor(log2 |lr|) - 28), the same bits the kernel derives
static inline float tile_lsb(float lr) {
    uint32_t u; memcpy(&u, &lr, 4);
    const uint32_t eb = (u >> 23) & 0xffu;
    const uint32_t ex = (eb < 30u ? 30u : eb) - 28u;
    const uint32_t v = ex << 23; float f; memcpy(&f, &v, 4);
    return f;
}
constexpr int kSharedBlock = 512;    // learners per block of k_shared_step: 256 blocks = one per CU for a 131 072-env shard

// ---- (basis, domain, parameter) -> Model type: model_list.hpp
static bool model_supported(const rsrl_hip_config& cfg) {
    return is_reg_fourier(cfg) || for_mem_model(cfg, [](auto) {});
}
// calls fn(tag) with tag::type the ctx's model, first match; false if none matches
template <class Fn>
static bool for_model(const rsrl_hip_ctx* c, Fn&& fn) {
    return (c->cfg.basis == RSRL_FOURIER && for_reg_fourier(c->cfg.domain, c->cfg.order, fn)) || for_mem_model(c->cfg, fn);
}
static BasisGeom make_geom(const rsrl_hip_ctx* c) {
    return BasisGeom{c->F, c->cfg.basis == RSRL_FOURIER ? c->cfg.order : c->cfg.tiles_per_dim};
}
// wave family (one wavefront per learner): Fourier order 7 on the 4-D domains, f32 or bf16 weights
static bool is_wave(const rsrl_hip_config& cfg) {
    return cfg.basis == RSRL_FOURIER && cfg.order == kWaveOrder && (cfg.domain == RSRL_CART_POLE || cfg.domain == RSRL_ACROBOT);
}
static inline unsigned wave_grid_for(int64_t items) { return (unsigned)((items + (kBlock / 64) - 1) / (kBlock / 64)); }
// the HIVTreatment entry point of a multi-rank call: per-learner weights only, nothing to exchange
#define HIV_NO_EXCHANGE(c) do { if ((c)->cfg.domain == RSRL_HIV_TREATMENT) return fail(RSRL_HIP_EINVAL, "HIVTreatment supports per-learner weights only: " \
    "no communicator, peer exchange or group (shard by env_offset instead)"); \
    if ((c)->cfg.domain == RSRL_CLIFF_WALK) return fail(RSRL_HIP_EINVAL, "CliffWalk supports per-learner tables only: " \
    "no communicator, peer exchange or group (shard by env_offset instead)"); } while (0)
#define NO_MODEL(c) fail(RSRL_HIP_EINVAL, "no kernel for basis %d domain %d order %d tilings %d", (c)->cfg.basis, (c)->cfg.domain, (c)->cfg.order, (c)->cfg.n_tilings)

#define TRY(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)
// ---- host / device array arguments: the call frame ------------------------------------------------------------------------------------
// THE rule (include/rsrl_hip.h, "Conventions"): a device or managed pointer is used in place and the call is asynchronous; a host array is staged
// through a scratch buffer of the ctx, and the call returns once host inputs have been read and host outputs have landed.  So a call synchronises
// exactly when at least one non-null array it registered is host memory -- that is finish(), and no entry point says it again.
static bool is_device_ptr(const void* p) {
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}
static int scratch_reserve(rsrl_hip_ctx* c, int slot, size_t bytes) {
    Scratch& s = c->scratch[slot];
    if (s.cap >= bytes) return RSRL_HIP_OK;
    if (s.p) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(s.p)); s.p = nullptr; s.cap = 0; }
    HIP_TRY(hipMalloc(&s.p, bytes));
    s.cap = bytes;
    return RSRL_HIP_OK;
}
// One CallFrame per entry-point call.  in() / out() register the call's arrays: null gives null, a device pointer itself, a host array the next
// scratch slot (0 .. 6 in registration order; slot 7 belongs to the two direct users of scratch_reserve, the checksum of abi_weights.hip and
// set_states' device validation in abi_ctx.hip).  finish() copies the staged outputs back in registration order and synchronises once, by the rule
// above; an error return before it does not synchronise.  The runtime is asked about a pointer once per call: host() / device() remember the
// answer, for the validators and the deferral tests that need it before anything is staged.
// A helper that runs inside an entry point either OWNS the call's frame (qop, beta_op, staged_rw) or is handed device pointers only
// (launch_trait_handle; qop under sample_emit: a frame that sees device pointers alone takes no slot and never synchronises) -- two frames that
// both staged would hand out the same slots.
struct CallFrame {
    rsrl_hip_ctx* const c;
    explicit CallFrame(rsrl_hip_ctx* ctx) : c(ctx) {}
    bool host(const void* p) {           // a non-null array in host memory
        if (!p) return false;
        for (int i = 0; i < n_seen; ++i) if (seen[i].p == p) return seen[i].host;
        const bool h = !is_device_ptr(p);
        if (n_seen < kArrays) seen[n_seen++] = {p, h};      // (no call has more than 8 arrays; a ninth would be asked about again)
        return h;
    }
    bool device(const void* p) { return p && !host(p); }
    bool all_device() const { return !any_host; }      // of the arrays registered so far
    template <class T> int in(const T* user, size_t count, const T** dev) {
        void* d = nullptr;
        TRY(place(user, count * sizeof(T), &d));
        if (d != user && count) HIP_TRY(hipMemcpyAsync(d, user, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
        *dev = (const T*)d;
        return RSRL_HIP_OK;
    }
    template <class T> int out(T* user, size_t count, T** dev) {
        void* d = nullptr;
        TRY(place(user, count * sizeof(T), &d));
        if (d != user) outs[n_out++] = {user, d, count * sizeof(T)};
        *dev = (T*)d;
        return RSRL_HIP_OK;
    }
    int finish() {
        for (int i = 0; i < n_out; ++i)
            if (outs[i].bytes) HIP_TRY(hipMemcpyAsync(outs[i].user, outs[i].dev, outs[i].bytes, hipMemcpyDeviceToHost, c->stream));
        if (any_host) HIP_TRY(hipStreamSynchronize(c->stream));
        return RSRL_HIP_OK;
    }
private:
    static constexpr int kArrays = 8, kSlots = 7;
    struct Seen { const void* p; bool host; } seen[kArrays];
    struct Out { void* user; const void* dev; size_t bytes; } outs[kSlots];
    int n_seen = 0, n_out = 0, n_slots = 0;
    bool any_host = false;
    int place(const void* user, size_t bytes, void** dev) {
        *dev = const_cast<void*>(user);
        if (!host(user)) return RSRL_HIP_OK;
        any_host = true;
        if (n_slots == kSlots) return fail(RSRL_HIP_EINVAL, "internal: a call stages more than %d host arrays", kSlots);
        TRY(scratch_reserve(c, n_slots, bytes));
        *dev = c->scratch[n_slots++].p;
        return RSRL_HIP_OK;
    }
};
// caller-supplied actions index weight columns (W[:,a]): a HOST array is validated (EINVAL, where the reference would
// panic on the out-of-range column); a DEVICE array cannot be inspected from here and is clamped by the kernels instead
static int check_host_actions(CallFrame& f, const int32_t* a, size_t n, int A) {
    if (!f.host(a)) return RSRL_HIP_OK;
    for (size_t i = 0; i < n; ++i)
        if (a[i] < 0 || a[i] >= A) return fail(RSRL_HIP_EINVAL, "action[%zu] = %d is outside [0, %d)", i, a[i], A);
    return RSRL_HIP_OK;
}
// caller-supplied f32 actions (a continuous ctx): a HOST array must hold finite values (bounded: inside ContinuousMountainCar's action bounds too); a
// DEVICE array is clamped by the kernels instead
static int check_host_actions_f32(CallFrame& f, const float* a, size_t n, bool bounded) {
    if (!f.host(a)) return RSRL_HIP_OK;
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(a[i])) return fail(RSRL_HIP_EINVAL, "action[%zu] = %g is not finite", i, (double)a[i]);
        if (bounded && !(a[i] >= -1.0f && a[i] <= 1.0f)) return fail(RSRL_HIP_EINVAL, "action[%zu] = %g is outside [-1, 1]", i, (double)a[i]);
    }
    return RSRL_HIP_OK;
}
// caller-supplied STATES: the reference's wrap! (rsrl_domains/src/macros.rs:14-24) brings an angle home by repeated +-2 pi -- a loop that does not end
// for an infinite value and practically not for a huge one (Acrobot; on the device that is a hung GPU).  A HOST array is validated (EINVAL: every
// component finite and within 1000 widths of its dimension's bounds); a DEVICE array cannot be inspected from here and is clamped into that range
// by k_clamp_states (NaN stays NaN: comparisons with it are false, nothing loops).
extern "C" __attribute__((visibility("hidden"))) void state_limits(const rsrl_hip_ctx* c, float* lo, float* hi);      // (abi_ctx.hip; internal: hidden visibility)
static int check_host_states(CallFrame& f, const float* s, size_t n_cols) {
    if (!f.host(s)) return RSRL_HIP_OK;
    const rsrl_hip_ctx* c = f.c;
    float lo[8], hi[8];
    state_limits(c, lo, hi);
    for (int d = 0; d < c->D; ++d)
        for (size_t i = 0; i < n_cols; ++i) {
            const float x = s[(size_t)d * n_cols + i];
            if (!(x >= lo[d] && x <= hi[d]))
                return fail(RSRL_HIP_EINVAL, "state[%d][%zu] = %g is not a finite value within 1000 widths of the dimension's bounds [%g, %g]", d, i, (double)x,
                            (double)lo[d], (double)hi[d]);
        }
    return RSRL_HIP_OK;
}
struct StateLimits { float lo[8], hi[8]; };
// a DEVICE array of states is validated on the device, with the host path's rule (it used to be clamped silently, and NaN passed): *bad counts the
// components that are not finite values within the limits; the caller copies the array into the ctx only when there are none
static __global__ void k_check_states(const float* __restrict__ s, int64_t n, int D, StateLimits lim, unsigned* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned cnt = 0;
    for (int d = 0; d < D; ++d) {
        const float x = s[(int64_t)d * n + i];
        cnt += (x >= lim.lo[d] && x <= lim.hi[d]) ? 0u : 1u;
    }
    if (cnt) atomicAdd(bad, cnt);
}
#define KCHECK() HIP_TRY(hipGetLastError())

#define NCCL_TRY(expr)                                                                                   \
    do {                                                                                                 \
        ncclResult_t _r = (expr);                                                                        \
        if (_r != ncclSuccess) return fail(RSRL_HIP_ERCCL, "%s failed: %s", #expr, ncclGetErrorString(_r)); \
    } while (0)
// The one exchange step of the path: sum the (F x A) f32 weight delta over the ranks so that every rank applies the
// identical update and the replicas of W stay bit-identical.  In place on c->dW, on the ctx's stream, no host
// synchronisation, capturable into the step graph.  A communicator of size 1 runs the same sequence (that is how the
// multi-rank path is exercised on a one-GPU box).  At 432 B (MountainCar Fourier(5)) this is latency-bound, not link-bound.
//   t / t_dev: the batch-step this exchange belongs to (PEER: slot parity and granule tag); t_dev != nullptr inside a graph.
// Grid of the peer-exchange kernels (grid-stride loops over the n outputs).  A rank that has its device to itself takes one block per 256 outputs, as
// before.  Ranks that SHARE a device (oversubscribed tests, several ranks per GPU) wait -- bounded -- for each other's pushes while occupying compute
// units: eight ranks x 768 waiting blocks (a 16 x 8^4 x 3 tile table) fill the device and the rank they wait for never gets a unit (found by
// tests/fuzz_ranks.py as an exchange time-out).  So the group's waiting blocks together may take at most HALF of the device's resident blocks.
static unsigned peer_grid(const rsrl_hip_ctx* c, int n) {
    const unsigned full = (unsigned)((n + 255) / 256);
    if (c->peer_share <= 1) return full;
    const unsigned resident = (unsigned)(c->n_cu > 0 ? c->n_cu : 256) * 8u;            // 256-thread blocks per device at full occupancy
    const unsigned cap = std::max(1u, resident / 2u / (unsigned)c->peer_share);
    return std::min(full, cap);
}
static int exchange_dw(rsrl_hip_ctx* c, uint64_t t, const uint64_t* t_dev, int64_t xdelta) {
    if (!c->multi) return RSRL_HIP_OK;
    const int n = (int)c->dw_elems;
    if (c->cfg.exchange == RSRL_EXCHANGE_PEER) {
        hipLaunchKernelGGL(k_peer_push, dim3(peer_grid(c, n)), dim3(256), 0, c->stream, c->dW, n, c->d_peer_ptrs, c->world_size, c->rank, t, t_dev, xdelta);
        hipLaunchKernelGGL(k_peer_reduce, dim3(peer_grid(c, n)), dim3(256), 0, c->stream, c->dW, n, c->peer_recv, c->world_size, t, t_dev, xdelta, c->d_peer_err,
                           c->peer_timeout);
        KCHECK();
        return RSRL_HIP_OK;
    }
    NCCL_TRY(ncclAllReduce(c->dW, c->dW, c->dw_elems, ncclFloat, ncclSum, c->comm, c->stream));
    return RSRL_HIP_OK;
}
// a rank that waited too long for a peer left a mark: report it at the next synchronising call
static int peer_check(rsrl_hip_ctx* c) {
    if (!c->d_peer_err) return RSRL_HIP_OK;
    uint32_t e = 0;
    HIP_TRY(hipMemcpyAsync(&e, c->d_peer_err, sizeof(e), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (e) return fail(RSRL_HIP_ERCCL, "shared-W exchange timed out: a block or rank did not deliver its weight delta (rank %d of %d); the update was not applied "
                                       "(per-step exchange: the weights are poisoned with NaN)", c->rank, c->world_size);
    return RSRL_HIP_OK;
}

int flush_pending(rsrl_hip_ctx* c);      // launch what the ctx has accepted but not launched yet (train's coalesced batch-steps, deferred trait calls)
int trait_flush(rsrl_hip_ctx* c);        // ... the deferred trait calls alone, one kernel per call
int timing_begin(rsrl_hip_ctx* c);
int timing_end(rsrl_hip_ctx* c, uint32_t launches = 1);
int trait_cache_ready(rsrl_hip_ctx* c);
static inline bool trait_fast(const rsrl_hip_ctx* c) { return c->tq_key != nullptr; }
int launch_trait_handle(rsrl_hip_ctx* c, const Common& k, const float* from, const int32_t* act, const float* rew, const float* to,
                               const uint8_t* term, int64_t M, uint64_t t, float* td);
int launch_domain_step(rsrl_hip_ctx* c, const Common& k, const int32_t* d_act, float* from, float* next, float* rew, uint8_t* term);
int launch_domain_reset(rsrl_hip_ctx* c, const Common& k, const uint8_t* d_mask);
#define FLUSH(c) TRY(flush_pending(c))

// ---- defined in one unit, used by others
// g_fx_saturations (models.hpp) is a translation-unit-local device counter: every unit whose kernels quantise has its own, rsrl_hip_fx_saturations adds them up
#define RSRL_DEFINE_FX_READER(name) \
    int name(unsigned int* n) { return hipMemcpyFromSymbol(n, HIP_SYMBOL(g_fx_saturations), sizeof(*n), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }
int fx_saturations_train(unsigned int* n);      // abi_train.hip: k_shared_step / k_shared_ca / k_shared_persist
int fx_saturations_trait(unsigned int* n);      // abi_trait.hip: k_handle on shared weights
int fx_saturations_util(unsigned int* n);       // kernels_util.hip: k_tile_scatter
int fx_saturations_launch(unsigned int* n);     // launch_shared.hip: k_sparse_trace_scatter
int train_now(rsrl_hip_ctx* c, int64_t n_steps, rsrl_hip_stats* stats_out);                                                              // abi_train.hip
int enqueue_shared_step(rsrl_hip_ctx* c, const Common& k, const BasisGeom& g, DevStats* d_stats, int do_c, uint64_t t, const uint64_t* t_dev, int xpart = 0);
int enqueue_shared_c(rsrl_hip_ctx* c, const Common& k, const BasisGeom& g, uint64_t t_last);
int exchange_table(rsrl_hip_ctx* c, uint64_t t);
bool persist_capable(rsrl_hip_ctx* c);
bool persist_ok(rsrl_hip_ctx* c);
unsigned persist_budget_shared(rsrl_hip_ctx* c);
// the kernels that read Common::qcache: the register family's one-step loops
static inline bool carries_q(const rsrl_hip_ctx* c) { return family_row(c).can & kCarriesQ; }
bool no_coalesce_switch();                                                                                                                  // abi_ctx.hip
// the per-learner families' launch, driver loop (io == nullptr: chunk batch-steps from batch-step t) or Handler::handle on io's transitions (the families
// with a handle kernel of their own; rsrl_hip_handle takes the rest to k_handle / k_wave_handle)                                            abi_train.hip
int launch_agent(rsrl_hip_ctx* c, const Common& k, const BasisGeom& g, uint64_t t, int chunk, DevStats* d_stats, const Transitions* io);
extern "C" __attribute__((visibility("hidden"))) int traces_rw(rsrl_hip_ctx* c, int64_t env_index, float* out, const float* in);                                                          // abi_weights.hip
constexpr int kStepsPerGraph = 32;       // batch-steps per captured step graph (abi_train.hip)
#define ST_RCCL_GUARD(c) do { if ((c)->st_rccl_group) return fail(RSRL_HIP_ESTATE, "this ctx is a rank of a single-thread RCCL group: its collectives must be " \
    "issued for all ranks together -- step the group with rsrl_hip_group_train (or use one thread / process per rank, or RSRL_EXCHANGE_PEER)"); } while (0)
