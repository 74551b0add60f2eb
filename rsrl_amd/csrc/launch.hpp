// launch.hpp -- launchers of the fused train kernels, one translation unit per domain so the
// (order x algo x policy) instantiations compile in parallel.
#pragma once
#include "kernels_reg.hpp"
#include "kernels_reg_q4.hpp"

namespace rsrl {

// returns false when no instantiation exists for (order, algo, policy)
bool launch_train_reg_d0(int order, int algo, int policy, dim3 grid, dim3 block, hipStream_t st,
                         const Common& k, uint64_t t, int chunk, DevStats* stats, const uint64_t* t_dev = nullptr);
bool launch_train_reg_d1(int order, int algo, int policy, dim3 grid, dim3 block, hipStream_t st,
                         const Common& k, uint64_t t, int chunk, DevStats* stats, const uint64_t* t_dev = nullptr);
bool launch_train_reg_d2(int order, int algo, int policy, dim3 grid, dim3 block, hipStream_t st,
                         const Common& k, uint64_t t, int chunk, DevStats* stats, const uint64_t* t_dev = nullptr);

// chunk == -1 selects the single-step streaming kernel (k_step_reg), -2 its learner-major form (k_step_reg_lm), -3 the learner-major
// form with four lanes per learner (k_step_reg_q4: grid = learners / 64)

// Handler::handle's M caller-supplied transitions (device arrays; td_out may be null).  The launchers below take a pointer to them: nullptr
// runs the driver loop (chunk batch-steps of the ctx's learners) instead.  Host only: the kernels take the fields as arguments of their own.
struct Transitions {
    const float* from = nullptr; const int32_t* act = nullptr; const float* rew = nullptr; const float* to = nullptr; const uint8_t* term = nullptr;
    int64_t M = 0; float* td_out = nullptr;
};
// what a launcher passes to a kernel that serves both: the transitions, or the driver loop's empty set
static inline Transitions transitions_or_none(const Transitions* io) { return io ? *io : Transitions{}; }

struct LambdaParams;
struct BasisGeom;
bool launch_lambda(int domain, int order, int algo, int policy, dim3 grid, dim3 block, hipStream_t st, const Common& k, const LambdaParams& lp,
                   uint64_t t, int chunk, DevStats* stats, const Transitions* io);
// lambda agents on tile coding, per-learner tables: one block per learner (driver loop) or per transition (handle)
bool launch_lambda_tile(int domain, int n_tilings, hipStream_t st, const Common& k, const BasisGeom& g, const LambdaParams& lp, uint64_t t, int chunk,
                        DevStats* stats, const Transitions* io);

struct TdParams;
// TD / TDLambda on tile coding: one block per learner (driver loop) or per transition (handle); V(s) of M states into out
bool launch_td_tile(int domain, int n_tilings, bool lambda, hipStream_t st, const Common& k, const BasisGeom& g, const TdParams& tp, uint64_t t, int chunk,
                    DevStats* stats, const Transitions* io);
bool launch_v_tile(int domain, int n_tilings, hipStream_t st, const Common& k, const BasisGeom& g, const float* states, int64_t M, float* out);

struct GqParams;
bool launch_gq(int domain, int order, int policy, dim3 grid, dim3 block, hipStream_t st, const Common& k, const GqParams& gp, uint64_t t, int chunk,
               DevStats* stats, const Transitions* io);

// ActorCritic (train_ac.hip, kernels_ac.hpp): theta = the actor's preferences f32[A][F][N]; critic = AC_CRITIC_ADVANTAGE / AC_CRITIC_Q.  io: handle at
// batch-step t (the critic's inner draw), else chunk batch-steps of the driver loop from t
bool launch_ac(int domain, int order, int critic, dim3 grid, dim3 block, hipStream_t st, const Common& k, float* theta, uint64_t t, int chunk,
               DevStats* stats, const Transitions* io);
// ActorCritic with the TD(0) V critic (train_tdac.hip, kernels_tdac.hpp): k.W = w f32[F][N], theta f32[A][F][N].  io: handle, else chunk
// batch-steps of the driver loop from t
bool launch_tdac(int domain, int order, dim3 grid, dim3 block, hipStream_t st, const Common& k, float* theta, uint64_t t, int chunk, DevStats* stats,
                 const Transitions* io);
// REINFORCE / BaselineREINFORCE (train_reinforce.hip, kernels_reinforce.hpp): what the kernels carry besides Common (k.W = the baseline B f32[A][F][N])
struct ReinforceState {
    float* theta = nullptr;      // f32[A][F][N]: the agent's weights (the ctx's auxiliary matrix)
    float* theta_b = nullptr;    // f32[A][F][N]: the behaviour snapshot, theta when the open episode began
    float* g = nullptr;          // f32[N]: the open episode's running return
};
// Handler<&Batch>::handle's batches (device arrays): states [T][D][N], actions / rewards [T][N], lengths [N], ret_out [T][N] (may be null)
struct ReinforceBatch {
    const float* states = nullptr; const int32_t* act = nullptr; const float* rew = nullptr; const uint32_t* len = nullptr; int64_t T = 0;
    float* ret_out = nullptr;
};
// io: handle_batch on io's batches, else chunk batch-steps of the driver loop from t
bool launch_reinforce(int domain, int order, bool baseline, dim3 grid, dim3 block, hipStream_t st, const Common& k, const ReinforceState& rs, uint64_t t,
                      int chunk, DevStats* stats, const ReinforceBatch* io);
// new episodes for the learners in mask (every learner when mask is null): theta_b <- theta, g <- 0.  FA = F * A
void launch_reinforce_restart(hipStream_t st, const ReinforceState& rs, int64_t N, int64_t FA, const uint8_t* mask);

// RecursiveLSTD / iLSTD (train_lstd.hip, kernels_lstd.hpp): every learner's exact f64 state, learner-major, and the config's f64 parameters
struct LstdState {
    double* theta = nullptr;     // f64[N][F]
    double* mat = nullptr;       // f64[N][F][F], row-major per learner: C (RecursiveLSTD) or A (iLSTD)
    double* mu = nullptr;        // f64[N][F]: iLSTD only
    double gamma = 0.0, alpha = 0.0;
    int n_updates = 0;           // iLSTD's solve rounds (config.n_steps)
};
// lanes per learner of the LSTD kernels: the power of two >= F
static inline int lstd_group_lanes(int F) { return F <= 4 ? 4 : (F <= 16 ? 16 : (F <= 32 ? 32 : 64)); }
// incremental = iLSTD.  io: handle on io's transitions (transition i is learner i's), else chunk batch-steps of the driver loop from t.  The grid is
// the launcher's own (G lanes per learner)
bool launch_lstd(int domain, int order, bool incremental, hipStream_t st, const Common& k, const LstdState& ls, uint64_t t, int chunk, DevStats* stats,
                 const Transitions* io);
// V(s_i) of learner i for M states; Random.sample of the ctx's learners at (t, blk) into out and k.action; theta <-> f32
bool launch_lstd_v(int domain, int order, hipStream_t st, const double* theta, const float* states, int64_t M, float* out);
void launch_lstd_sample(int domain, hipStream_t st, const Common& k, uint64_t t, uint32_t blk, int32_t* out);
void launch_lstd_theta_get(hipStream_t st, const double* theta, int F, int64_t i, float* w);
void launch_lstd_theta_set(hipStream_t st, double* theta, int F, int64_t first, int64_t count, const float* w);
// every learner's F x F block of mat (n = N * F * F doubles) := diag * I
void launch_lstd_fill_eye(hipStream_t st, double* mat, int64_t n, int F, double diag);
// ActorCritic::tdac with the iLSTD critic (train_tdac_lstd.hip, kernels_tdac_lstd.hpp): iLSTD's f64 state (ls.alpha = iLSTD's alpha, config.lr), the
// actor's theta f32[A][F][N] and ActorCritic.alpha in f64.  io: handle, else chunk batch-steps of the driver loop from t; the grid is the launcher's own
struct TdacLstdState {
    LstdState ls;
    float* theta = nullptr;
    double alpha = 0.0;
};
bool launch_tdac_lstd(int domain, int order, hipStream_t st, const Common& k, const TdacLstdState& ts, uint64_t t, int chunk, DevStats* stats,
                      const Transitions* io);

bool launch_td(int domain, int order, bool lambda, dim3 grid, dim3 block, hipStream_t st, const Common& k, const TdParams& tp, uint64_t t, int chunk,
               DevStats* stats, const Transitions* io);
bool launch_v_evaluate(int domain, int order, dim3 grid, dim3 block, hipStream_t st, const Common& k, const float* states, int64_t Mn, float* out);
bool launch_reset_td(int domain, dim3 grid, dim3 block, hipStream_t st, const Common& k, uint64_t t);

struct QsParams;
bool launch_qsigma(int domain, int order, dim3 grid, dim3 block, hipStream_t st, const Common& k, const QsParams& qp, const BasisGeom& g, uint64_t t,
                   int chunk, DevStats* stats, const Transitions* io);

// the same agents on the models without a register-family kernel (tile coding, generic Fourier orders); false if the configuration
// has a register-family kernel (use the launchers above) or none at all
}  // namespace rsrl
#include "../../include/rsrl_hip.h"
namespace rsrl {
bool launch_gq_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const GqParams& gp, const BasisGeom& g, uint64_t t,
                     int chunk, DevStats* stats, const Transitions* io);
bool launch_lambda_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const LambdaParams& lp, const BasisGeom& g,
                         uint64_t t, int chunk, DevStats* stats, const Transitions* io);
bool launch_td_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const TdParams& tp, const BasisGeom& g, bool lambda,
                     uint64_t t, int chunk, DevStats* stats, const Transitions* io);
bool launch_v_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const BasisGeom& g, const float* states, int64_t M,
                    float* out);
bool launch_qsigma_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const QsParams& qp, const BasisGeom& g, uint64_t t,
                         int chunk, DevStats* stats, const Transitions* io);

// HIVTreatment (train_hiv.hip, kernels_hiv.hpp): one-step agents, per-learner f32 weights, Fourier orders 1-3.  Y = the hidden states f64[6][N]
struct TrajOut;
struct RolloutPolicy;
void launch_hiv_reset(hipStream_t st, const Common& k, const BasisGeom& g, double* Y, uint64_t t);
void launch_hiv_domain_step(hipStream_t st, const Common& k, double* Y, const int32_t* act, float* from, float* next, float* rew, uint8_t* term);
void launch_hiv_domain_reset(hipStream_t st, const Common& k, double* Y, const uint8_t* mask);
// state = emit(Y); from_obs: first Y = 10^state
void launch_hiv_emit(hipStream_t st, double* Y, float* state, int64_t N, bool from_obs);
void launch_hiv_qop(hipStream_t st, const Common& k, const BasisGeom& g, int op, const float* states, int64_t Mn, uint64_t call, float* fout, int32_t* iout,
                    const float* fin, const int32_t* iin);
void launch_hiv_handle(hipStream_t st, const Common& k, const BasisGeom& g, const Transitions& io, uint64_t t);
void launch_hiv_train(hipStream_t st, const Common& k, const BasisGeom& g, double* Y, uint64_t t, int chunk, DevStats* stats);
void launch_hiv_rollout(hipStream_t st, const Common& k, const BasisGeom& g, int64_t step_limit, uint32_t* n_states, float* total, int64_t Mn, const TrajOut& tr,
                        const RolloutPolicy& rp);

#define RSRL_TRAIN_CASE(DM, OR, AL, PO)                                                                     \
    if (order == OR && algo == AL && policy == PO) {                                                        \
        if (chunk == -3) {                                                                                  \
            if constexpr (FourierReg<DM, OR>::F % 4 == 0 && Domain<DM>::A <= 3)                               \
                hipLaunchKernelGGL((k_step_reg_q4<DM, OR, AL, PO>), dim3((unsigned)((k.n_envs + 63) / 64)), block, 0, st, k, t, stats, t_dev); \
            else return false;                                                                              \
        } else if (chunk == -2) {                                                                           \
            if constexpr ((Domain<DM>::A * FourierReg<DM, OR>::F) % 4 == 0 && FourierReg<DM, OR>::F % 4 == 0)     \
                hipLaunchKernelGGL((k_step_reg_lm<DM, OR, AL, PO>), grid, block, 0, st, k, t, stats, t_dev);       \
            else return false;                                                                              \
        } else if (chunk == -1)                                                                             \
            hipLaunchKernelGGL((k_step_reg<DM, OR, AL, PO>), grid, block, 0, st, k, t, stats, t_dev);              \
        else if (PO == POL_EGREEDY && k.eps) {      /* per-learner epsilon schedule: an instantiation of its own (EpsilonGreedy only) */ \
            if constexpr (PO == POL_EGREEDY) hipLaunchKernelGGL((k_train_reg<DM, OR, AL, PO, true>), grid, block, 0, st, k, t, chunk, stats); \
        } else                                                                                              \
            hipLaunchKernelGGL((k_train_reg<DM, OR, AL, PO>), grid, block, 0, st, k, t, chunk, stats);            \
        return true;                                                                                        \
    }
#define RSRL_TRAIN_POLICIES(DM, OR, AL) \
    RSRL_TRAIN_CASE(DM, OR, AL, 0) RSRL_TRAIN_CASE(DM, OR, AL, 1) RSRL_TRAIN_CASE(DM, OR, AL, 2) RSRL_TRAIN_CASE(DM, OR, AL, 3)
#define RSRL_TRAIN_ALGOS(DM, OR) RSRL_TRAIN_POLICIES(DM, OR, 0) RSRL_TRAIN_POLICIES(DM, OR, 1) RSRL_TRAIN_POLICIES(DM, OR, 2) RSRL_TRAIN_POLICIES(DM, OR, 5)

}  // namespace rsrl
