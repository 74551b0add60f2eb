// train_tdac_beta.hip -- ActorCritic::tdac with the iLSTD critic and the Beta policy on ContinuousMountainCar (kernels_tdac_beta.hpp), Fourier orders
// 1-5: the fused driver loop, Handler::handle, the policy side on explicit states (sample, mode, params, pdf), reset's initial sample, the mode
// rollout and the domain's f32 transition.  The value side runs train_lstd.hip's V kernel on the f64 theta (the features are MountainCar's).  Kept
// in a translation unit of its own so that no other kernel's machine code moves.
#include "launch.hpp"
#include "kernels_tdac_beta.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_tdac_beta(int order, hipStream_t st, const Common& k, const TdacBetaState& ts, uint64_t t, int chunk, DevStats* stats, const TransitionsF32* io) {
#define X(OR)                                                                                                                                   \
    if (order == OR) {                                                                                                                          \
        const dim3 grid = lstd_grid(io ? io->M : k.n_envs, LstdGroup<FourierReg<kCmc, OR>::F>::G), block(kBlock);                               \
        if (io) hipLaunchKernelGGL((k_handle_tdac_beta<OR>), grid, block, 0, st, k, ts, io->from, io->act, io->rew, io->to, io->term, io->M, io->td_out); \
        else hipLaunchKernelGGL((k_train_tdac_beta<OR>), grid, block, 0, st, k, ts, t, chunk, stats);                                          \
        return true;                                                                                                                            \
    }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

static inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

bool launch_beta_policy(int order, hipStream_t st, const Common& k, const float* w, int op, const float* states, int64_t M, uint64_t t, uint32_t purpose,
                        const float* act_in, float* out0, float* out1, float* keep) {
#define X(OR) if (order == OR) { hipLaunchKernelGGL((k_beta_policy<OR>), grid1(M), dim3(kBlock), 0, st, k, w, op, states, M, t, purpose, act_in, out0, out1, keep); return true; }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

bool launch_beta_reset(int order, hipStream_t st, const Common& k, const float* w, uint64_t t, float* action) {
#define X(OR) if (order == OR) { hipLaunchKernelGGL((k_beta_reset<OR>), grid1(k.n_envs), dim3(kBlock), 0, st, k, w, t, action); return true; }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

bool launch_beta_rollout_mode(int order, hipStream_t st, const Common& k, const float* w, int64_t step_limit, uint32_t* n_states, float* total) {
#define X(OR) if (order == OR) { hipLaunchKernelGGL((k_beta_rollout_mode<OR>), grid1(k.n_envs), dim3(kBlock), 0, st, k, w, step_limit, n_states, total); return true; }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

void launch_cmc_domain_step(hipStream_t st, const Common& k, const float* act, const float* pending, float* from, float* next, float* rew, uint8_t* term) {
    hipLaunchKernelGGL(k_cmc_domain_step, grid1(k.n_envs), dim3(kBlock), 0, st, k, act, pending, from, next, rew, term);
}
void launch_cmc_clamp_actions(hipStream_t st, float* a, int64_t n) { hipLaunchKernelGGL(k_cmc_clamp_actions, grid1(n), dim3(kBlock), 0, st, a, n); }

}  // namespace rsrl
