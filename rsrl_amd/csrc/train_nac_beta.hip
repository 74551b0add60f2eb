// train_nac_beta.hip -- NAC with the Beta policy and a SARSA critic over the stable compatible basis on ContinuousMountainCar
// (kernels_nac_beta.hpp), Fourier orders 1-5: the fused driver loop, critic.handle, NAC::handle(()), Q(s, a), the 2 * mode - 1 rollout and the
// domain's transition on the pending actions.  The policy side on explicit states and reset's initial sample run train_tdac_beta.hip's kernels on the
// same columns.  Kept in a translation unit of its own so that no other kernel's machine code moves.
#define RSRL_BETA_DEVICE_FUNCTIONS_ONLY      // (kernels_tdac_beta.hpp: its two non-template kernels are train_tdac_beta.hip's)
#include "launch.hpp"
#include "kernels_nac_beta.hpp"
#include "model_list.hpp"

namespace rsrl {

static inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

bool launch_nac_beta(int order, hipStream_t st, const Common& k, const NacBetaState& ns, uint64_t t, int chunk, DevStats* stats, const TransitionsF32* io) {
#define X(OR)                                                                                                                                              \
    if (order == OR) {                                                                                                                                     \
        if (io) hipLaunchKernelGGL((k_handle_nac_beta<OR>), grid1(io->M), dim3(kBlock), 0, st, k, ns, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out); \
        else hipLaunchKernelGGL((k_train_nac_beta<OR>), grid1(k.n_envs), dim3(kBlock), 0, st, k, ns, t, chunk, stats);                                    \
        return true;                                                                                                                                       \
    }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

bool launch_nac_update(int order, hipStream_t st, const Common& k, const NacBetaState& ns, const uint8_t* mask, float* norm_out) {
#define X(OR) if (order == OR) { hipLaunchKernelGGL((k_nac_update<OR>), grid1(k.n_envs), dim3(kBlock), 0, st, k, ns, mask, norm_out); return true; }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

bool launch_nac_q(int order, hipStream_t st, const Common& k, const NacBetaState& ns, const float* states, const float* act, int64_t M, float* q_out) {
#define X(OR) if (order == OR) { hipLaunchKernelGGL((k_nac_q<OR>), grid1(M), dim3(kBlock), 0, st, k, ns, states, act, M, q_out); return true; }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

bool launch_nac_rollout_mode(int order, hipStream_t st, const Common& k, const float* pol, int64_t step_limit, uint32_t* n_states, float* total) {
#define X(OR) if (order == OR) { hipLaunchKernelGGL((k_nac_rollout_mode<OR>), grid1(k.n_envs), dim3(kBlock), 0, st, k, pol, step_limit, n_states, total); return true; }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

void launch_nac_domain_step(hipStream_t st, const Common& k, const float* act, const float* pending, float* from, float* next, float* rew, uint8_t* term) {
    hipLaunchKernelGGL(k_nac_domain_step, grid1(k.n_envs), dim3(kBlock), 0, st, k, act, pending, from, next, rew, term);
}

}  // namespace rsrl
