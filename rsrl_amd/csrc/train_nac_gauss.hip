// train_nac_gauss.hip -- NAC with the Gaussian policy and a SARSA critic over the stable compatible basis on ContinuousMountainCar
// (kernels_nac_gauss.hpp), Fourier orders 1-5: the fused driver loop, critic.handle and Q(s, a); and the Gaussian policy's own kernels
// (kernels_gaussian.hpp): the policy side on explicit states, reset's initial sample and the mode rollout.  NAC::handle(()) on its own is
// train_nac_beta.hip's k_nac_update, and the domain's transition on the pending actions, which this loop does not map, train_tdac_beta.hip's
// k_cmc_domain_step.  Kept in a translation unit of its own so that no other kernel's machine code moves.
#define RSRL_BETA_DEVICE_FUNCTIONS_ONLY      // (kernels_tdac_beta.hpp: its two non-template kernels are train_tdac_beta.hip's)
#include "launch.hpp"
#include "kernels_nac_gauss.hpp"
#include "model_list.hpp"

namespace rsrl {

static inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

bool launch_nac_gauss(int order, hipStream_t st, const Common& k, const NacBetaState& ns, uint64_t t, int chunk, DevStats* stats, const TransitionsF32* io) {
#define X(OR)                                                                                                                                              \
    if (order == OR) {                                                                                                                                     \
        if (io) hipLaunchKernelGGL((k_handle_nac_gauss<OR>), grid1(io->M), dim3(kBlock), 0, st, k, ns, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out); \
        else hipLaunchKernelGGL((k_train_nac_gauss<OR>), grid1(k.n_envs), dim3(kBlock), 0, st, k, ns, t, chunk, stats);                                   \
        return true;                                                                                                                                       \
    }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

bool launch_nac_gauss_q(int order, hipStream_t st, const Common& k, const NacBetaState& ns, const float* states, const float* act, int64_t M, float* q_out) {
#define X(OR) if (order == OR) { hipLaunchKernelGGL((k_nac_gauss_q<OR>), grid1(M), dim3(kBlock), 0, st, k, ns, states, act, M, q_out); return true; }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

bool launch_gauss_policy(int order, hipStream_t st, const Common& k, const float* w, int op, const float* states, int64_t M, uint64_t t, uint32_t purpose,
                         const float* act_in, float* out0, float* out1, float* keep) {
#define X(OR) if (order == OR) { hipLaunchKernelGGL((k_gauss_policy<OR>), grid1(M), dim3(kBlock), 0, st, k, w, op, states, M, t, purpose, act_in, out0, out1, keep); return true; }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

bool launch_gauss_reset(int order, hipStream_t st, const Common& k, const float* w, uint64_t t, float* action) {
#define X(OR) if (order == OR) { hipLaunchKernelGGL((k_gauss_reset<OR>), grid1(k.n_envs), dim3(kBlock), 0, st, k, w, t, action); return true; }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

bool launch_gauss_rollout_mode(int order, hipStream_t st, const Common& k, const float* w, int64_t step_limit, uint32_t* n_states, float* total) {
#define X(OR) if (order == OR) { hipLaunchKernelGGL((k_gauss_rollout_mode<OR>), grid1(k.n_envs), dim3(kBlock), 0, st, k, w, step_limit, n_states, total); return true; }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

}  // namespace rsrl
