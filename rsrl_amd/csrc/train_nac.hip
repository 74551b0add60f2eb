// train_nac.hip -- NAC with the Gaussian or the Beta policy and a SARSA critic over the stable compatible basis on ContinuousMountainCar
// (kernels_cont.hpp), Fourier orders 1-5: the fused driver loop, critic.handle, NAC::handle(()) and Q(s, a).  The policy side is
// train_cont_policy.hip's.
#include "launch.hpp"
#include "kernels_cont.hpp"
#include "model_list.hpp"

namespace rsrl {

static inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

bool launch_nac(int order, ContPolicy policy, hipStream_t st, const Common& k, const ContState& cs, uint32_t period, uint64_t t, int chunk, DevStats* stats,
                const TransitionsF32* io) {
#define X(OR)                                                                                                                                              \
    if (order == OR) {                                                                                                                                     \
        const bool g = policy == ContPolicy::Gaussian;                                                                                                     \
        if (io && g) hipLaunchKernelGGL((k_handle_nac<OR, ContPolicy::Gaussian>), grid1(io->M), dim3(kBlock), 0, st, k, cs, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out); \
        else if (io) hipLaunchKernelGGL((k_handle_nac<OR, ContPolicy::Beta>), grid1(io->M), dim3(kBlock), 0, st, k, cs, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out); \
        else if (g) hipLaunchKernelGGL((k_train_nac<OR, ContPolicy::Gaussian>), grid1(k.n_envs), dim3(kBlock), 0, st, k, cs, period, t, chunk, stats);                    \
        else hipLaunchKernelGGL((k_train_nac<OR, ContPolicy::Beta>), grid1(k.n_envs), dim3(kBlock), 0, st, k, cs, period, t, chunk, stats);                            \
        return true;                                                                                                                                       \
    }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

bool launch_nac_update(int order, hipStream_t st, const Common& k, const ContState& cs, const uint8_t* mask, float* norm_out) {
#define X(OR) if (order == OR) { hipLaunchKernelGGL((k_nac_update<OR>), grid1(k.n_envs), dim3(kBlock), 0, st, k, cs, mask, norm_out); return true; }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

bool launch_nac_q(int order, ContPolicy policy, hipStream_t st, const Common& k, const ContState& cs, const float* states, const float* act, int64_t M,
                  float* q_out) {
#define X(OR)                                                                                                                                         \
    if (order == OR) {                                                                                                                                \
        if (policy == ContPolicy::Gaussian) hipLaunchKernelGGL((k_nac_q<OR, ContPolicy::Gaussian>), grid1(M), dim3(kBlock), 0, st, k, cs, states, act, M, q_out); \
        else hipLaunchKernelGGL((k_nac_q<OR, ContPolicy::Beta>), grid1(M), dim3(kBlock), 0, st, k, cs, states, act, M, q_out);                      \
        return true;                                                                                                                                  \
    }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

}  // namespace rsrl
