// train_nac.hip -- NAC with the Gaussian or the Beta policy and a SARSA critic over the stable compatible basis on ContinuousMountainCar
// (kernels_cont.hpp), Fourier orders 1-5: the fused driver loop, critic.handle, NAC::handle(()) and Q(s, a).  The policy side is
// train_cont_policy.hip's.
#include "launch.hpp"
#include "kernels_cont.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_nac(int order, ContPolicy policy, hipStream_t st, const Common& k, const ContState& cs, uint32_t period, uint64_t t, int chunk, DevStats* stats,
                const TransitionsF32* io) {
    if (io)
        return for_cmc_order(order, [&](auto o) { for_cont_policy(policy, [&](auto p) {
            hipLaunchKernelGGL((k_handle_nac<decltype(o)::value, p.value>), dim3(grid_for(io->M)), dim3(kBlock), 0, st, k, cs, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out);
        }); });
    return for_cmc_order(order, [&](auto o) { for_cont_policy(policy, [&](auto p) {
        hipLaunchKernelGGL((k_train_nac<decltype(o)::value, p.value>), dim3(grid_for(k.n_envs)), dim3(kBlock), 0, st, k, cs, period, t, chunk, stats);
    }); });
}

bool launch_nac_update(int order, hipStream_t st, const Common& k, const ContState& cs, const uint8_t* mask, float* norm_out) {
    return for_cmc_order(order, [&](auto o) { hipLaunchKernelGGL((k_nac_update<o.value>), dim3(grid_for(k.n_envs)), dim3(kBlock), 0, st, k, cs, mask, norm_out); });
}

bool launch_nac_q(int order, ContPolicy policy, hipStream_t st, const Common& k, const ContState& cs, const float* states, const float* act, int64_t M,
                  float* q_out) {
    return for_cmc_order(order, [&](auto o) { for_cont_policy(policy, [&](auto p) {
        hipLaunchKernelGGL((k_nac_q<decltype(o)::value, p.value>), dim3(grid_for(M)), dim3(kBlock), 0, st, k, cs, states, act, M, q_out);
    }); });
}

}  // namespace rsrl
