// train_gibbs_nac.hip -- NAC over the Gibbs policy with a SARSA critic over the stable compatible basis (kernels_gibbs_nac.hpp) on the
// register-family Fourier orders: the fused driver loop, critic.handle, NAC::handle(()) and Q(s, .).  The policy side of the other entry points
// (reset's initial sample, the policy operations, rollouts) runs the existing model kernels on theta, as ActorCritic's.  Kept in a translation
// unit of its own so that no other kernel's machine code moves.
#include "launch.hpp"
#include "kernels_gibbs_nac.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_gibbs_nac(int domain, int order, dim3 grid, dim3 block, hipStream_t st, const Common& k, float* theta, uint32_t period, uint64_t t, int chunk,
                      DevStats* stats, const Transitions* io) {
    return for_reg_fourier(domain, order, [&](auto m) {
        if (io) hipLaunchKernelGGL((k_handle_gibbs_nac<m.domain, m.order>), grid, block, 0, st, k, theta, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out);
        else hipLaunchKernelGGL((k_train_gibbs_nac<m.domain, m.order>), grid, block, 0, st, k, theta, period, t, chunk, stats);
    });
}

bool launch_gibbs_nac_update(int domain, int order, hipStream_t st, const Common& k, float* theta, const uint8_t* mask, float* norm_out) {
    return for_reg_fourier(domain, order, [&](auto m) {
        hipLaunchKernelGGL((k_gibbs_nac_update<m.domain, m.order>), dim3(grid_for(k.n_envs)), dim3(kBlock), 0, st, k, theta, mask, norm_out);
    });
}

bool launch_gibbs_nac_q(int domain, int order, hipStream_t st, const Common& k, const float* theta, const float* states, int64_t M, float* q_out) {
    return for_reg_fourier(domain, order, [&](auto m) {
        hipLaunchKernelGGL((k_gibbs_nac_q<m.domain, m.order>), dim3(grid_for(M)), dim3(kBlock), 0, st, k, theta, states, M, q_out);
    });
}

}  // namespace rsrl
