// train_tdac.hip -- ActorCritic with the TD(0) state-value critic (kernels_tdac.hpp) on the register-family Fourier orders: the fused driver loop
// and Handler::handle.  The actor's side of the other entry points (reset's initial sample, the policy operations, rollouts) runs the existing model
// kernels on theta, the value side the TD agents' V kernels on w.  Kept in a translation unit of its own so that no other kernel's machine code moves.
#include "launch.hpp"
#include "kernels_tdac.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_tdac(int domain, int order, dim3 grid, dim3 block, hipStream_t st, const Common& k, float* theta, uint64_t t, int chunk, DevStats* stats,
                 const Transitions* io) {
    return for_reg_fourier(domain, order, [&](auto m) {
        if (io) hipLaunchKernelGGL((k_handle_tdac<m.domain, m.order>), grid, block, 0, st, k, theta, io->from, io->act, io->rew, io->to, io->term, io->M, io->td_out);
        else hipLaunchKernelGGL((k_train_tdac<m.domain, m.order>), grid, block, 0, st, k, theta, t, chunk, stats);
    });
}

}  // namespace rsrl
