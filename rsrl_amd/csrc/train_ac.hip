// train_ac.hip -- ActorCritic (kernels_ac.hpp) on the register-family Fourier orders: the fused driver loop and Handler::handle, both critics.
// The actor's side of the other entry points (reset's initial sample, the policy operations, rollouts) runs the existing model kernels on
// theta (abi_*.hip hand them a Common whose weight pointer is the auxiliary matrix).  Kept in a translation unit of its own so that no other
// kernel's machine code moves.
#include "launch.hpp"
#include "kernels_ac.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_ac(int domain, int order, int critic, dim3 grid, dim3 block, hipStream_t st, const Common& k, float* theta, uint64_t t, int chunk,
               DevStats* stats, const Transitions* io) {
    bool found = false;
    for_reg_fourier(domain, order, [&](auto m) { found = for_int<AC_CRITIC_ADVANTAGE, AC_CRITIC_Q>(critic, [&](auto cr) {
        constexpr int DM = decltype(m)::domain, OR = decltype(m)::order, CR = cr.value;
        if (io) hipLaunchKernelGGL((k_handle_ac<DM, OR, CR>), grid, block, 0, st, k, theta, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out);
        else hipLaunchKernelGGL((k_train_ac<DM, OR, CR>), grid, block, 0, st, k, theta, t, chunk, stats);
    }); });
    return found;
}

}  // namespace rsrl
