// train_reinforce.hip -- REINFORCE and BaselineREINFORCE (kernels_reinforce.hpp) on the register-family Fourier orders: the fused driver loop,
// Handler<&Batch>::handle and the episode restart of theta_b / g.  The policy side of the other entry points (reset's initial sample, the policy
// operations, rollouts) runs the existing model kernels on theta.  Kept in a translation unit of its own so that no other kernel's machine code moves.
#include "launch.hpp"
#include "kernels_reinforce.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_reinforce(int domain, int order, bool baseline, dim3 grid, dim3 block, hipStream_t st, const Common& k, const ReinforceState& rs, uint64_t t,
                      int chunk, DevStats* stats, const ReinforceBatch* io) {
    return for_reg_fourier(domain, order, [&](auto m) {
        constexpr int DM = m.domain, OR = m.order;
        if (io) {
            if (baseline) hipLaunchKernelGGL((k_handle_reinforce<DM, OR, true>), grid, block, 0, st, k, rs.theta, io->states, io->act, io->rew, io->len, io->T, io->ret_out);
            else hipLaunchKernelGGL((k_handle_reinforce<DM, OR, false>), grid, block, 0, st, k, rs.theta, io->states, io->act, io->rew, io->len, io->T, io->ret_out);
        } else if (baseline) hipLaunchKernelGGL((k_train_reinforce<DM, OR, true>), grid, block, 0, st, k, rs, t, chunk, stats);
        else hipLaunchKernelGGL((k_train_reinforce<DM, OR, false>), grid, block, 0, st, k, rs, t, chunk, stats);
    });
}

void launch_reinforce_restart(hipStream_t st, const ReinforceState& rs, int64_t N, int64_t FA, const uint8_t* mask) {
    const int64_t n = FA * N;
    hipLaunchKernelGGL(k_reinforce_restart, dim3(grid_for(n)), dim3(kBlock), 0, st, rs, N, FA, mask);
}

}  // namespace rsrl
