// train_gmc.hip -- GradientMC (kernels_gmc.hpp) on the register-family Fourier orders: the fused driver loop with its per-learner episode record,
// Handler<&Trajectory>::handle and the record's read-out.  The value side of the other entry points (q_evaluate, get / set_weights) and reset's
// Random sample run TD's kernels on the one-column W.  Kept in a translation unit of its own so that no other kernel's machine code moves.
#include "launch.hpp"
#include "kernels_gmc.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_gmc(int domain, int order, dim3 grid, dim3 block, hipStream_t st, const Common& k, const GmcState& gs, uint64_t t, int chunk, DevStats* stats,
                const GmcBatch* io) {
    return for_reg_fourier(domain, order, [&](auto m) {
        if (io) hipLaunchKernelGGL((k_handle_gmc<m.domain, m.order>), grid, block, 0, st, k, io->states, io->rew, io->len, io->T, io->ret_out);
        else hipLaunchKernelGGL((k_train_gmc<m.domain, m.order>), grid, block, 0, st, k, gs, t, chunk, stats);
    });
}

void launch_gmc_record_get(hipStream_t st, const GmcState& gs, const uint32_t* ep_step, int64_t N, int64_t cap, int D, float* states, float* rew) {
    const int64_t n = cap * N;
    hipLaunchKernelGGL(k_gmc_record_get, dim3(grid_for(n)), dim3(kBlock), 0, st, gs, ep_step, N, cap, D, states, rew);
}

}  // namespace rsrl
