// train_lspe.hip -- LambdaLSPE (kernels_lstd_batch.hpp) on the register-family Fourier orders: the fused driver loop with its per-learner episode
// record, Handler<&Batch>::handle on whole transitions and the agent's solve() (the row rule, the relaxed step, the zeroing).  Everything around
// them -- V(s), the theta <-> f32 weights, the Random sample, the record's read-out -- runs LSTD's kernels.  Kept in a translation unit of its own
// so that LSTD's and LSTDLambda's machine code (train_lstd_batch.hip) does not move.
#include "launch.hpp"
#include "kernels_lstd_batch.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_lspe(int domain, int order, hipStream_t st, const Common& k, const LspeState& ls, uint64_t t, int chunk, DevStats* stats, const TransitionBatch* io) {
    return for_reg_fourier(domain, order, [&](auto m) {
        constexpr int DM = m.domain, OR = m.order;
        const dim3 grid = lstd_grid(k.n_envs, LstdGroup<FourierReg<DM, OR>::F>::G), block(kBlock);
        if (io) hipLaunchKernelGGL((k_handle_lspe<DM, OR>), grid, block, 0, st, ls, io->from, io->rew, io->to, io->term, io->len, io->T, k.n_envs, io->td_out);
        else hipLaunchKernelGGL((k_train_lspe<DM, OR>), grid, block, 0, st, k, ls, t, chunk, stats);
    });
}

bool launch_lspe_solve(int domain, int order, hipStream_t st, const LspeState& ls, int64_t N) {
    return for_reg_fourier(domain, order, [&](auto m) {
        const dim3 grid = lstd_grid(N, LstdGroup<FourierReg<m.domain, m.order>::F>::G), block(kBlock);
        hipLaunchKernelGGL((k_lspe_solve<m.domain, m.order>), grid, block, 0, st, ls, N);
    });
}

}  // namespace rsrl
