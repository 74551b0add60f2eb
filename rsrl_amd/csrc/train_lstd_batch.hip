// train_lstd_batch.hip -- LSTD and LSTDLambda (kernels_lstd_batch.hpp) on the register-family Fourier orders: the fused driver loop with its per-learner
// episode record, Handler<&Batch>::handle on whole transitions and the agents' solve().  V(s), the theta <-> f32 weights and the driver loop's Random
// sample run train_lstd.hip's kernels, the record's read-out train_gmc.hip's.  Kept in a translation unit of its own so that no other kernel's
// machine code moves.
#include "launch.hpp"
#include "kernels_lstd_batch.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_lstd_batch(int domain, int order, bool lambda, hipStream_t st, const Common& k, const LstdBatchState& ls, uint64_t t, int chunk, DevStats* stats,
                       const TransitionBatch* io) {
    return for_reg_fourier(domain, order, [&](auto m) {
        constexpr int DM = m.domain, OR = m.order;
        const dim3 grid = lstd_grid(k.n_envs, LstdGroup<FourierReg<DM, OR>::F>::G), block(kBlock);
        auto run = [&](auto la) {
            if (io) hipLaunchKernelGGL((k_handle_lstd_batch<DM, OR, la.value>), grid, block, 0, st, ls, io->from, io->rew, io->to, io->term, io->len, io->T, k.n_envs, io->td_out);
            else hipLaunchKernelGGL((k_train_lstd_batch<DM, OR, la.value>), grid, block, 0, st, k, ls, t, chunk, stats);
        };
        if (lambda) run(std::true_type{}); else run(std::false_type{});
    });
}

bool launch_lstd_batch_solve(int domain, int order, bool lambda, hipStream_t st, const LstdBatchState& ls, int64_t N) {
    return for_reg_fourier(domain, order, [&](auto m) {
        const dim3 grid = lstd_grid(N, LstdGroup<FourierReg<m.domain, m.order>::F>::G), block(kBlock);
        if (lambda) hipLaunchKernelGGL((k_lstd_batch_solve<m.domain, m.order, true>), grid, block, 0, st, ls, N);
        else hipLaunchKernelGGL((k_lstd_batch_solve<m.domain, m.order, false>), grid, block, 0, st, ls, N);
    });
}

}  // namespace rsrl
