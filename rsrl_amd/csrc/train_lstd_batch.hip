// train_lstd_batch.hip -- LSTD and LSTDLambda (kernels_lstd_batch.hpp) on the register-family Fourier orders: the fused driver loop with its per-learner
// episode record, Handler<&Batch>::handle on whole transitions and the agents' solve().  V(s), the theta <-> f32 weights and the driver loop's Random
// sample run train_lstd.hip's kernels, the record's read-out train_gmc.hip's.  Kept in a translation unit of its own so that no other kernel's
// machine code moves.
#include "launch.hpp"
#include "kernels_lstd_batch.hpp"
#include "model_list.hpp"

namespace rsrl {

#define RSRL_LSTD_BATCH_KERNELS(DM, OR, LA)                                                                                                     \
    if (io) hipLaunchKernelGGL((k_handle_lstd_batch<DM, OR, LA>), grid, block, 0, st, ls, io->from, io->rew, io->to, io->term, io->len, io->T, k.n_envs, \
                               io->td_out);                                                                                                     \
    else hipLaunchKernelGGL((k_train_lstd_batch<DM, OR, LA>), grid, block, 0, st, k, ls, t, chunk, stats);

#define RSRL_LSTD_BATCH_CASE(DM, OR)                                                                                                            \
    if (domain == DM && order == OR) {                                                                                                          \
        const dim3 grid = lstd_grid(k.n_envs, LstdGroup<FourierReg<DM, OR>::F>::G), block(kBlock);                                              \
        if (lambda) { RSRL_LSTD_BATCH_KERNELS(DM, OR, true) } else { RSRL_LSTD_BATCH_KERNELS(DM, OR, false) }                                   \
        return true;                                                                                                                            \
    }

bool launch_lstd_batch(int domain, int order, bool lambda, hipStream_t st, const Common& k, const LstdBatchState& ls, uint64_t t, int chunk, DevStats* stats,
                       const TransitionBatch* io) {
    RSRL_REG_FOURIER(RSRL_LSTD_BATCH_CASE)
    return false;
}

#define RSRL_LSTD_BATCH_SOLVE_CASE(DM, OR)                                                                                                      \
    if (domain == DM && order == OR) {                                                                                                          \
        const dim3 grid = lstd_grid(N, LstdGroup<FourierReg<DM, OR>::F>::G), block(kBlock);                                                     \
        if (lambda) hipLaunchKernelGGL((k_lstd_batch_solve<DM, OR, true>), grid, block, 0, st, ls, N);                                          \
        else hipLaunchKernelGGL((k_lstd_batch_solve<DM, OR, false>), grid, block, 0, st, ls, N);                                                \
        return true;                                                                                                                            \
    }

bool launch_lstd_batch_solve(int domain, int order, bool lambda, hipStream_t st, const LstdBatchState& ls, int64_t N) {
    RSRL_REG_FOURIER(RSRL_LSTD_BATCH_SOLVE_CASE)
    return false;
}

}  // namespace rsrl
