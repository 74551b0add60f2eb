// train_tdac_beta.hip -- ActorCritic::tdac with the iLSTD critic and the Beta policy on ContinuousMountainCar (kernels_tdac_beta.hpp), Fourier orders
// 1-5: the fused driver loop and Handler::handle.  The policy side is train_cont_policy.hip's; the value side runs train_lstd.hip's V kernel on the
// f64 theta (the features are MountainCar's).
#include "launch.hpp"
#include "kernels_tdac_beta.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_tdac_beta(int order, hipStream_t st, const Common& k, const TdacBetaState& ts, uint64_t t, int chunk, DevStats* stats, const TransitionsF32* io) {
    return for_cmc_order(order, [&](auto o) {
        const dim3 grid = lstd_grid(io ? io->M : k.n_envs, LstdGroup<FourierReg<kCmc, o.value>::F>::G), block(kBlock);
        if (io) hipLaunchKernelGGL((k_handle_tdac_beta<o.value>), grid, block, 0, st, k, ts, io->from, io->act, io->rew, io->to, io->term, io->M, io->td_out);
        else hipLaunchKernelGGL((k_train_tdac_beta<o.value>), grid, block, 0, st, k, ts, t, chunk, stats);
    });
}

}  // namespace rsrl
