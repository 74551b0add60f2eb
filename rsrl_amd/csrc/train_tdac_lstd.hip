// train_tdac_lstd.hip -- ActorCritic::tdac with the iLSTD critic (kernels_tdac_lstd.hpp) on the register-family Fourier orders: the fused driver loop
// and Handler::handle.  The actor's side of the other entry points (reset's initial sample, the policy operations, rollouts) runs the existing model
// kernels on the actor's theta, the value side train_lstd.hip's V kernel on the f64 theta.  Kept in a translation unit of its own so that no other
// kernel's machine code moves.
#include "launch.hpp"
#include "kernels_tdac_lstd.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_tdac_lstd(int domain, int order, hipStream_t st, const Common& k, const TdacLstdState& ts, uint64_t t, int chunk, DevStats* stats,
                      const Transitions* io) {
    return for_reg_fourier(domain, order, [&](auto m) {
        const dim3 grid = lstd_grid(io ? io->M : k.n_envs, LstdGroup<FourierReg<m.domain, m.order>::F>::G), block(kBlock);
        if (io) hipLaunchKernelGGL((k_handle_tdac_lstd<m.domain, m.order>), grid, block, 0, st, k, ts, io->from, io->act, io->rew, io->to, io->term, io->M, io->td_out);
        else hipLaunchKernelGGL((k_train_tdac_lstd<m.domain, m.order>), grid, block, 0, st, k, ts, t, chunk, stats);
    });
}

}  // namespace rsrl
