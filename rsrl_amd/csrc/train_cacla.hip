// train_cacla.hip -- CACLA over the Gaussian policy with a TD(0) critic on ContinuousMountainCar (kernels_cacla.hpp), Fourier orders 1-5: the fused
// driver loop and eval.handle + CACLA::handle on caller transitions.  The policy side on explicit states, reset's initial sample and the mode rollout
// are train_nac_gauss.hip's (kernels_gaussian.hpp), V(s) train_td.hip's k_v_evaluate and the domain's transition train_tdac_beta.hip's
// k_cmc_domain_step.  Kept in a translation unit of its own so that no other kernel's machine code moves.
#define RSRL_BETA_DEVICE_FUNCTIONS_ONLY      // (kernels_tdac_beta.hpp: its two non-template kernels are train_tdac_beta.hip's)
#include "launch.hpp"
#include "kernels_cacla.hpp"
#include "model_list.hpp"

namespace rsrl {

static inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

bool launch_cacla(int order, hipStream_t st, const Common& k, const CaclaState& cs, uint64_t t, int chunk, DevStats* stats, const TransitionsF32* io) {
#define X(OR)                                                                                                                                          \
    if (order == OR) {                                                                                                                                 \
        if (io) hipLaunchKernelGGL((k_handle_cacla<OR>), grid1(io->M), dim3(kBlock), 0, st, k, cs, io->from, io->act, io->rew, io->to, io->term, io->M, io->td_out); \
        else hipLaunchKernelGGL((k_train_cacla<OR>), grid1(k.n_envs), dim3(kBlock), 0, st, k, cs, t, chunk, stats);                                   \
        return true;                                                                                                                                   \
    }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

}  // namespace rsrl
