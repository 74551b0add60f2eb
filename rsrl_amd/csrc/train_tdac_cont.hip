// train_tdac_cont.hip -- ActorCritic::tdac with a TD(0) critic over the Gaussian or the Beta policy on ContinuousMountainCar
// (kernels_tdac_cont.hpp), Fourier orders 1-5: the fused driver loop and eval.handle + ActorCritic::handle on caller transitions, one
// instantiation per order and policy.  The policy side on explicit states, reset's initial sample and the mode rollout are train_nac_gauss.hip's
// (Gaussian) and train_tdac_beta.hip's / train_nac_beta.hip's (Beta), V(s) train_td.hip's k_v_evaluate and the domain's transition
// k_cmc_domain_step (Gaussian) or k_nac_domain_step (Beta).  Kept in a translation unit of its own so that no other kernel's machine code moves.
#define RSRL_BETA_DEVICE_FUNCTIONS_ONLY          // (kernels_tdac_beta.hpp: its two non-template kernels are train_tdac_beta.hip's)
#define RSRL_NAC_BETA_DEVICE_FUNCTIONS_ONLY      // (kernels_nac_beta.hpp: its one non-template kernel is train_nac_beta.hip's)
#include "launch.hpp"
#include "kernels_tdac_cont.hpp"
#include "model_list.hpp"

namespace rsrl {

static inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

template <ContPolicy POLICY>
static bool launch_tdac_cont_of(int order, hipStream_t st, const Common& k, const TdacContState& ts, uint64_t t, int chunk, DevStats* stats,
                                const TransitionsF32* io) {
#define X(OR)                                                                                                                                          \
    if (order == OR) {                                                                                                                                 \
        if (io) hipLaunchKernelGGL((k_handle_tdac_cont<OR, POLICY>), grid1(io->M), dim3(kBlock), 0, st, k, ts, io->from, io->act, io->rew, io->to, io->term, io->M, io->td_out); \
        else hipLaunchKernelGGL((k_train_tdac_cont<OR, POLICY>), grid1(k.n_envs), dim3(kBlock), 0, st, k, ts, t, chunk, stats);                      \
        return true;                                                                                                                                   \
    }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}

bool launch_tdac_cont(int order, ContPolicy policy, hipStream_t st, const Common& k, const TdacContState& ts, uint64_t t, int chunk, DevStats* stats,
                      const TransitionsF32* io) {
    return policy == ContPolicy::Gaussian ? launch_tdac_cont_of<ContPolicy::Gaussian>(order, st, k, ts, t, chunk, stats, io)
                                          : launch_tdac_cont_of<ContPolicy::Beta>(order, st, k, ts, t, chunk, stats, io);
}

}  // namespace rsrl
