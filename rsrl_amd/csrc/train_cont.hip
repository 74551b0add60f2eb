// train_cont.hip -- CACLA over the Gaussian policy and ActorCritic::tdac with a TD(0) critic over the Gaussian or the Beta policy on
// ContinuousMountainCar (kernels_cont.hpp), Fourier orders 1-5: the fused driver loop and eval.handle + the agent's handle on caller transitions,
// one instantiation per order and rule.  The policy side is train_cont_policy.hip's, V(s) train_td.hip's k_v_evaluate.
#include "launch.hpp"
#include "kernels_cont.hpp"
#include "model_list.hpp"

namespace rsrl {

static inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

bool launch_td0_cont(int order, bool cacla, ContPolicy policy, hipStream_t st, const Common& k, const ContState& cs, uint64_t t, int chunk, DevStats* stats,
                     const TransitionsF32* io) {
    if (cacla && policy != ContPolicy::Gaussian) return false;
#define RULE(OR, ...)                                                                                                                                  \
    {                                                                                                                                                  \
        if (io) hipLaunchKernelGGL((k_handle_td0_cont<OR, __VA_ARGS__>), grid1(io->M), dim3(kBlock), 0, st, k, cs, io->from, io->act, io->rew, io->to, io->term, io->M, io->td_out); \
        else hipLaunchKernelGGL((k_train_td0_cont<OR, __VA_ARGS__>), grid1(k.n_envs), dim3(kBlock), 0, st, k, cs, t, chunk, stats);                   \
        return true;                                                                                                                                   \
    }
#define X(OR)                                                                                                                                          \
    if (order == OR) {                                                                                                                                 \
        if (cacla) RULE(OR, CaclaRule)                                                                                                                 \
        if (policy == ContPolicy::Gaussian) RULE(OR, TdacContRule<ContPolicy::Gaussian>)                                                              \
        RULE(OR, TdacContRule<ContPolicy::Beta>)                                                                                                       \
    }
    RSRL_CMC_ORDERS(X)
#undef X
#undef RULE
    return false;
}

}  // namespace rsrl
