// train_cont.hip -- CACLA over the Gaussian policy and ActorCritic::tdac with a TD(0) critic over the Gaussian or the Beta policy on
// ContinuousMountainCar (kernels_cont.hpp), Fourier orders 1-5: the fused driver loop and eval.handle + the agent's handle on caller transitions,
// one instantiation per order and rule.  The policy side is train_cont_policy.hip's, V(s) train_td.hip's k_v_evaluate.
#include "launch.hpp"
#include "kernels_cont.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_td0_cont(int order, bool cacla, ContPolicy policy, hipStream_t st, const Common& k, const ContState& cs, uint64_t t, int chunk, DevStats* stats,
                     const TransitionsF32* io) {
    if (cacla && policy != ContPolicy::Gaussian) return false;
    return for_cmc_order(order, [&](auto o) {
        constexpr int OR = o.value;
        auto run = [&](auto rule) {
            using Rule = typename decltype(rule)::type;
            if (io) hipLaunchKernelGGL((k_handle_td0_cont<OR, Rule>), dim3(grid_for(io->M)), dim3(kBlock), 0, st, k, cs, io->from, io->act, io->rew, io->to, io->term, io->M, io->td_out);
            else hipLaunchKernelGGL((k_train_td0_cont<OR, Rule>), dim3(grid_for(k.n_envs)), dim3(kBlock), 0, st, k, cs, t, chunk, stats);
        };
        if (cacla) run(Tag<CaclaRule>{});
        else for_cont_policy(policy, [&](auto p) { run(Tag<TdacContRule<p.value>>{}); });
    });
}

}  // namespace rsrl
