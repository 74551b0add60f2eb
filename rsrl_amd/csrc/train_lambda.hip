// fused eligibility-trace driver loops (SARSA(lambda), Q(lambda)) for the register family
#include "launch.hpp"
#include "kernels_lambda.hpp"
#include "kernels_lambda_mem.hpp"
#include "model_list.hpp"
namespace rsrl {

bool launch_lambda(int domain, int order, int algo, int policy, dim3 grid, dim3 block, hipStream_t st, const Common& k, const LambdaParams& lp,
                   uint64_t t, int chunk, DevStats* stats, const Transitions* io) {
    if (io)
        return for_reg_fourier(domain, order, [&](auto m) {
            hipLaunchKernelGGL((k_handle_lambda<m.domain, m.order>), grid, block, 0, st, k, lp, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out);
        });
    bool found = false;
    for_reg_fourier(domain, order, [&](auto m) { for_int<3, 4>(algo, [&](auto al) { found = for_policy(policy, [&](auto po) {
        hipLaunchKernelGGL((k_train_lambda<decltype(m)::domain, decltype(m)::order, decltype(al)::value, po.value>), grid, block, 0, st, k, lp, t, chunk, stats);
    }); }); });
    return found;
}
// SARSALambda / QLambda on the generic Fourier orders (kernels_lambda_mem.hpp); the driver loop runs four threads per learner, 64 learners per block
bool launch_lambda_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const LambdaParams& lp, const BasisGeom& g,
                         uint64_t t, int chunk, DevStats* stats, const Transitions* io) {
    if (cfg.basis != RSRL_FOURIER || cfg.order < 1 || cfg.order > 7) return false;
    return for_domain3(cfg.domain, [&](auto d) {
        using M = FourierGenericModel<d.value>;
        if (io) hipLaunchKernelGGL((k_handle_lambda_mem<M>), grid, block, 0, st, k, lp, g, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out);
        else hipLaunchKernelGGL((k_train_lambda_mem4<M>), dim3(grid_for(k.n_envs, 64)), dim3(256), 0, st, k, lp, g, t, chunk, stats);
    });
}
}  // namespace rsrl
