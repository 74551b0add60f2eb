// fused eligibility-trace driver loops (SARSA(lambda), Q(lambda)) for the register family
#include "launch.hpp"
#include "kernels_lambda.hpp"
#include "kernels_lambda_mem.hpp"
#include "model_list.hpp"
namespace rsrl {

#define RSRL_LAMBDA_CASE(DM, OR, AL, PO)                                                                      \
    if (domain == DM && order == OR && algo == AL && policy == PO) {                                          \
        hipLaunchKernelGGL((k_train_lambda<DM, OR, AL, PO>), grid, block, 0, st, k, lp, t, chunk, stats);     \
        return true;                                                                                          \
    }
#define RSRL_LAMBDA_POLICIES(DM, OR, AL) \
    RSRL_LAMBDA_CASE(DM, OR, AL, 0) RSRL_LAMBDA_CASE(DM, OR, AL, 1) RSRL_LAMBDA_CASE(DM, OR, AL, 2) RSRL_LAMBDA_CASE(DM, OR, AL, 3)
#define RSRL_LAMBDA_ALGOS(DM, OR) RSRL_LAMBDA_POLICIES(DM, OR, 3) RSRL_LAMBDA_POLICIES(DM, OR, 4)

#define RSRL_HL_CASE(DM, OR)                                                                                                        \
    if (domain == DM && order == OR) {                                                                                              \
        hipLaunchKernelGGL((k_handle_lambda<DM, OR>), grid, block, 0, st, k, lp, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out); \
        return true;                                                                                                                \
    }
bool launch_lambda(int domain, int order, int algo, int policy, dim3 grid, dim3 block, hipStream_t st, const Common& k, const LambdaParams& lp,
                   uint64_t t, int chunk, DevStats* stats, const Transitions* io) {
    if (io) {
        RSRL_REG_FOURIER(RSRL_HL_CASE)
        return false;
    }
    RSRL_REG_FOURIER(RSRL_LAMBDA_ALGOS)
    return false;
}
// SARSALambda / QLambda on the generic Fourier orders (kernels_lambda_mem.hpp); the driver loop runs four threads per learner, 64 learners per block
bool launch_lambda_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const LambdaParams& lp, const BasisGeom& g,
                         uint64_t t, int chunk, DevStats* stats, const Transitions* io) {
#define RSRL_LM_CASE(DM)                                                                                                             \
    if (cfg.domain == DM) {                                                                                                          \
        using M = FourierGenericModel<DM>;                                                                                           \
        if (io) hipLaunchKernelGGL((k_handle_lambda_mem<M>), grid, block, 0, st, k, lp, g, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out); \
        else hipLaunchKernelGGL((k_train_lambda_mem4<M>), dim3((unsigned)((k.n_envs + 63) / 64)), dim3(256), 0, st, k, lp, g, t, chunk, stats);               \
        return true;                                                                                                                 \
    }
    if (cfg.basis != RSRL_FOURIER || cfg.order < 1 || cfg.order > 7) return false;
    RSRL_LM_CASE(0) RSRL_LM_CASE(1) RSRL_LM_CASE(2)
    return false;
}
}  // namespace rsrl
