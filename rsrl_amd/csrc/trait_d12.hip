// trait-granular kernels (kernels_trait.hpp), CartPole / Acrobot, Fourier order 1; the dispatcher; policy.sample
#include "kernels_trait.hpp"
namespace rsrl {
bool launch_trait_lm_d0_low(int domain, int order, int algo, int policy, hipStream_t st, const Common& k, const TraitIo& io, uint64_t t);
bool launch_trait_lm_d0_high(int domain, int order, int algo, int policy, hipStream_t st, const Common& k, const TraitIo& io, uint64_t t);
static bool launch_trait_lm_d12(int domain, int order, int algo, int policy, hipStream_t st, const Common& k, const TraitIo& io, uint64_t t) {
    if (domain == 1) return launch_trait_lm_orders<1, 1>(order, algo, policy, st, k, io, t);
    return domain == 2 && launch_trait_lm_orders<2, 1>(order, algo, policy, st, k, io, t);
}
bool trait_lm_available(int domain, int order, int algo) {
    return for_trait_fourier(domain, order, [](auto) {}) && is_one_step_algo(algo);
}
bool launch_trait_lm(int domain, int order, int algo, int policy, hipStream_t st, const Common& k, const TraitIo& io, uint64_t t) {
    if (!trait_lm_available(domain, order, algo)) return false;
    if (domain == 0) return order == 5 ? launch_trait_lm_d0_high(domain, order, algo, policy, st, k, io, t) : launch_trait_lm_d0_low(domain, order, algo, policy, st, k, io, t);
    return launch_trait_lm_d12(domain, order, algo, policy, st, k, io, t);
}
bool launch_trait_sample(int domain, int order, hipStream_t st, const Common& k, const float* states, int64_t Mn, uint64_t t, uint32_t blk, float* qkey,
                         float* qval, int32_t* actions_out) {
    return for_trait_fourier(domain, order, [&](auto m) {
        hipLaunchKernelGGL((k_trait_sample<m.domain, m.order>), dim3(grid_for(Mn)), dim3(kBlock), 0, st, k, states, Mn, t, blk, qkey, qval, actions_out);
    });
}
}  // namespace rsrl
