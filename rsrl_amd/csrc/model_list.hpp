// model_list.hpp -- the lists the launchers range over, each spelled once, and one dispatcher per list (host only).  A dispatcher takes the
// run-time values and a generic lambda, calls fn(tag) for the entry that matches (first match, in the list's order) and returns whether one
// did; the tag carries the entry as compile-time constants, so the lambda's body is ordinary, type-checked C++:
//   for_int<Vs...>(v, fn)                the primitive: fn(std::integral_constant<int, V>{}) for v == V
//   RSRL_REG_FOURIER  for_reg_fourier    the register-family Fourier (domain, order) pairs: F = (order+1)^D <= 36 features per learner held in
//                                        VGPRs.  Tag: FourierTag<domain, order> (::type = FourierModel<domain, order>)
//   RSRL_TRAIT_FOURIER for_trait_fourier the rows of RSRL_REG_FOURIER that have trait-granular kernels (kernels_trait.hpp).  Tag: FourierTag
//   RSRL_CMC_ORDERS   for_cmc_order      ContinuousMountainCar's Fourier orders.  Tag: integral_constant
//   RSRL_TILE_CONFIGS for_tile           tile coding's (domain, tilings): T tilings as a template parameter (indices in VGPRs), tiles_per_dim at
//                                        run time.  Tag: TileTag<domain, n_tilings> (::type = TileModel<domain, n_tilings>)
//   0, 1, 2           for_domain3        the classic domains (MountainCar, CartPole, Acrobot)
//   0, 1, 2, 5        for_one_step_algo  the one-step agents of the fused loops (QLearning, SARSA, ExpectedSARSA, PAL)
//   0 .. 3            for_policy         the discrete policies
//   for_mem_model(cfg, fn)               the models WITHOUT a register-family kernel of their own (what the *_mem agent kernels are instantiated
//                                        for): the tile configurations, then the generic-order Fourier model (any order 1..7) of a classic
//                                        domain.  Tag: ::type = the Model
// (for_cont_policy, over the two continuous policies, is launch.hpp's, next to ContPolicy.)
// Model lookup is first match: the RSRL_REG_FOURIER rows, then for_mem_model (ctx.hpp for_model).
#pragma once

#include "../../include/rsrl_hip.h"
#include "models.hpp"

// the register-family Fourier (domain, order) pairs, in the order every launcher instantiates them (moving one moves the
// PC-relative offsets of the others' machine code).  The models of the Fourier rows: FourierModel<domain, order>
#define RSRL_REG_FOURIER(X) X(0, 1) X(0, 2) X(0, 3) X(0, 4) X(0, 5) X(1, 1) X(2, 1)
// ... of which the trait-granular kernels are instantiated for MountainCar's orders 1, 3, 5 and order 1 of CartPole and Acrobot
#define RSRL_TRAIT_FOURIER(X) X(0, 1) X(0, 3) X(0, 5) X(1, 1) X(2, 1)
// ContinuousMountainCar (domain 4, f32 actions): the Fourier orders its agents run on -- MountainCar's register-family
// orders, with MountainCar's features.  NOT rows of RSRL_REG_FOURIER: no model kernel (an index action per learner) is instantiated for it
#define RSRL_CMC_ORDERS(X) X(1) X(2) X(3) X(4) X(5)
// tile coding: (domain, tilings)
#define RSRL_TILE_CONFIGS(X) X(0, 4) X(0, 8) X(0, 16) X(1, 4) X(1, 8) X(1, 16) X(2, 4) X(2, 8) X(2, 16)

namespace rsrl {
template <class T> struct Tag { using type = T; };
template <int DM, int OR> struct FourierTag { static constexpr int domain = DM, order = OR; using type = FourierModel<DM, OR>; };
template <int DM, int TT> struct TileTag { static constexpr int domain = DM, n_tilings = TT; using type = TileModel<DM, TT>; };

template <int... Vs, class Fn>
static inline bool for_int(int v, Fn&& fn) {
    return (... || (v == Vs && (fn(std::integral_constant<int, Vs>{}), true)));      // (a left fold: instantiated first to last)
}
template <class Fn> static inline bool for_domain3(int domain, Fn&& fn) { return for_int<0, 1, 2>(domain, fn); }
template <class Fn> static inline bool for_one_step_algo(int algo, Fn&& fn) { return for_int<0, 1, 2, 5>(algo, fn); }
template <class Fn> static inline bool for_policy(int policy, Fn&& fn) { return for_int<0, 1, 2, 3>(policy, fn); }
static inline bool is_one_step_algo(int algo) { return for_one_step_algo(algo, [](auto) {}); }

// X of for_reg_fourier and for_trait_fourier: one row of either list
#define RSRL_FOURIER_ROW(DM, OR) if (domain == DM && order == OR) { fn(FourierTag<DM, OR>{}); return true; }
template <class Fn>
static inline bool for_reg_fourier(int domain, int order, Fn&& fn) {
    RSRL_REG_FOURIER(RSRL_FOURIER_ROW)
    return false;
}
template <class Fn>
static inline bool for_trait_fourier(int domain, int order, Fn&& fn) {
    RSRL_TRAIT_FOURIER(RSRL_FOURIER_ROW)
    return false;
}
#undef RSRL_FOURIER_ROW
template <class Fn>
static inline bool for_cmc_order(int order, Fn&& fn) {
#define X(OR) if (order == OR) { fn(std::integral_constant<int, OR>{}); return true; }
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}
template <class Fn>
static inline bool for_tile(int domain, int n_tilings, Fn&& fn) {
#define X(DM, TT) if (domain == DM && n_tilings == TT) { fn(TileTag<DM, TT>{}); return true; }
    RSRL_TILE_CONFIGS(X)
#undef X
    return false;
}
template <class Fn>
static inline bool for_mem_model(const rsrl_hip_config& cfg, Fn&& fn) {
    if (cfg.basis == RSRL_TILE_CODING) return for_tile(cfg.domain, cfg.n_tilings, fn);
    return cfg.basis == RSRL_FOURIER && cfg.order >= 1 && cfg.order <= 7 &&
           for_domain3(cfg.domain, [&](auto d) { fn(Tag<FourierGenericModel<d.value>>{}); });
}

// every row of RSRL_TRAIT_FOURIER is a row of RSRL_REG_FOURIER
constexpr bool reg_fourier_row(int domain, int order) {
#define X(DM, OR) if (domain == DM && order == OR) return true;
    RSRL_REG_FOURIER(X)
#undef X
    return false;
}
#define X(DM, OR) static_assert(reg_fourier_row(DM, OR), "RSRL_TRAIT_FOURIER: not a row of RSRL_REG_FOURIER");
RSRL_TRAIT_FOURIER(X)
#undef X

// a register-family Fourier configuration (which excludes the order-7 wave family and HIVTreatment)
static inline bool is_reg_fourier(const rsrl_hip_config& cfg) {
    return cfg.basis == RSRL_FOURIER && for_reg_fourier(cfg.domain, cfg.order, [](auto) {});
}
// a ContinuousMountainCar configuration on one of its Fourier orders
static inline bool is_cmc_fourier(const rsrl_hip_config& cfg) {
    return cfg.basis == RSRL_FOURIER && cfg.domain == RSRL_CONTINUOUS_MOUNTAIN_CAR && for_cmc_order(cfg.order, [](auto) {});
}
}  // namespace rsrl
