// model_list.hpp -- the (basis, domain, parameter) -> Model type table shared by the translation units that dispatch over it.
//   Fourier register family: F = (order+1)^D <= 36 features per learner held in VGPRs (FourierModel).
//   Tile coding: T tilings as a template parameter (indices in VGPRs), tiles_per_dim at run time (TileModel).
//   param -1: the generic-order Fourier model (any order 1..7 without a specialised kernel; listed last).
// Model lookup is first match: the RSRL_REG_FOURIER rows, then RSRL_MEM_MODELS (ctx.hpp for_model).
#pragma once

#include "../../include/rsrl_hip.h"
#include "models.hpp"

// the register-family Fourier (domain, order) pairs, in the order every launcher instantiates them (moving one moves the
// PC-relative offsets of the others' machine code).  The models of the Fourier rows: FourierModel<domain, order>
#define RSRL_REG_FOURIER(X) X(0, 1) X(0, 2) X(0, 3) X(0, 4) X(0, 5) X(1, 1) X(2, 1)
// ContinuousMountainCar (domain 4, f32 actions): the Fourier orders its one agent runs on (train_tdac_beta.hip) -- MountainCar's register-family
// orders, with MountainCar's features.  NOT rows of RSRL_REG_FOURIER: no model kernel (an index action per learner) is instantiated for it
#define RSRL_CMC_ORDERS(X) X(1) X(2) X(3) X(4) X(5)
// the models WITHOUT a register-family kernel of their own (what the *_mem agent kernels are instantiated for)
#define RSRL_MEM_MODELS(X)                                                                   \
    X((TileModel<0, 4>), RSRL_TILE_CODING, 0, 4) X((TileModel<0, 8>), RSRL_TILE_CODING, 0, 8) X((TileModel<0, 16>), RSRL_TILE_CODING, 0, 16) \
    X((TileModel<1, 4>), RSRL_TILE_CODING, 1, 4) X((TileModel<1, 8>), RSRL_TILE_CODING, 1, 8) X((TileModel<1, 16>), RSRL_TILE_CODING, 1, 16) \
    X((TileModel<2, 4>), RSRL_TILE_CODING, 2, 4) X((TileModel<2, 8>), RSRL_TILE_CODING, 2, 8) X((TileModel<2, 16>), RSRL_TILE_CODING, 2, 16) \
    X((FourierGenericModel<0>), RSRL_FOURIER, 0, -1) X((FourierGenericModel<1>), RSRL_FOURIER, 1, -1) X((FourierGenericModel<2>), RSRL_FOURIER, 2, -1)

namespace rsrl {
template <class T> struct Tag { using type = T; };
#define RSRL_UNPAREN(...) __VA_ARGS__
static inline bool model_match(const rsrl_hip_config& cfg, int basis, int domain, int param) {
    if (cfg.basis != basis || cfg.domain != domain) return false;
    if (param == -1) return cfg.order >= 1 && cfg.order <= 7;
    return (basis == RSRL_FOURIER ? cfg.order : cfg.n_tilings) == param;
}
// a register-family Fourier configuration (which excludes the order-7 wave family and HIVTreatment)
static inline bool is_reg_fourier(const rsrl_hip_config& cfg) {
#define X(DM, OR) if (model_match(cfg, RSRL_FOURIER, DM, OR)) return true;
    RSRL_REG_FOURIER(X)
#undef X
    return false;
}
// a ContinuousMountainCar configuration on one of its Fourier orders
static inline bool is_cmc_fourier(const rsrl_hip_config& cfg) {
#define X(OR) if (model_match(cfg, RSRL_FOURIER, RSRL_CONTINUOUS_MOUNTAIN_CAR, OR)) return true;
    RSRL_CMC_ORDERS(X)
#undef X
    return false;
}
}  // namespace rsrl
