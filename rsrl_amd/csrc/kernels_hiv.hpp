// kernels_hiv.hpp -- HIVTreatment (rsrl_domains/src/hiv.rs), the one domain whose transition is integrated in f64: 1 000 classical RK4 sub-steps
// of a 6-D ODE per env-step.  Only the kernels of train_hiv.hip include this header (their own translation unit: no other kernel's code moves).
//
// The ctx keeps every learner's hidden state y = [T1, T1*, T2, T2*, V, E] as f64[6][N] (learner fastest, hiv.rs:42-52); the f32 env state of the
// ctx (Common::state) is its observation clip(-5, log10 y, 8) (hiv.rs:112-119), the input of the Fourier basis.  The integration is IEEE f64
// in the reference's operation order (the build passes -ffp-contract=off and no fast-math flag), so the hidden state is the reference's bit for bit.
#pragma once

#include "models.hpp"

namespace rsrl {

// The feature model's view of the domain (FourierGenericModel<3>): six observation dimensions on [-5, 8] (hiv.rs:137-145), four actions.
// Deliberately NO f32 reset / step: a driver-loop template of the other domains instantiated for HIV fails to compile instead of silently
// running without the hidden state.
template <> struct Domain<3> {
    static constexpr int D = 6, A = 4;
    __host__ __device__ static constexpr double lo_d(int) { return -5.0; }     // LIMITS (hiv.rs:34)
    __host__ __device__ static constexpr double hi_d(int) { return 8.0; }
};

namespace hiv {

constexpr int D = 6, A = 4;
constexpr int kSimSteps = 1000;                         // SIM_STEPS (hiv.rs:29)
constexpr double kDtStep = 5.0 / 1000.0;                // DT_STEP = DT / SIM_STEPS as f64 (:28-31)
// HIVTreatment::default() (:102-106)
__host__ __device__ constexpr double default_y(int i) {
    return i == 0 ? 163573.0 : i == 1 ? 11945.0 : i == 2 ? 5.0 : i == 3 ? 46.0 : i == 4 ? 63919.0 : 24.0;
}
// ALL_ACTIONS[a] = [0,0] [0.7,0] [0,0.3] [0.7,0.3] (:35): eps0 is bit 0 of the action, eps1 bit 1
__host__ __device__ constexpr double eps0_of(int a) { return (a & 1) ? 0.7 : 0.0; }
__host__ __device__ constexpr double eps1_of(int a) { return (a & 2) ? 0.3 : 0.0; }

// the model parameters (:5-25)
constexpr double LAMBDA1 = 1e4, LAMBDA2 = 31.98, D1 = 0.01, D2 = 0.01, F = 0.34, K1 = 8e-7, K2 = 1e-4, DELTA = 0.7, M1 = 1e-5, M2 = 1e-5;
constexpr double NT = 100.0, C = 13.0, RHO1 = 1.0, RHO2 = 1.0, LAMBDA_E = 1.0, BE = 0.3, KB = 100.0, DE = 0.25, KD = 500.0, DELTA_E = 0.1;

// The action-dependent prefactors of grad (:73-100), each the left-to-right product the reference forms first in its expression -- e.g.
// tmp1 = (1.0 - eps0) * K1 * v * t1 is ((c1 * v) * t1) with c1 = (1.0 - eps0) * K1.  Formed once per env-step from the same operands in the same
// order: the same bits as forming them in every gradient.
struct Coef { double c1, c2, cv, cr1, cr2; };
__device__ __forceinline__ Coef coef(int a) {
    const double e0 = eps0_of(a), e1 = eps1_of(a);
    Coef k;
    k.c1 = (1.0 - e0) * K1;
    k.c2 = (1.0 - F * e0) * K2;
    k.cv = ((1.0 - e1) * NT) * DELTA;
    k.cr1 = ((1.0 - e0) * RHO1) * K1;
    k.cr2 = ((1.0 - F * e0) * RHO2) * K2;
    return k;
}

// HIVTreatment::grad (:73-100), operation for operation.  The two Michaelis-Menten quotients of E' stay IEEE divisions.
__device__ __forceinline__ void grad(const Coef& k, const double (&y)[D], double (&o)[D]) {
    const double t1 = y[0], t1s = y[1], t2 = y[2], t2s = y[3], v = y[4], e = y[5];
    const double tmp1 = (k.c1 * v) * t1;
    const double tmp2 = (k.c2 * v) * t2;
    const double sum_ts = t1s + t2s;
    o[0] = (LAMBDA1 - D1 * t1) - tmp1;
    o[1] = (tmp1 - DELTA * t1s) - (M1 * e) * t1s;
    o[2] = (LAMBDA2 - D2 * t2) - tmp2;
    o[3] = (tmp2 - DELTA * t2s) - (M2 * e) * t2s;
    o[4] = (k.cv * sum_ts - C * v) - ((k.cr1 * t1) + (k.cr2 * t2)) * v;
    o[5] = ((LAMBDA_E + ((BE * sum_ts) / (sum_ts + KB)) * e) - ((DE * sum_ts) / (sum_ts + KD)) * e) - DELTA_E * e;
}

// runge_kutta4 (ode.rs:1-43) with dx = DT_STEP; the time argument is unused by grad.  b / 2.0 is the exact product b * 0.5; the final / 6.0
// stays an IEEE division (no replacement proven correctly rounded for every f64 input).
__device__ __forceinline__ void rk4_step(const Coef& k, double (&y)[D]) {
    double k1[D], k2[D], k3[D], k4[D], t[D];
    grad(k, y, k1);
#pragma unroll
    for (int i = 0; i < D; ++i) { k1[i] = k1[i] * kDtStep; t[i] = y[i] + k1[i] / 2.0; }
    grad(k, t, k2);
#pragma unroll
    for (int i = 0; i < D; ++i) { k2[i] = k2[i] * kDtStep; t[i] = y[i] + k2[i] / 2.0; }
    grad(k, t, k3);
#pragma unroll
    for (int i = 0; i < D; ++i) { k3[i] = k3[i] * kDtStep; t[i] = y[i] + k3[i]; }
    grad(k, t, k4);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        k4[i] = k4[i] * kDtStep;
        y[i] += (((k1[i] + 2.0 * k2[i]) + 2.0 * k3[i]) + k4[i]) / 6.0;
    }
}

// HIVTreatment::update_state (:54-71): SIM_STEPS sub-steps under the action's treatment
__device__ __forceinline__ void integrate(double (&y)[D], int a) {
    const Coef k = coef(a);
#pragma unroll 1
    for (int s = 0; s < kSimSteps; ++s) rk4_step(k, y);
}

// emit (:112-119): clip!(-5, log10 y_i, 8) = (-5).max(8.min(log10 y_i)) in f64 -- f64::min / max return the other operand for a NaN, as fmin / fmax
// do -- rounded once to f32 for the feature model
__device__ __forceinline__ void observe(const double (&y)[D], double (&obs)[D], float (&s)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) { obs[i] = fmax(-5.0, fmin(8.0, log10(y[i]))); s[i] = (float)obs[i]; }
}
// step's reward (:121-135), from the OBSERVATION: (1e3 E - 0.1 V - 2e4 eps0^2 - 2e3 eps1^2) / 1e5 in f64 (powi(2) is x * x), rounded once to f32
__device__ __forceinline__ float reward(const double (&obs)[D], int a) {
    const double e0 = eps0_of(a), e1 = eps1_of(a);
    const double r = ((1e3 * obs[5] - 0.1 * obs[4]) - 2e4 * (e0 * e0)) - 2e3 * (e1 * e1);
    return (float)(r / 1e5);
}
// Domain::step: integrate, emit, reward.  emit is always Observation::Full: HIV has no terminal state.
__device__ __forceinline__ float step(double (&y)[D], float (&s)[D], int a) {
    integrate(y, a);
    double obs[D];
    observe(y, obs, s);
    return reward(obs, a);
}
__device__ __forceinline__ void reset(double (&y)[D], float (&s)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) y[i] = default_y(i);
    double obs[D];
    observe(y, obs, s);
}
__device__ __forceinline__ void load(const double* __restrict__ Y, int64_t N, int64_t i, double (&y)[D]) {
#pragma unroll
    for (int d = 0; d < D; ++d) y[d] = Y[(int64_t)d * N + i];
}
__device__ __forceinline__ void store(double* __restrict__ Y, int64_t N, int64_t i, const double (&y)[D]) {
#pragma unroll
    for (int d = 0; d < D; ++d) Y[(int64_t)d * N + i] = y[d];
}

}  // namespace hiv
}  // namespace rsrl
