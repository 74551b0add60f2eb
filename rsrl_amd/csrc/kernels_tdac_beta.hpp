// kernels_tdac_beta.hpp -- ActorCritic::tdac with an iLSTD critic and a Beta policy on ContinuousMountainCar, the agent of examples/tdac_beta.rs:
//   the domain                     rsrl_domains/src/mountain_car/continuous.rs: Domain<4> (device_core.hpp), one f32 action in [-1, 1]
//   ActorCritic::tdac / TDCritic   rsrl/src/control/ac.rs; the V learner iLSTD (prediction/lstd/ilstd.rs): kernels_tdac_lstd.hpp's critic half, unchanged
//   the actor                      Beta (rsrl/src/policies/beta.rs) over two Composition<ScalarLFA, Softplus> (fa/composition.rs:98-115, fa/transforms.rs:196-218)
// Per learner: iLSTD's f64 theta / A / mu (kernels_lstd.hpp's layout) and the policy's two weight columns w_a, w_b f32[2][F][N] (the ctx's auxiliary
// matrix: column 0 = alpha's, column 1 = beta's).  The policy's functions are cont_policy.hpp's; this loop hands the domain the action itself.
// Per transition (s, a, r, s', term), in tdac_beta.rs's order:
//     alpha, beta at s from the PRE-update columns
//     iLSTD   LstdLane<F, LSTD_INCREMENTAL>::step, the bits of an RSRL_ILSTD ctx's on the same transitions
//     critic  TdacLstdLane::step's target from the updated f64 theta (V of the terminal state itself on a terminal transition)
//     e       = (float)(ActorCritic.alpha * c), the one rounding out of f64
//     actor   w_a += e * g_a * sigma(x_a) * phi(s),  w_b += e * g_b * sigma(x_b) * phi(s)      (g the Beta score, sigma Softplus's gradient)
//
// Layout: kernels_tdac_lstd.hpp's.  Lane 0 of a learner's group owns w_a, lane 1 owns w_b (G >= 4 at every order; lanes >= 2 carry a copy of w_b and
// never store it); the two preferences are exchanged by shuffle before the scalar chain, which every lane runs.  TdacBetaLane::step is the ONE step
// both kernels below run.
#pragma once

#include "kernels_lstd.hpp"
#include "cont_policy.hpp"

namespace rsrl {

template <int ORDER>
struct TdacBetaLane {
    using Bas = FourierReg<kCmc, ORDER>;
    static constexpr int F = Bas::F, G = LstdGroup<F>::G;
    static constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    using Phi = PhiBuf<F, PK>;
    static_assert(G >= 2, "a lane per policy column");

    LstdLane<F, LSTD_INCREMENTAL> L;
    WBuf<1, F, PK> col;                                   // the policy's column min(r, 1)

    __device__ __forceinline__ static int column(int r) { return r < 1 ? 0 : 1; }

    __device__ __forceinline__ void load(const TdacBetaState& ts, int64_t N, int64_t i, int r) {
        L.load(ts.ls, i, r);
        mat_load<1, F, PK>(col, ts.w + (int64_t)column(r) * F * N, N, i);
    }
    __device__ __forceinline__ void store(const TdacBetaState& ts, int64_t N, int64_t i, int r) const {
        L.store(ts.ls, i, r);
        if (r < 2) mat_store<1, F, PK>(col, ts.w + (int64_t)r * F * N, N, i);
    }
    // x_a = <w_a, phi>, x_b = <w_b, phi>: lane b's preference, handed round the group
    __device__ __forceinline__ void prefs(const Phi& phi, float& xa, float& xb) const {
        float hb[1];
        col.q(phi, hb);
        xa = __shfl(hb[0], 0, G);
        xb = __shfl(hb[0], 1, G);
    }

    // one transition of the lane's learner (TdacLstdLane::step's arguments; xa, xb the preferences at s with the pre-update columns, a the action).
    // Returns iLSTD's diagnostic delta.
    __device__ __forceinline__ double step(const TdacBetaState& ts, double (*lv)[F], int r, double phs, double phn, const Phi& phi_s, float xa, float xb,
                                           float a, double rew, bool term) {
        // ---- iLSTD::handle
        const double delta = L.template step<G>(ts.ls, lv, r, phs, phn, rew, term);
        // ---- TDCritic::target with the updated theta
        const float e = (float)(ts.alpha * tdcritic_target<F>(L.theta, ts.ls.gamma, lv, r, phs, phn, rew, term));
        // ---- the actor: this lane's column
        float alpha, beta;
        beta_params(xa, xb, alpha, beta);
        const float ac = beta_clamp(a);
        const float psi_ab = digamma_dev(alpha + beta);
        const float g_a = logf(ac) - digamma_dev(alpha) + psi_ab;
        const float g_b = logf(1.0f - ac) - digamma_dev(beta) + psi_ab;
        const float s_a = e * g_a * softplus_grad_dev(xa);
        const float s_b = e * g_b * softplus_grad_dev(xb);
        const float sb[1] = {r < 1 ? s_a : s_b};
        col.axpy(sb, phi_s);
        return delta;
    }
};

// the driver loop (tdac_beta.rs), modelled on k_train_tdac_lstd: transition, iLSTD, critic + actor, then the behaviour sample a' ~ Beta(alpha, beta)(s')
// with the UPDATED columns, taken after the restart (BLK_STEP; BLK_RESET after a cut episode is its alias).  The sample's preferences are the next step's
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_train_tdac_beta(Common c, TdacBetaState ts, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Dom = Domain<kCmc>;
    using Lane = TdacBetaLane<ORDER>;
    using Bas = typename Lane::Bas;
    using Phi = typename Lane::Phi;
    constexpr int D = Dom::D, F = Lane::F, G = Lane::G;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LV_N][F];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = tid / G;
    const int r = (int)(tid % G);
    const int64_t N = c.n_envs;
    unsigned long long n_ep = 0, n_trunc = 0, sum_len = 0;
    double sum_abs = 0.0, sum_r = 0.0;
    if (i < N) {
        double (*lv)[F] = lds[threadIdx.x / G];
        const uint32_t gid = (uint32_t)(c.env_offset + i);
        const uint32_t cap = c.max_episode_steps;
        float s[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = c.state[(int64_t)d * N + i];
        float a = ts.action[i];
        uint32_t ep = c.ep_step[i];
        Lane ln;
        ln.load(ts, N, i, r);
        double phs = lstd_feature<kCmc, ORDER>(s, r);
        Phi phi_s;
        float xa, xb;
        ac_project<Bas>(s, phi_s);
        ln.prefs(phi_s, xa, xb);
        double acc_abs = 0.0, acc_r = 0.0;
        for (int k = 0; k < n_steps; ++k) {
            const uint64_t t = t0 + (uint64_t)k;
            if (r < F) lv[LV_PHS][r] = phs;
            float ns[D];
#pragma unroll
            for (int d = 0; d < D; ++d) ns[d] = s[d];
            float rw;
            const bool term = Dom::step(ns, a, rw);
            ep += 1;
            const bool trunc = !term && cap > 0 && ep >= cap;
            double phn = lstd_feature<kCmc, ORDER>(ns, r);            // s' itself, the terminal state included: TDCritic reads V(s')
            const double delta = ln.step(ts, lv, r, phs, phn, phi_s, xa, xb, a, (double)rw, term);
            acc_abs += fabs(delta); acc_r += (double)rw;
            if (term) { n_ep += 1; sum_len += ep; ep = 0; }
            if (trunc) { n_ep += 1; n_trunc += 1; sum_len += ep; ep = 0; }
            if (term || trunc) {                                      // the restart state is where the sample is taken
                Dom::reset(ns);
                phn = lstd_feature<kCmc, ORDER>(ns, r);
            }
            // ---- policy.sample(rng, s') with the UPDATED columns
            ac_project<Bas>(ns, phi_s);
            ln.prefs(phi_s, xa, xb);
            float alpha, beta;
            beta_params(xa, xb, alpha, beta);
            a = beta_sample(c.seed, gid, t, BLK_STEP, alpha, beta);
#pragma unroll
            for (int d = 0; d < D; ++d) s[d] = ns[d];
            phs = phn;
            lstd_wave_sync();                             // (this step's reads of the slice before the next step's writes)
        }
        ln.store(ts, N, i, r);
        if (r == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
            ts.action[i] = a;
            c.ep_step[i] = ep;
            sum_abs = acc_abs; sum_r = acc_r;
        } else {
            n_ep = 0; n_trunc = 0; sum_len = 0;
        }
    }
    if (stats) block_stats_accumulate(stats, n_ep, n_trunc, sum_len, sum_abs, sum_r);
}

// iLSTD::handle then ActorCritic::handle (tdac_beta.rs's order) on caller-supplied transitions: transition i is learner i's
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_handle_tdac_beta(Common c, TdacBetaState ts, const float* __restrict__ from, const float* __restrict__ act,
                                                             const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                             int64_t Mn, float* __restrict__ td_out) {
    using Dom = Domain<kCmc>;
    using Lane = TdacBetaLane<ORDER>;
    using Bas = typename Lane::Bas;
    constexpr int D = Dom::D, F = Lane::F;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LV_N][F];
    const auto g = GroupId<F, LV_N>::here();
    const int r = g.r;
    if (g.i >= Mn) return;
    double (*lv)[F] = g.slice(lds);
    GroupGiven<D> tr;
    tr.load(from, to, termf, Mn, g.i);
    const float a = act[g.i];
    Lane ln;
    ln.load(ts, c.n_envs, g.i, r);
    const double phs = lstd_feature<kCmc, ORDER>(tr.s, r);
    const double phn = lstd_feature<kCmc, ORDER>(tr.ns, r);
    typename Lane::Phi phi_s;
    float xa, xb;
    ac_project<Bas>(tr.s, phi_s);
    ln.prefs(phi_s, xa, xb);
    if (g.own()) lv[LV_PHS][r] = phs;
    const double delta = ln.step(ts, lv, r, phs, phn, phi_s, xa, xb, a, (double)rew[g.i], tr.term);
    ln.store(ts, c.n_envs, g.i, r);
    g.report(td_out, delta);
}

}  // namespace rsrl
