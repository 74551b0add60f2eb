// kernels_tdac_lstd.hpp -- ActorCritic::tdac with an iLSTD critic, the agent of examples/tdac.rs, on the register-family Fourier orders:
//   ActorCritic::tdac / TDCritic   rsrl/src/control/ac.rs:32-52, :87-98, :108-114     driver rsrl/examples/tdac.rs (eval.handle, agent.handle, sample)
//   the V learner                  iLSTD::new(basis, alpha, gamma, n_updates) (prediction/lstd/ilstd.rs): kernels_lstd.hpp's LstdLane, f64
//   the actor                      Gibbs::standard(LFA::vector(basis, SGD(1.0), A)) = Softmax(tau), as in kernels_ac.hpp / kernels_tdac.hpp, f32
// Two agents per learner: iLSTD's f64 theta / A / mu (learner-major, kernels_lstd.hpp's layout) and the actor's preferences th f32[A][F][N] (the
// ctx's auxiliary matrix, what the ABI's policy side reads).  Per transition (s, a, r, s', term), in tdac.rs's order:
//     p       = softmax_stable(th^T phi32(s) / tau)                       (th BEFORE this step's update; the f32 features of the other register kernels)
//     iLSTD   LstdLane<F, LSTD_INCREMENTAL>::step on the f64 features     (terminal: pd = phi(s)); its delta is the step's diagnostic
//     critic  c = r - V'(s') (terminal: V' of the terminal state itself) | r + gamma*V'(s') - V'(s), V' = phi . theta with the UPDATED f64 theta,
//             every product rounded, summed in index order
//     actor   e = (float)(alpha * c), the one rounding out of f64;  th[:,b] += e*(1[b==a] - p_b)*phi32(s) for every b     (tdac_step's f32 expressions)
// There is no inner draw.  s' of a terminal transition is the terminal state (what rsrl_hip_domain_step reports): the driver loop projects it for
// the critic and projects the restart state afterwards, on terminal and truncated steps only.
//
// Layout: kernels_lstd.hpp's.  A learner is a group of G lanes, lane r < F owns row r of A, theta_r and mu_r; vectors travel through the group's LDS
// slice.  Lane b < A also owns column b of the actor (A <= 3 <= G everywhere): it evaluates its preference <th[:,b], phi32(s)> and its axpy with the
// single-column forms of kernels_tdac.hpp (tdac_probs_mem: the bits of the WBuf<A, ..> ones, which the model kernels of the policy side compute), the
// A preferences are exchanged by shuffle, and every lane of the group runs the same softmax and the same sample.  Every lane evaluates the whole f32
// projection (its bits are those of FourierReg::project only as a whole); lanes r >= A carry a copy of column A - 1 and never store it.
// TdacLstdLane::step is the ONE step both kernels below run: train, handle and the trait-granular loop give the same bits, and theta / A / mu / delta
// are the bits of an iLSTD ctx's on the same transitions whatever the actor is.
#pragma once

#include "kernels_lstd.hpp"
#include "kernels_tdac.hpp"

namespace rsrl {

template <int DOMAIN, int ORDER>
struct TdacLstdLane {
    using Bas = FourierReg<DOMAIN, ORDER>;
    static constexpr int A = Domain<DOMAIN>::A, F = Bas::F, G = LstdGroup<F>::G;
    static constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    using Phi = PhiBuf<F, PK>;
    static_assert(A <= G, "a lane per actor column");

    LstdLane<F, LSTD_INCREMENTAL> L;
    WBuf<1, F, PK> col;                                   // the actor's column min(r, A - 1)

    __device__ __forceinline__ static int column(int r) { return r < A ? r : A - 1; }

    __device__ __forceinline__ void load(const TdacLstdState& ts, int64_t N, int64_t i, int r) {
        L.load(ts.ls, i, r);
        mat_load<1, F, PK>(col, ts.theta + (int64_t)column(r) * F * N, N, i);
    }
    __device__ __forceinline__ void store(const TdacLstdState& ts, int64_t N, int64_t i, int r) const {
        L.store(ts.ls, i, r);
        if (r < A) mat_store<1, F, PK>(col, ts.theta + (int64_t)r * F * N, N, i);
    }

    // pi_th(s) = softmax(th^T phi / tau): lane b's preference, handed round the group
    __device__ __forceinline__ void probs(const Common& c, const Phi& phi, float (&p)[A]) const {
        float hb[1];
        col.q(phi, hb);
        float h[A];
#pragma unroll
        for (int b = 0; b < A; ++b) h[b] = __shfl(hb[0], b, G);
        softmax_probs<A>(h, c.pol.tau, p);
    }

    // one transition of the lane's learner.  phs / phn: this lane's f64 features of s and s' (s' the terminal state itself on a terminal transition);
    // phi_s: the f32 features of s; p_s = pi_th(s) with the pre-update th; lv: the group's LDS vectors, lv[LV_PHS] already holds phi(s) of every lane.
    // Returns iLSTD's diagnostic delta.
    __device__ __forceinline__ double step(const Common& c, const TdacLstdState& ts, double (*lv)[F], int r, double phs, double phn, const Phi& phi_s,
                                           const float (&p_s)[A], int a, double rew, bool term) {
        // ---- iLSTD::handle
        const double delta = L.template step<G>(ts.ls, lv, r, phs, phn, rew, term);
        // ---- TDCritic::target with the updated theta
        const float e = (float)(ts.alpha * tdcritic_target<F>(L.theta, ts.ls.gamma, lv, r, phs, phn, rew, term));
        // ---- the actor: this lane's column
        const int bb = column(r);
        float pb = p_s[0];
#pragma unroll
        for (int b = 1; b < A; ++b) pb = (bb == b) ? p_s[b] : pb;
        const float sb[1] = {e * (((a == bb) ? 1.0f : 0.0f) - pb)};      // grad_log: (1[b==a] - p_b) phi(s)
        col.axpy(sb, phi_s);
        return delta;
    }
};

// the driver loop (tdac.rs): transition, iLSTD, critic + actor, then the behaviour sample a' ~ pi_th'(s') with the UPDATED th (BLK_STEP; an episode
// cut by max_episode_steps restarts and samples there on BLK_RESET, a terminal one restarts before the sample), as k_train_tdac.  Every lane of a
// group steps the learner's environment and draws the sample (the same bits in each); the rows and the columns stay in registers for the whole
// launch, and the sample's probabilities are the next step's p (th does not move in between): one f32 projection and one softmax per
// non-terminal step.  (A bound of two waves per SIMD -- what k_train_lstd reaches up to order 4 -- spills here: 100 to 432 B of scratch at F = 16 and 25)
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_train_tdac_lstd(Common c, TdacLstdState ts, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Dom = Domain<DOMAIN>;
    using Lane = TdacLstdLane<DOMAIN, ORDER>;
    using Bas = typename Lane::Bas;
    using Phi = typename Lane::Phi;
    constexpr int D = Dom::D, A = Lane::A, F = Lane::F, G = Lane::G;
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
        int a = c.action[i];
        uint32_t ep = c.ep_step[i];
        Lane ln;
        ln.load(ts, N, i, r);
        double phs = lstd_feature<DOMAIN, ORDER>(s, r);
        Phi phi_s;
        float p_s[A];
        ac_project<Bas>(s, phi_s);
        ln.probs(c, phi_s, p_s);
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
            double phn = lstd_feature<DOMAIN, ORDER>(ns, r);          // s' itself, the terminal state included: TDCritic reads V(s')
            const double delta = ln.step(c, ts, lv, r, phs, phn, phi_s, p_s, a, (double)rw, term);
            acc_abs += fabs(delta); acc_r += (double)rw;
            uint32_t blk = BLK_STEP;
            if (term) { n_ep += 1; sum_len += ep; ep = 0; }
            if (trunc) { n_ep += 1; n_trunc += 1; sum_len += ep; ep = 0; blk = BLK_RESET; }
            if (term || trunc) {                                      // the restart state is where the sample is taken
                Dom::reset(ns);
                phn = lstd_feature<DOMAIN, ORDER>(ns, r);
            }
            // ---- policy.sample(rng, s') with the UPDATED th
            ac_project<Bas>(ns, phi_s);
            ln.probs(c, phi_s, p_s);
            const U4 x = draw(c.seed, gid, t, blk);
            a = sample_probs<A>(p_s, x.z);
#pragma unroll
            for (int d = 0; d < D; ++d) s[d] = ns[d];
            phs = phn;
            lstd_wave_sync();                             // (this step's reads of the slice before the next step's writes)
        }
        ln.store(ts, N, i, r);
        if (r == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
            c.action[i] = a;
            c.ep_step[i] = ep;
            sum_abs = acc_abs; sum_r = acc_r;
        } else {
            n_ep = 0; n_trunc = 0; sum_len = 0;
        }
    }
    if (stats) block_stats_accumulate(stats, n_ep, n_trunc, sum_len, sum_abs, sum_r);
}

// iLSTD::handle then ActorCritic::handle (tdac.rs's order) on caller-supplied transitions: transition i is learner i's
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_handle_tdac_lstd(Common c, TdacLstdState ts, const float* __restrict__ from, const int32_t* __restrict__ act,
                                                             const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                             int64_t Mn, float* __restrict__ td_out) {
    using Dom = Domain<DOMAIN>;
    using Lane = TdacLstdLane<DOMAIN, ORDER>;
    using Bas = typename Lane::Bas;
    constexpr int D = Dom::D, A = Lane::A, F = Lane::F;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LV_N][F];
    const auto g = GroupId<F, LV_N>::here();
    const int r = g.r;
    if (g.i >= Mn) return;
    double (*lv)[F] = g.slice(lds);
    GroupGiven<D> tr;
    tr.load(from, to, termf, Mn, g.i);
    const int a = clamp_action<A>(act[g.i]);
    Lane ln;
    ln.load(ts, c.n_envs, g.i, r);
    const double phs = lstd_feature<DOMAIN, ORDER>(tr.s, r);
    const double phn = lstd_feature<DOMAIN, ORDER>(tr.ns, r);
    typename Lane::Phi phi_s;
    float p_s[A];
    ac_project<Bas>(tr.s, phi_s);
    ln.probs(c, phi_s, p_s);
    if (g.own()) lv[LV_PHS][r] = phs;
    const double delta = ln.step(c, ts, lv, r, phs, phn, phi_s, p_s, a, (double)rew[g.i], tr.term);
    ln.store(ts, c.n_envs, g.i, r);
    g.report(td_out, delta);
}

}  // namespace rsrl
