// kernels_cacla.hpp -- CACLA (continuous actor-critic learning automaton) over the Gaussian policy with a TD(0) state-value critic on
// ContinuousMountainCar:
//   CACLA::handle           rsrl/src/control/cacla.rs:42-64     critic: a closure over V, read and never written; policy; alpha; gamma
//   the V learner           TD{v_func = ScalarLFA(basis, SGD(lr)), gamma} (prediction/td/td.rs:38-58): the caller's `eval`, trained before the agent sees
//                           the transition (the order of tdac.rs, tdac_beta.rs and nac.rs; the reference has no example for CACLA)
//   the policy              Gaussian over a ScalarLFA and a Composition<ScalarLFA, Softplus>: kernels_gaussian.hpp's device functions, unchanged;
//                           Gaussian::handle(StateActionUpdate) is policies/gaussian/general.rs:196-212
// Three one-column approximators per learner: the V learner's w f32[F][N] (the ctx's weights, TD's layout) and the policy's two columns w_m, w_s
// f32[2][F][N] (the ctx's auxiliary matrix).  One thread per learner with w, w_m, w_s, phi(s) and phi(s') in registers (5F floats, 180 at order 5):
// k_train_nac_gauss's layout and launch bounds.  Per transition (s, a, r, s', term), all f32, in this order:
//     1.  x_m = <w_m, phi(s)>, x_s = <w_s, phi(s)>
//     2.  TD::handle, tdac_step's expressions:   v_s = <w, phi(s)>, v_n = <w, phi(s')>;  td = r - v_s (terminal) | r + gamma * v_n - v_s;
//                                                w += (lr * td) phi(s), one fma per element
//     3.  with the UPDATED w:   v = <w, phi(s)>;  target = r (terminal: r alone, not r - V(s')) | r + gamma * <w, phi(s')>;   gate = target > v
//         (strict; a NaN on either side closes it)
//     4.  gate open only:   (mu, sd) = gauss_params(x_m, x_s);  e = (a - mu) * alpha;  (c_m, c_s) = gauss_coef(x_s, mu, sd, a);
//                           w_m += (e * c_m) phi(s);  w_s += (e * c_s) phi(s)
// A closed gate leaves both columns' BITS as they were, whatever the coefficients would have been (they are not even computed): the update sits
// behind the gate itself, never behind a product with 0 -- fma(0, phi, -0.0) is +0.0, and 0 * inf a NaN.
// THE LITERAL RULE: the mean's step is e * c_m = alpha (a - mu)^2 / Sigma >= 0 whatever side of the mean the action lay on -- the reference hands the
// policy `error: (a - mode) * alpha` and the policy multiplies it by its score once more.  This is not van Hasselt's mu += alpha (a - mu); it is what
// cacla.rs and general.rs say, and it is built as they say it.  There is no safeguard: sd is floored at 0.01 only, so the coefficients reach 1e4.
// There is no inner draw.  cacla_step is the ONE step both kernels below run: train, handle and the trait-granular loop give the same bits, and w / td
// are the bits of a TD ctx's on the same transitions whatever the columns are.
// The step holds no data-dependent loop, no shuffle and no LDS access.
#pragma once

#include "kernels_gaussian.hpp"

namespace rsrl {

// one transition on projected phi(s), phi(s').  Returns TD's error; `gate`: whether the policy moved
template <int F, bool PK>
__device__ __forceinline__ float cacla_step(const Common& c, WBuf<1, F, PK>& w, WBuf<2, F, PK>& pol, const PhiBuf<F, PK>& phi_s, const PhiBuf<F, PK>& phi_n, float a,
                                            float r, bool term, bool& gate) {
    const float gamma = c.alg.gamma, lr = c.alg.lr;
    float x[2];
    pol.q(phi_s, x);
    // ---- TD::handle (the expressions of k_train_td / k_handle_td, as tdac_step states them)
    float v_s[1], v_n[1];
    w.q(phi_s, v_s);
    w.q(phi_n, v_n);
    const float td = term ? (r - v_s[0]) : (r + gamma * v_n[0] - v_s[0]);
    const float sb[1] = {lr * td};
    w.axpy(sb, phi_s);
    // ---- CACLA::handle: the critic closure reads the updated V
    w.q(phi_s, v_s);
    w.q(phi_n, v_n);
    const float target = term ? r : (r + gamma * v_n[0]);
    gate = target > v_s[0];
    if (gate) {
        float mu, sd, cm, cs;
        gauss_params(x[0], x[1], mu, sd);
        const float e = (a - mu) * c.alg.alpha;
        gauss_coef(x[1], mu, sd, a, cm, cs);
        const float sp[2] = {e * cm, e * cs};
        pol.axpy(sp, phi_s);
    }
    return td;
}

// the driver loop: transition on the action itself (the domain clips it), eval.handle, agent.handle, then the behaviour sample a' ~ N(mu, sd^2) with
// the UPDATED columns, after the restart when the episode ended, terminal or cut (restart_then_sample's convention; BLK_STEP, BLK_RESET is its
// alias).  s' is projected as it is, the terminal state included (TD does not read it there, and neither does the gate); phi(s') becomes the next
// step's phi(s) (two buffers that swap roles) unless the episode ended: then the restart state is projected in its place.  The statistics' sum
// |delta| is TD's
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_train_cacla(Common c, CaclaState st, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Dom = Domain<kCmc>;
    using Bas = FourierReg<kCmc, ORDER>;
    constexpr int D = Dom::D, F = Bas::F;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    using Phi = PhiBuf<F, PK>;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    Tally tally;
    if (i < N) {
        const uint32_t gid = (uint32_t)(c.env_offset + i);
        const uint32_t cap = c.max_episode_steps;
        float s[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = c.state[(int64_t)d * N + i];
        float a = st.action[i];
        uint32_t ep = c.ep_step[i];
        WBuf<1, F, PK> w;
        WBuf<2, F, PK> pol;
        mat_load<1, F, PK>(w, c.W, N, i);
        mat_load<2, F, PK>(pol, st.pol, N, i);
        Phi phi_a, phi_b;
        ac_project<Bas>(s, phi_a);

        ping_pong(phi_a, phi_b, t0, n_steps, [&](const Phi& phi_s, Phi& phi_n, uint64_t t) {
            float rw;
            const bool term = Dom::step(s, a, rw);                    // s <- s' (the domain clips the action: map_onto)
            ep += 1;
            const bool trunc = !term && cap > 0 && ep >= cap;
            ac_project<Bas>(s, phi_n);
            bool gate;
            const float td = cacla_step<F, PK>(c, w, pol, phi_s, phi_n, a, rw, term, gate);
            if (term || trunc) {                                      // the restart state is where the sample is taken
                tally.episode_end(ep, trunc);
                Dom::reset(s);
                ac_project<Bas>(s, phi_n);
            }
            float x[2], mu, sd;
            pol.q(phi_n, x);
            gauss_params(x[0], x[1], mu, sd);
            a = gauss_sample(c.seed, gid, t, BLK_STEP, mu, sd);
            tally.step(td, rw);
        });
#pragma unroll
        for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
        st.action[i] = a;
        c.ep_step[i] = ep;
        mat_store<1, F, PK>(w, c.W, N, i);
        mat_store<2, F, PK>(pol, st.pol, N, i);
    }
    tally.hand_over(stats);
}

// eval.handle then CACLA::handle on caller-supplied transitions: transition i is learner i's.  The columns are stored by the learners whose gate
// opened only
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_handle_cacla(Common c, CaclaState st, const float* __restrict__ from, const float* __restrict__ act,
                                                         const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                         int64_t Mn, float* __restrict__ td_out) {
    using Bas = FourierReg<kCmc, ORDER>;
    constexpr int D = Domain<kCmc>::D, F = Bas::F;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const int64_t N = c.n_envs;
    Given<D> tr;
    tr.load(from, rew, to, termf, Mn, i);
    PhiBuf<F, PK> phi_s, phi_n;
    ac_project<Bas>(tr.s, phi_s);
    ac_project<Bas>(tr.ns, phi_n);
    WBuf<1, F, PK> w;
    WBuf<2, F, PK> pol;
    mat_load<1, F, PK>(w, c.W, N, i);
    mat_load<2, F, PK>(pol, st.pol, N, i);
    bool gate;
    const float td = cacla_step<F, PK>(c, w, pol, phi_s, phi_n, act[i], tr.r, tr.term, gate);
    mat_store<1, F, PK>(w, c.W, N, i);
    if (gate) mat_store<2, F, PK>(pol, st.pol, N, i);
    if (td_out) td_out[i] = td;
}

}  // namespace rsrl
