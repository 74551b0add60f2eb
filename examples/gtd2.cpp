// examples/gtd2.cpp -- gradient-TD prediction on the HIP path: GTD2 (or TDC) learns V of the uniform Random policy on MountainCar with
// Fourier(order).with_bias(), N environments at once, episodes capped at `cap` steps.  Two ScalarLFAs on one basis: theta is the value function
// (Session::weights), w the correction's estimator (Session::td_weights).  The reference has no example for these agents (rsrl/examples holds control agents
// only); this one follows examples/gradient_mc.cpp.  The reference applies theta's updates past the optimiser, with step size
// 1, which diverges on a Fourier basis: here the first LFA's rate scales theta's moves and the second's w's (include/rsrl_hip.h, RSRL_GTD2).
// After the fused loop one transition per learner is taken by hand (transition, handle), the reference's own calls.
//
//   g++ -std=c++17 -O2 examples/gtd2.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o gtd2
//   ./gtd2 [n_envs] [batches] [steps per batch] [order] [cap] [tdc: 0 | 1]
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../rsrl_amd/host/rsrl.hpp"

using namespace rsrl;

static double max_abs(const std::vector<float>& v) {
    double m = 0;
    for (float x : v) m = std::fabs(x) > m ? std::fabs(x) : m;
    return m;
}

int main(int argc, char** argv) {
    const int64_t n_envs = argc > 1 ? atoll(argv[1]) : 64;
    const int batches = argc > 2 ? atoi(argv[2]) : 5;
    const int steps = argc > 3 ? atoi(argv[3]) : 1000;
    const int order = argc > 4 ? atoi(argv[4]) : 3;
    const uint32_t cap = argc > 5 ? (uint32_t)atoi(argv[5]) : 200;
    const bool tdc = argc > 6 && atoi(argv[6]) != 0;

    domains::MountainCar env(n_envs);
    auto basis = fa::linear::basis::Fourier::from_space(order, env).with_bias();
    auto fa_theta = make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(0.005), 1));
    auto fa_w = fa::linear::LFA::vector(basis, fa::linear::optim::SGD(0.01), 1);
    policies::Random policy(3);
    const control::td::Agent agent = tdc ? (control::td::Agent)prediction::td::TDC(fa_theta, fa_w, 0.99)
                                         : (control::td::Agent)prediction::td::GTD2(fa_theta, fa_w, 0.99);

    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/cap);
    sess.reset();
    for (int e = 0; e < batches; ++e) {
        auto st = sess.train(steps);
        printf("Batch %d: %llu episodes finished (%llu truncated), mean reward %.4f, mean |td| %.4g\n", e + 1, (unsigned long long)st.episodes,
               (unsigned long long)st.episodes_truncated, st.sum_reward / (double)st.env_steps, st.sum_abs_td_error / (double)st.env_steps);
    }

    // one transition per learner by hand: agent.handle(&t) returns the TD error and moves both columns
    const std::vector<float> th0 = sess.weights(0), w0 = sess.td_weights(0);
    domains::Transition t = sess.transition(sess.sample());
    const std::vector<float> td = sess.handle(t);
    const std::vector<float> th1 = sess.weights(0), w1 = sess.td_weights(0);
    double moved_th = 0, moved_w = 0;
    for (size_t f = 0; f < th1.size(); ++f) {
        moved_th = std::fabs(th1[f] - th0[f]) > moved_th ? std::fabs(th1[f] - th0[f]) : moved_th;
        moved_w = std::fabs(w1[f] - w0[f]) > moved_w ? std::fabs(w1[f] - w0[f]) : moved_w;
    }
    printf("%s: one transition handled, td of learner 0 %.6g; max |theta| of learner 0: %.6g (%zu weights), moved by %.3g; max |w| of learner 0: %.6g "
           "(%zu weights), moved by %.3g\n", tdc ? "TDC" : "GTD2", (double)td[0], max_abs(th1), th1.size(), moved_th, max_abs(w1), w1.size(), moved_w);
    return 0;
}
