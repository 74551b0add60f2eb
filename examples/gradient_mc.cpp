// examples/gradient_mc.cpp -- every-visit gradient Monte-Carlo prediction on the HIP path: GradientMC (lr 0.001, gamma 0.99) learns V of the uniform
// Random policy on MountainCar with Fourier(order).with_bias(), N environments at once, episodes capped at `cap` steps.  The fused loop records every
// learner's open episode on the device and, when it ends, walks it backwards: sum = r + gamma * sum, w += lr * (sum - V(s)) * phi(s).  Afterwards
// one trajectory per learner is collected by hand (transition, sample) and handed to agent.handle(&trajectory), the reference's own call.
//
//   g++ -std=c++17 -O2 examples/gradient_mc.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o gradient_mc
//   ./gradient_mc [n_envs] [batches] [steps per batch] [order] [cap]
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../rsrl_amd/host/rsrl.hpp"

using namespace rsrl;

int main(int argc, char** argv) {
    const int64_t n_envs = argc > 1 ? atoll(argv[1]) : 64;
    const int batches = argc > 2 ? atoi(argv[2]) : 5;
    const int steps = argc > 3 ? atoi(argv[3]) : 1000;
    const int order = argc > 4 ? atoi(argv[4]) : 3;
    const uint32_t cap = argc > 5 ? (uint32_t)atoi(argv[5]) : 200;

    domains::MountainCar env(n_envs);
    auto basis = fa::linear::basis::Fourier::from_space(order, env).with_bias();
    auto v_func = make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(0.001), 1));
    policies::Random policy(3);
    prediction::mc::GradientMC agent(v_func, 0.99);

    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/cap);
    sess.reset();
    for (int e = 0; e < batches; ++e) {
        auto st = sess.train(steps);
        printf("Batch %d: %llu episodes finished (%llu truncated), mean reward %.4f, mean |sum - V| per visit %.4g\n", e + 1,
               (unsigned long long)st.episodes, (unsigned long long)st.episodes_truncated, st.sum_reward / (double)st.env_steps,
               st.sum_episode_steps ? st.sum_abs_td_error / (double)st.sum_episode_steps : 0.0);
    }

    // one trajectory of `len` transitions per learner, from fresh episodes: start, then (state, action, reward) per step
    const int64_t len = cap < 20 ? (int64_t)cap : 20, N = n_envs;
    const size_t DN = (size_t)sess.state_dim() * (size_t)N;
    sess.reset();
    domains::Trajectory tr;
    tr.n_states.assign((size_t)N, (uint32_t)(len + 1));
    tr.total_reward.assign((size_t)N, 0.0f);
    tr.terminal.assign((size_t)N, 0);
    tr.states.assign((size_t)(len + 1) * DN, 0.0f);
    tr.actions.assign((size_t)len * N, 0);
    tr.rewards.assign((size_t)len * N, 0.0f);
    std::vector<int32_t> a = sess.sample();
    for (int64_t k = 0; k < len; ++k) {
        domains::Transition t = sess.transition(a);
        for (size_t j = 0; j < DN; ++j) { tr.states[(size_t)k * DN + j] = t.from[j]; tr.states[(size_t)(k + 1) * DN + j] = t.to[j]; }
        for (int64_t i = 0; i < N; ++i) {
            tr.actions[(size_t)(k * N + i)] = a[(size_t)i];
            tr.rewards[(size_t)(k * N + i)] = t.reward[(size_t)i];
            tr.total_reward[(size_t)i] += t.reward[(size_t)i];
        }
        a = sess.sample();
    }
    const std::vector<float> w0 = sess.weights(0);
    const std::vector<float> g = sess.handle(tr);
    const std::vector<float> w1 = sess.weights(0);
    double wmax = 0, moved = 0;
    for (size_t f = 0; f < w1.size(); ++f) {
        wmax = std::fabs(w1[f]) > wmax ? std::fabs(w1[f]) : wmax;
        moved = std::fabs(w1[f] - w0[f]) > moved ? std::fabs(w1[f] - w0[f]) : moved;
    }
    printf("GradientMC: a %lld-step trajectory handled, return from its start %.6g; max |w| of learner 0: %.6g (%zu features), moved by %.3g\n",
           (long long)len, (double)g[0], wmax, w1.size(), moved);
    return 0;
}
