// examples/lstd_lambda.cpp -- batch least-squares policy evaluation on the HIP path: LSTDLambda (gamma 0.99, lambda 0.8) or LSTD (gamma 0.99) learns V
// of the uniform Random policy on MountainCar with Fourier(order).with_bias(), N environments at once, episodes capped at `cap` steps.  The fused loop
// records every learner's open episode on the device and, when it ends, hands it to agent.handle(&batch): the transitions accumulate into A and b
// (LSTDLambda walks them last to first with its trace z) and solve() takes theta = A^-1 b.  Afterwards one batch per learner is collected by hand
// (transition, sample) and handed to agent.handle(&batch), the reference's own call.
//
//   g++ -std=c++17 -O2 examples/lstd_lambda.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o lstd_lambda
//   ./lstd_lambda [n_envs] [batches] [steps per batch] [order] [cap] [lambda|lstd]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../rsrl_amd/host/rsrl.hpp"

using namespace rsrl;

int main(int argc, char** argv) {
    const int64_t n_envs = argc > 1 ? atoll(argv[1]) : 64;
    const int batches = argc > 2 ? atoi(argv[2]) : 5;
    const int steps = argc > 3 ? atoi(argv[3]) : 1000;
    const int order = argc > 4 ? atoi(argv[4]) : 3;
    const uint32_t cap = argc > 5 ? (uint32_t)atoi(argv[5]) : 200;
    const bool with_trace = !(argc > 6 && strcmp(argv[6], "lstd") == 0);

    domains::MountainCar env(n_envs);
    auto basis = fa::linear::basis::Fourier::from_space(order, env).with_bias();
    policies::Random policy(3);
    control::td::Agent agent = with_trace ? control::td::Agent(prediction::lstd::LSTDLambda(basis, 0.99, 0.8))
                                          : control::td::Agent(prediction::lstd::LSTD(basis, 0.99));

    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/cap);
    sess.reset();
    for (int e = 0; e < batches; ++e) {
        auto st = sess.train(steps);
        printf("Batch %d: %llu episodes finished (%llu truncated), mean reward %.4f, mean |delta| per handled transition %.4g\n", e + 1,
               (unsigned long long)st.episodes, (unsigned long long)st.episodes_truncated, st.sum_reward / (double)st.env_steps,
               st.sum_episode_steps ? st.sum_abs_td_error / (double)st.sum_episode_steps : 0.0);
    }

    // one batch of `len` whole transitions per learner, from fresh episodes
    const int64_t len = cap < 20 ? (int64_t)cap : 20, N = n_envs;
    const size_t DN = (size_t)sess.state_dim() * (size_t)N;
    sess.reset();
    domains::Batch b;
    b.T = len;
    b.states.assign((size_t)len * DN, 0.0f);
    b.to.assign((size_t)len * DN, 0.0f);
    b.rewards.assign((size_t)len * N, 0.0f);
    b.terminal.assign((size_t)len * N, 0);
    b.lengths.assign((size_t)N, (uint32_t)len);
    std::vector<int32_t> a = sess.sample();
    for (int64_t k = 0; k < len; ++k) {
        domains::Transition t = sess.transition(a);
        for (size_t j = 0; j < DN; ++j) { b.states[(size_t)k * DN + j] = t.from[j]; b.to[(size_t)k * DN + j] = t.to[j]; }
        for (int64_t i = 0; i < N; ++i) {
            b.rewards[(size_t)(k * N + i)] = t.reward[(size_t)i];
            b.terminal[(size_t)(k * N + i)] = t.terminal[(size_t)i];
        }
        a = sess.sample();
    }
    const auto before = sess.lstd_batch_state(0, with_trace);
    const std::vector<float> td = sess.handle(b);
    const auto after = sess.lstd_batch_state(0, with_trace);
    double tmax = 0, amax = 0, moved = 0;
    for (size_t f = 0; f < after.theta.size(); ++f) {
        tmax = std::fabs(after.theta[f]) > tmax ? std::fabs(after.theta[f]) : tmax;
        moved = std::fabs(after.theta[f] - before.theta[f]) > moved ? std::fabs(after.theta[f] - before.theta[f]) : moved;
    }
    for (double x : after.A) amax = std::fabs(x) > amax ? std::fabs(x) : amax;
    printf("%s: a %lld-transition batch handled, first diagnostic %.6g; max |theta| of learner 0: %.6g (%zu features), moved by %.3g, max |A| %.6g, "
           "%u abandoned solves\n", with_trace ? "LSTDLambda" : "LSTD", (long long)len, (double)td[0], tmax, after.theta.size(), moved, amax,
           after.singular_solves);
    return 0;
}
