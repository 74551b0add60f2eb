// examples/lambda_lspe.cpp -- least-squares policy evaluation on the HIP path: LambdaLSPE (alpha 0.5, gamma 0.99, lambda 0.8) learns V of the uniform
// Random policy on MountainCar with Fourier(order).with_bias(), N environments at once, episodes capped at `cap` steps.  The reference has no example
// for this agent; the loop is lstd_lambda.cpp's.  The fused loop records every learner's open episode on the device and, when it ends, hands it to
// agent.handle(&batch): the transitions, walked last to first, accumulate into the Gram matrix A, into b and into the return correction delta, and
// solve() -- once A holds as many rows as there are features -- relaxes theta towards A^-1 b and starts A, b and delta afresh.  Afterwards one short
// batch per learner is collected by hand and handed to agent.handle(&batch) twice: a batch shorter than F defers its solve.
//
//   g++ -std=c++17 -O2 examples/lambda_lspe.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o lambda_lspe
//   ./lambda_lspe [n_envs] [batches] [steps per batch] [order] [cap] [alpha]
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
    const double alpha = argc > 6 ? atof(argv[6]) : 0.5;

    domains::MountainCar env(n_envs);
    auto basis = fa::linear::basis::Fourier::from_space(order, env).with_bias();
    policies::Random policy(3);
    control::td::Agent agent = prediction::lstd::LambdaLSPE(basis, alpha, 0.99, 0.8);

    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/cap);
    sess.reset();
    for (int e = 0; e < batches; ++e) {
        auto st = sess.train(steps);
        printf("Batch %d: %llu episodes finished (%llu truncated), mean reward %.4f, mean |delta| per handled transition %.4g\n", e + 1,
               (unsigned long long)st.episodes, (unsigned long long)st.episodes_truncated, st.sum_reward / (double)st.env_steps,
               st.sum_episode_steps ? st.sum_abs_td_error / (double)st.sum_episode_steps : 0.0);
    }

    // one batch of `len` whole transitions per learner, from fresh episodes: half the features' count, so that one batch alone defers
    const size_t F = sess.lstd_batch_state(0, true).theta.size();
    const int64_t len = (int64_t)(F / 2 < cap ? F / 2 : cap), N = n_envs;
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
    for (int pass = 0; pass < 3; ++pass) {
        const auto before = sess.lstd_batch_state(0, true);
        const std::vector<float> td = sess.handle(b);
        const auto after = sess.lstd_batch_state(0, true);
        double tmax = 0, moved = 0;
        for (size_t f = 0; f < F; ++f) {
            tmax = std::fabs(after.theta[f]) > tmax ? std::fabs(after.theta[f]) : tmax;
            moved = std::fabs(after.theta[f] - before.theta[f]) > moved ? std::fabs(after.theta[f] - before.theta[f]) : moved;
        }
        printf("LambdaLSPE: a %lld-transition batch handled, first diagnostic %.6g; learner 0 held %g of %zu rows before and %g after (%s), delta %.6g, "
               "max |theta| %.6g, moved by %.3g, %u abandoned solves\n", (long long)len, (double)td[0], before.z[1], F, after.z[1],
               after.z[1] == 0.0 ? "solved" : (after.singular_solves != before.singular_solves ? "abandoned" : "deferred"), after.z[0], tmax, moved,
               after.singular_solves);
    }
    return 0;
}
