// examples/lstd.cpp -- least-squares policy evaluation on the HIP path: RecursiveLSTD (gamma 0.99) or iLSTD (alpha 0.01, gamma 0.99, 4 updates
// per transition) learns V of the uniform Random policy on MountainCar with Fourier(order).with_bias(), N environments at once, episodes capped at
// 1000 steps.  Per transition: env.transition, agent.handle, a' = Random.sample -- the loop of the prediction examples, fused on the device.
//
//   g++ -std=c++17 -O2 examples/lstd.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o lstd
//   ./lstd [n_envs] [batches] [steps per batch] [order] [recursive|ilstd]
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
    const bool incremental = argc > 5 && strcmp(argv[5], "ilstd") == 0;

    domains::MountainCar env(n_envs);
    auto basis = fa::linear::basis::Fourier::from_space(order, env).with_bias();
    policies::Random policy(3);
    control::td::Agent agent = incremental ? control::td::Agent(prediction::lstd::iLSTD(basis, 0.01, 0.99, 4))
                                           : control::td::Agent(prediction::lstd::RecursiveLSTD(basis, 0.99));

    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/1000);
    sess.reset();
    for (int e = 0; e < batches; ++e) {
        auto st = sess.train(steps);
        printf("Batch %d: %llu episodes finished (%llu truncated), mean reward %.4f, mean |delta| %.4g\n", e + 1, (unsigned long long)st.episodes,
               (unsigned long long)st.episodes_truncated, st.sum_reward / (double)st.env_steps, st.sum_abs_td_error / (double)st.env_steps);
    }
    auto ls = sess.lstd_state(0, incremental);
    double tmax = 0, mmax = 0;
    for (double x : ls.theta) tmax = std::fabs(x) > tmax ? std::fabs(x) : tmax;
    for (double x : ls.mat) mmax = std::fabs(x) > mmax ? std::fabs(x) : mmax;
    printf("%s: max |theta| of learner 0: %.6g (%zu features), max |%s| of learner 0: %.6g\n", incremental ? "iLSTD" : "RecursiveLSTD", tmax,
           ls.theta.size(), incremental ? "A" : "C", mmax);
    return 0;
}
