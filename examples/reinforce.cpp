// examples/reinforce.cpp -- REINFORCE with a Gibbs policy on the HIP path, N environments at once.  The reference has no REINFORCE example; this
// is the project's own, in the style of examples/tdac.cpp: each learner runs episodes of the discrete MountainCar (Fourier(3).with_bias(), capped
// at 1000 steps), every episode sampled from the policy as it stood when the episode began and handled as one Batch at its end (control/mc/
// reinforce.rs; the driver loop applies the batch's updates online, which gives the same bits).  Then the greedy rollout of tdac.rs.
//   argv: [n_envs] [batches] [steps per batch] [baseline: 0 / 1]
//
//   g++ -std=c++17 -O2 examples/reinforce.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o reinforce
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../rsrl_amd/host/rsrl.hpp"

using namespace rsrl;

int main(int argc, char** argv) {
    const int64_t n_envs = argc > 1 ? atoll(argv[1]) : 64;
    const int batches = argc > 2 ? atoi(argv[2]) : 10;
    const int steps = argc > 3 ? atoi(argv[3]) : 1000;
    const bool with_baseline = argc > 4 && atoi(argv[4]) != 0;

    domains::MountainCar env(n_envs);
    auto basis = fa::linear::basis::Fourier::from_space(3, env).with_bias();
    auto policy = policies::Gibbs::standard(make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(1.0), 3)));
    auto baseline = make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(1.0), 3));      // zero: BaselineREINFORCE == REINFORCE
    const control::td::Agent agent = with_baseline ? (control::td::Agent)control::mc::BaselineREINFORCE(baseline, policy, 0.001, 0.99)
                                                   : (control::td::Agent)control::mc::REINFORCE(policy, 0.001, 0.99);

    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/1000);
    sess.reset();
    for (int e = 0; e < batches; ++e) {
        auto st = sess.train(steps);
        printf("Batch %d: %llu episodes finished (%llu truncated), mean reward %.4f, mean |return| %.4f\n", e + 1, (unsigned long long)st.episodes,
               (unsigned long long)st.episodes_truncated, st.sum_reward / (double)st.env_steps, st.sum_abs_td_error / (double)st.env_steps);
    }
    auto th = sess.policy_weights(0);
    double tmax = 0;
    for (float x : th) tmax = std::fabs(x) > tmax ? std::fabs(x) : tmax;
    printf("max |theta| of learner 0: %.6g (%zu weights)\n", tmax, th.size());
    auto tr = sess.rollout(1000);                                    // MountainCar::default().rollout(|s| agent.policy.mode(s), Some(1000))
    double mean = 0; for (auto x : tr.total_reward) mean += x;
    printf("OOS: %.1f...\n", mean / n_envs);
    return 0;
}
