// examples/a2c.cpp -- the reference's rsrl/examples/a2c.rs on the HIP path: MountainCar, Fourier(3).with_bias(), the critic's
// q_func = LFA::vector(SGD(0.001)), the actor Gibbs::standard(LFA::vector(SGD(1.0))), SARSA(gamma 1.0) as the critic's evaluator,
// ActorCritic with a2c.rs's advantage closure and alpha 0.001, episodes capped at 1000 steps -- N environments instead of one.
//
//   g++ -std=c++17 -O2 examples/a2c.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o a2c
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../rsrl_amd/host/rsrl.hpp"

using namespace rsrl;

int main(int argc, char** argv) {
    const int64_t n_envs = argc > 1 ? atoll(argv[1]) : 64;
    const int batches = argc > 2 ? atoi(argv[2]) : 10;
    const int steps = argc > 3 ? atoi(argv[3]) : 1000;

    domains::MountainCar env(n_envs);
    auto basis = fa::linear::basis::Fourier::from_space(3, env).with_bias();
    auto q_func = make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(0.001), 3));
    auto policy = policies::Gibbs::standard(make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(1.0), 3)));
    control::td::SARSA eval(q_func, policy, 1.0);
    control::ac::ActorCritic agent(eval, policy, 0.001);

    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/1000);
    sess.reset();
    for (int e = 0; e < batches; ++e) {
        auto st = sess.train(steps);
        printf("Batch %d: %llu episodes finished (%llu truncated), mean reward %.4f, mean |td| %.4f\n", e + 1, (unsigned long long)st.episodes,
               (unsigned long long)st.episodes_truncated, st.sum_reward / (double)st.env_steps, st.sum_abs_td_error / (double)st.env_steps);
    }
    auto th = sess.policy_weights(0);
    double tmax = 0; for (float x : th) tmax = std::fabs(x) > tmax ? std::fabs(x) : tmax;
    printf("max |theta| of learner 0: %.6g\n", tmax);
    auto tr = sess.rollout(1000);                                    // MountainCar::default().rollout(|s| agent.policy.mode(s), Some(1000))
    double mean = 0; for (auto x : tr.total_reward) mean += x;
    printf("OOS: %.1f...\n", mean / n_envs);
    return 0;
}
