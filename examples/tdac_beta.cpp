// examples/tdac_beta.cpp -- the agent and the loop of the reference's rsrl/examples/tdac_beta.rs on the HIP path: ContinuousMountainCar with
// Fourier(3).with_bias(), policy = Beta::new(alpha, beta) over two Softplus-composed scalar LFAs, eval = iLSTD::new(basis, 1e-5, 0.999, 2),
// ActorCritic::tdac(critic, policy, 0.001, 0.999); per transition eval.handle, agent.handle, then a' = agent.policy.sample(s'); episodes capped at
// 1000 steps; a rollout with policy.mode at the end -- N environments instead of one.
//
//   g++ -std=c++17 -O2 examples/tdac_beta.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o tdac_beta
//   ./tdac_beta [n_envs] [batches] [steps per batch]
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../rsrl_amd/host/rsrl.hpp"

using namespace rsrl;

int main(int argc, char** argv) {
    const int64_t n_envs = argc > 1 ? atoll(argv[1]) : 64;
    const int batches = argc > 2 ? atoi(argv[2]) : 10;
    const int steps = argc > 3 ? atoi(argv[3]) : 1000;

    domains::ContinuousMountainCar env(n_envs);
    auto basis = fa::linear::basis::Fourier::from_space(3, env).with_bias();
    policies::Beta policy(basis);
    prediction::lstd::iLSTD eval(basis, 0.00001, 0.999, 2);
    auto agent = control::ac::ActorCritic::tdac(eval, policy, 0.001, 0.999);

    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/1000);
    sess.reset();
    for (int e = 0; e < batches; ++e) {
        auto st = sess.train(steps);
        printf("Batch %d: %llu episodes finished (%llu truncated), mean reward %.4f, mean |delta| %.4g\n", e + 1, (unsigned long long)st.episodes,
               (unsigned long long)st.episodes_truncated, st.sum_reward / (double)st.env_steps, st.sum_abs_td_error / (double)st.env_steps);
    }
    auto ls = sess.lstd_state(0, /*with_mu=*/true);
    auto w = sess.policy_weights(0);
    double vmax = 0, wmax = 0;
    for (double x : ls.theta) vmax = std::fabs(x) > vmax ? std::fabs(x) : vmax;
    for (float x : w) wmax = std::fabs(x) > wmax ? std::fabs(x) : wmax;
    auto ab = sess.policy_params(sess.emit());
    printf("iLSTD: max |theta| of learner 0: %.6g (%zu features); Beta: max |w| of learner 0: %.6g (%zu weights), alpha %.4f beta %.4f at its state\n", vmax,
           ls.theta.size(), wmax, w.size(), ab.first[0], ab.second[0]);
    auto tot = sess.rollout_total_reward(1000);                      // ContinuousMountainCar::default().rollout(|s| agent.policy.mode(s), Some(1000))
    double mean = 0; for (auto x : tot) mean += x;
    printf("OOS: %.1f...\n", mean / n_envs);
    return 0;
}
