// examples/tdac_beta_td.cpp -- the agent and the loop of the reference's rsrl/examples/tdac_beta.rs with TD(0) as `eval` on the HIP path
// (RSRL_CONTINUOUS_TD_ACTOR_CRITIC): ContinuousMountainCar with Fourier(3).with_bias(), policy = Beta::new(alpha, beta) over two Softplus-composed
// scalar LFAs, eval = TD{LFA::scalar(basis, SGD(0.01)), gamma 0.999} in iLSTD's place, ActorCritic::tdac(critic, policy, 0.001, 0.999); per transition
// eval.handle, agent.handle, then a' = agent.policy.sample(s'); the domain is handed 2a - 1 (nac_beta.rs's mapping of the sample's [0, 1] onto the
// domain's [-1, 1]) and the rollout at the end 2 mode - 1; episodes capped at 1000 steps -- N environments instead of one.
//
//   g++ -std=c++17 -O2 examples/tdac_beta_td.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o tdac_beta_td
//   ./tdac_beta_td [n_envs] [batches] [steps per batch]
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
    auto v_func = make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(0.01), 1));      // LFA::scalar(basis, SGD(0.01))
    prediction::td::TD eval(v_func, 0.999);
    auto agent = control::ac::ActorCritic::tdac(eval, policy, 0.001, 0.999);

    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/1000);
    sess.reset();
    for (int e = 0; e < batches; ++e) {
        auto st = sess.train(steps);
        printf("Batch %d: %llu episodes finished (%llu truncated), mean reward %.4f, mean |delta| %.4g\n", e + 1, (unsigned long long)st.episodes,
               (unsigned long long)st.episodes_truncated, st.sum_reward / (double)st.env_steps, st.sum_abs_td_error / (double)st.env_steps);
    }
    auto w = sess.policy_weights(0);
    float wmax = 0;
    for (float x : w) wmax = std::fabs(x) > wmax ? std::fabs(x) : wmax;
    auto ab = sess.policy_params(sess.emit());
    printf("Beta: max |w| of learner 0: %.6g (%zu weights), alpha %.4f beta %.4f at its state\n", wmax, w.size(), ab.first[0], ab.second[0]);
    auto tot = sess.rollout_total_reward(1000);      // ContinuousMountainCar::default().rollout(|s| 2 * agent.policy.mode(s) - 1, Some(1000))
    double mean = 0; for (auto x : tot) mean += x;
    printf("OOS: %.1f...\n", mean / n_envs);
    return 0;
}
