// examples/nac_softmax.cpp -- the agent and the loop of the reference's rsrl/examples/nac_softmax.rs on the HIP path: MountainCar with
// Fourier(3).with_bias(), policy = Softmax::new(LFA::vector(basis, SGD(1.0), n_actions), 1.0), critic = SARSA{LFA::scalar(SCB{policy, basis},
// SGD(0.01)), policy, gamma 0.999}, NAC::new(critic, policy, 0.01); per transition env.transition(a), critic.handle, a' = policy.sample(s'), and
// agent.handle(()) at every 100th step of an episode; episodes capped at 1000 steps; a rollout with policy.mode at the end -- N environments
// instead of one.  SCB's features are grad_log flattened row-major, then phi: the one line of SCB::project the library restores
// (include/rsrl_hip.h, RSRL_GIBBS_NAC) -- as it stands the reference example stops at its first critic.handle.
//
//   g++ -std=c++17 -O2 examples/nac_softmax.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o nac_softmax
//   ./nac_softmax [n_envs] [batches] [steps per batch]
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
    policies::Gibbs policy(make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(1.0), 3)), 1.0);
    fa::linear::basis::SCB basis_c{policy, basis};
    auto cfa = make_shared(fa::linear::LFA::scalar(basis_c, fa::linear::optim::SGD(0.01)));
    control::td::SARSA critic(cfa, policy, 0.999);
    control::nac::NAC agent(critic, policy, 0.01, /*period=*/100);

    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/1000);
    sess.reset();
    for (int e = 0; e < batches; ++e) {
        auto st = sess.train(steps);
        printf("Batch %d: %llu episodes finished (%llu truncated), mean reward %.4f, mean |delta| %.4g\n", e + 1, (unsigned long long)st.episodes,
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
