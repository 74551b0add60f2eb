// examples/tdac_ilstd.cpp -- the agent and the loop of the reference's rsrl/examples/tdac.rs on the HIP path: eval = iLSTD::new(basis, 0.0001, 0.99, 2),
// the critic closure phi(s) . eval.theta, ActorCritic::tdac(critic, policy, 0.002, 0.99); per transition eval.handle, agent.handle, then
// a' = agent.policy.sample(s'); episodes capped at 1000 steps -- N environments instead of one.  Two substitutions remain, because the library runs
// discrete actions with linear Fourier features (examples/tdac.cpp makes a third: TD(0) in place of iLSTD):
//   1. the domain is the discrete MountainCar with Fourier(3).with_bias(), not ContinuousMountainCar;
//   2. the actor is Gibbs::standard(LFA::vector(SGD(1.0))) over the three actions, not a Gaussian over a continuous one.
//
//   g++ -std=c++17 -O2 examples/tdac_ilstd.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o tdac_ilstd
//   ./tdac_ilstd [n_envs] [batches] [steps per batch]
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
    auto policy = policies::Gibbs::standard(make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(1.0), 3)));
    prediction::lstd::iLSTD eval(basis, 0.0001, 0.99, 2);
    auto agent = control::ac::ActorCritic::tdac(eval, policy, 0.002, 0.99);

    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/1000);
    sess.reset();
    for (int e = 0; e < batches; ++e) {
        auto st = sess.train(steps);
        printf("Batch %d: %llu episodes finished (%llu truncated), mean reward %.4f, mean |delta| %.4g\n", e + 1, (unsigned long long)st.episodes,
               (unsigned long long)st.episodes_truncated, st.sum_reward / (double)st.env_steps, st.sum_abs_td_error / (double)st.env_steps);
    }
    auto ls = sess.lstd_state(0, /*with_mu=*/true);
    auto th = sess.policy_weights(0);
    double vmax = 0, amax = 0, tmax = 0;
    for (double x : ls.theta) vmax = std::fabs(x) > vmax ? std::fabs(x) : vmax;
    for (double x : ls.mat) amax = std::fabs(x) > amax ? std::fabs(x) : amax;
    for (float x : th) tmax = std::fabs(x) > tmax ? std::fabs(x) : tmax;
    printf("iLSTD: max |theta| of learner 0: %.6g (%zu features), max |A| of learner 0: %.6g; actor: max |theta| of learner 0: %.6g (%zu weights)\n", vmax,
           ls.theta.size(), amax, tmax, th.size());
    auto tr = sess.rollout(1000);                                    // MountainCar::default().rollout(|s| agent.policy.mode(s), Some(1000))
    double mean = 0; for (auto x : tr.total_reward) mean += x;
    printf("OOS: %.1f...\n", mean / n_envs);
    return 0;
}
