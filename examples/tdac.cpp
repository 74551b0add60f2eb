// examples/tdac.cpp -- the loop of the reference's rsrl/examples/tdac.rs on the HIP path: per transition eval.handle, agent.handle, then
// a' = agent.policy.sample(s'), with ActorCritic::tdac (alpha 0.002, gamma 0.99) reading its TDCritic off the evaluator's V, episodes capped at
// 1000 steps -- N environments instead of one.  Three substitutions, because the library runs discrete actions with linear Fourier features:
//   1. the domain is the discrete MountainCar with Fourier(3).with_bias(), not ContinuousMountainCar;
//   2. the actor is Gibbs::standard(LFA::vector(SGD(1.0))) over the three actions, not a Gaussian over a continuous one;
//   3. the evaluator is the TD(0) prediction agent on a ScalarLFA (SGD(0.01)), not iLSTD.
//
//   g++ -std=c++17 -O2 examples/tdac.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o tdac
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
    auto v_func = make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(0.01), 1));      // V: one weight column
    auto policy = policies::Gibbs::standard(make_shared(fa::linear::LFA::vector(basis, fa::linear::optim::SGD(1.0), 3)));
    auto agent = control::ac::ActorCritic::tdac(v_func, policy, 0.002, 0.99);

    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/1000);
    sess.reset();
    for (int e = 0; e < batches; ++e) {
        auto st = sess.train(steps);
        printf("Batch %d: %llu episodes finished (%llu truncated), mean reward %.4f, mean |td| %.4f\n", e + 1, (unsigned long long)st.episodes,
               (unsigned long long)st.episodes_truncated, st.sum_reward / (double)st.env_steps, st.sum_abs_td_error / (double)st.env_steps);
    }
    auto w = sess.weights(0);
    auto th = sess.policy_weights(0);
    double wmax = 0, tmax = 0;
    for (float x : w) wmax = std::fabs(x) > wmax ? std::fabs(x) : wmax;
    for (float x : th) tmax = std::fabs(x) > tmax ? std::fabs(x) : tmax;
    printf("max |w| of learner 0: %.6g (%zu weights), max |theta| of learner 0: %.6g (%zu weights)\n", wmax, w.size(), tmax, th.size());
    auto tr = sess.rollout(1000);                                    // MountainCar::default().rollout(|s| agent.policy.mode(s), Some(1000))
    double mean = 0; for (auto x : tr.total_reward) mean += x;
    printf("OOS: %.1f...\n", mean / n_envs);
    return 0;
}
