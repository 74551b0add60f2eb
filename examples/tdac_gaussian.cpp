// examples/tdac_gaussian.cpp -- ActorCritic::tdac (rsrl/src/control/ac.rs) with a TD(0) critic over the Gaussian policy on the HIP path
// (RSRL_CONTINUOUS_TD_ACTOR_CRITIC): ContinuousMountainCar with Fourier(3).with_bias(), policy = Gaussian::new(lfa, clfa) -- the mean a scalar LFA,
// the stddev a Softplus-composed one, SGD(1.0) on both --, eval = TD{LFA::scalar(basis, SGD(0.01)), gamma 0.999},
// ActorCritic::tdac(|s| eval.v_func.evaluate(s), policy, 0.001, 0.999).  The reference has no example that builds tdac over its Gaussian policy; the
// loop is the one tdac.rs, tdac_beta.rs and nac.rs all use: per transition env.transition(a) -- the action itself: the domain clips it --,
// eval.handle, agent.handle (its critic reads eval's updated weights), a' = policy.sample(s'); episodes capped at 1000 steps; a rollout with
// policy.mode at the end -- N environments instead of one.  There is no safeguard on the score: sd is floored at 0.01 only.
//
//   g++ -std=c++17 -O2 examples/tdac_gaussian.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o tdac_gaussian
//   ./tdac_gaussian [n_envs] [batches] [steps per batch]
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
    policies::Gaussian policy(basis);
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
    auto tot = sess.rollout_total_reward(1000);      // ContinuousMountainCar::default().rollout(|s| agent.policy.mode(s), Some(1000))
    double mean = 0; for (auto x : tot) mean += x;
    printf("OOS: %.1f...\n", mean / n_envs);
    return 0;
}
