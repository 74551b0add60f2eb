// examples/cliff_walk.cpp -- cliff walking, the textbook use of the one-step agents: QLearning (off-policy: it learns the path along the cliff edge) against
// SARSA (on-policy: under an exploring policy it learns to keep away from the edge), both under EpsilonGreedy on rsrl_domains' CliffWalk::default() with
// the tabular Q of rsrl/src/fa/tabular/dense.rs, N independent learners each.  Prints, for each agent, the share of learners whose greedy rollout
// takes the 13-step path along the edge and the share that reaches the goal on a longer path; it asserts nothing about the shares.
//
//   g++ -std=c++17 -O2 examples/cliff_walk.cpp -Lrsrl_amd/lib -lrsrl_hip -Wl,-rpath,$PWD/rsrl_amd/lib -o cliff_walk
#include <cstdio>
#include <cstdlib>

#include "../rsrl_amd/host/rsrl.hpp"

using namespace rsrl;

static void run(const char* name, const domains::CliffWalk& env, const control::td::Agent& agent, const policies::Policy& policy, int steps) {
    Session sess(env, agent, policy, /*seed=*/0, /*max_episode_steps=*/1000);
    sess.reset();
    auto st = sess.train(steps);
    auto tr = sess.rollout(100);                                     // rollout(|s| policy.mode(s), Some(100))
    int64_t edge = 0, longer = 0;
    for (int64_t i = 0; i < env.n_envs; ++i) {
        const bool goal = tr.terminal[i] && tr.total_reward[i] > 0.0f;
        edge += goal && tr.n_states[i] == 14;                        // the start state + 13 steps
        longer += goal && tr.n_states[i] > 14;
    }
    printf("%-9s %llu env-steps, %llu episodes: the 13-step path along the edge %.3f, a longer path to the goal %.3f\n", name,
           (unsigned long long)st.env_steps, (unsigned long long)st.episodes, (double)edge / (double)env.n_envs, (double)longer / (double)env.n_envs);
}

int main(int argc, char** argv) {
    const int64_t n_envs = argc > 1 ? atoll(argv[1]) : 256;
    const int steps = argc > 2 ? atoi(argv[2]) : 20000;
    const double epsilon = argc > 3 ? atof(argv[3]) : 0.1;

    domains::CliffWalk env(n_envs);
    {
        auto q_func = make_shared(fa::tabular::Table::zeros(60, 4, /*step=*/0.5));
        policies::EpsilonGreedy policy(policies::Greedy(q_func), policies::Random(4), epsilon);
        run("QLearning", env, control::td::QLearning(q_func, 0.9), policy, steps);
    }
    {
        auto q_func = make_shared(fa::tabular::Table::zeros(60, 4, /*step=*/0.5));
        policies::EpsilonGreedy policy(policies::Greedy(q_func), policies::Random(4), epsilon);
        run("SARSA", env, control::td::SARSA(q_func, policy, 0.9), policy, steps);
    }
    return 0;
}
