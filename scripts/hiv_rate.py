"""HIVTreatment driver-loop rate: us per batch-step and env-steps/s of k_hiv_train (QLearning, epsilon-greedy, per-learner f32 weights) at
65 536, 262 144 and 1 048 576 learners for Fourier orders 1 and 3.  One JSON line per configuration.
    python scripts/hiv_rate.py [--steps 8] [--warmup 2] [--sizes 65536,262144,1048576] [--orders 1,3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rsrl_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="65536,262144,1048576")
    ap.add_argument("--orders", default="1,3")
    ap.add_argument("--domain-step", action="store_true", help="also run two rsrl_hip_domain_step calls: k_hiv_domain_step is the ODE alone "
                    "(a kernel trace then splits the loop's time into integration and learning)")
    a = ap.parse_args()
    for order in [int(x) for x in a.orders.split(",")]:
        for n in [int(x) for x in a.sizes.split(",")]:
            with rsrl_amd.Context(domain=rsrl_amd.HIV_TREATMENT, order=order, n_envs=n, policy=rsrl_amd.EPSILON_GREEDY, epsilon=0.1,
                                  lr=0.01, max_episode_steps=200, steps_per_launch=a.steps) as c:
                c.reset()
                c.train(a.warmup, want_stats=False)
                c.sync()
                c.timing_enable(True)
                c.train(a.steps, want_stats=False)
                ms, launches, name = c.timing_read()
                us = ms * 1e3 / a.steps
                print(json.dumps(dict(kernel=name, order=order, features=c.F, n_envs=n, batch_steps=a.steps, launches=launches,
                                      us_per_batch_step=round(us, 1), env_steps_per_s=n / (us * 1e-6))), flush=True)
                if a.domain_step:
                    for _ in range(2):
                        c.domain_step()
                    c.sync()


if __name__ == "__main__":
    main()
