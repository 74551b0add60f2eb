"""REINFORCE driver-loop rate: us per batch-step and env-steps/s of k_train_reinforce (REINFORCE and BaselineREINFORCE) on MountainCar at 65 536
and 262 144 learners, Fourier orders 3 and 5 -- next to k_train_ac (ActorCritic with the SARSA critic and a2c.rs's target) on the same shapes as
the yardstick.  One JSON line per configuration.
    python scripts/reinforce_rate.py [--steps 256] [--warmup 32] [--sizes 65536,262144] [--orders 3,5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rsrl_amd  # noqa: E402

AGENTS = (("REINFORCE", dict(algo=rsrl_amd.REINFORCE, policy=rsrl_amd.SOFTMAX, alpha=0.001, gamma=0.99)),
          ("BaselineREINFORCE", dict(algo=rsrl_amd.BASELINE_REINFORCE, policy=rsrl_amd.SOFTMAX, alpha=0.001, gamma=0.99)),
          ("ActorCritic", dict(algo=rsrl_amd.ACTOR_CRITIC, policy=rsrl_amd.SOFTMAX, alpha=0.001, lr=0.001, gamma=1.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--sizes", default="65536,262144")
    ap.add_argument("--orders", default="3,5")
    a = ap.parse_args()
    for order in [int(x) for x in a.orders.split(",")]:
        for n in [int(x) for x in a.sizes.split(",")]:
            for agent, kw in AGENTS:
                with rsrl_amd.Context(domain=rsrl_amd.MOUNTAIN_CAR, order=order, n_envs=n, max_episode_steps=1000, steps_per_launch=a.steps, **kw) as c:
                    c.reset()
                    c.train(a.warmup, want_stats=False)
                    c.sync()
                    c.timing_enable(True)
                    c.train(a.steps, want_stats=False)
                    ms, launches, name = c.timing_read()
                    us = ms * 1e3 / a.steps
                    print(json.dumps(dict(agent=agent, kernel=name, order=order, features=c.F, n_envs=n, batch_steps=a.steps, launches=launches,
                                          us_per_batch_step=round(us, 2), env_steps_per_s=n / (us * 1e-6))), flush=True)


if __name__ == "__main__":
    main()
