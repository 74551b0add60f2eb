"""The Beta-policy iLSTD ActorCritic's driver-loop rate: us per batch-step and env-steps/s of k_train_tdac_beta on ContinuousMountainCar at 65 536
learners, Fourier order 3, episodes capped at 1 000 steps, with tdac_beta.rs's constants (iLSTD(1e-5, 0.999, n_updates 2), alpha 0.001) -- next to
the Gibbs iLSTD ActorCritic (k_train_tdac_lstd on MountainCar, the same F, the same critic) on the same build.  One JSON line per configuration;
vs_gibbs is the rate relative to the Gibbs actor's at the same shape.
    python scripts/tdac_beta_rate.py [--steps 256] [--warmup 32] [--sizes 65536] [--orders 3] [--spl N]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rsrl_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--sizes", default="65536")
    ap.add_argument("--orders", default="3")
    ap.add_argument("--spl", type=int, default=0, help="steps per launch (0: the library's default)")
    a = ap.parse_args()
    critic = dict(algo=rsrl_amd.ILSTD_ACTOR_CRITIC, lr=1e-5, gamma=0.999, n_steps=2, alpha=0.001)
    agents = (("Gibbs iLSTD ActorCritic", dict(critic, domain=rsrl_amd.MOUNTAIN_CAR, policy=rsrl_amd.SOFTMAX, tau=1.0)),
              ("Beta iLSTD ActorCritic", dict(critic, domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, policy=rsrl_amd.BETA)))
    for order in [int(x) for x in a.orders.split(",")]:
        for n in [int(x) for x in a.sizes.split(",")]:
            base = None
            for agent, kw in agents:
                with rsrl_amd.Context(order=order, n_envs=n, max_episode_steps=1000, steps_per_launch=a.spl, **kw) as c:
                    c.reset()
                    c.train(a.warmup, want_stats=False)
                    c.sync()
                    c.timing_enable(True)
                    c.train(a.steps, want_stats=False)
                    ms, launches, name = c.timing_read()
                    us = ms * 1e3 / a.steps
                    rate = n / (us * 1e-6)
                    base = rate if base is None else base
                    print(json.dumps(dict(agent=agent, kernel=name, order=order, features=c.F, n_envs=n, batch_steps=a.steps, launches=launches,
                                          us_per_batch_step=round(us, 2), env_steps_per_s=rate, vs_gibbs=round(rate / base, 3))), flush=True)


if __name__ == "__main__":
    main()
