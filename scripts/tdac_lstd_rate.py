"""The iLSTD ActorCritic's driver-loop rate: us per batch-step and env-steps/s of k_train_tdac_lstd on MountainCar at 262 144 learners, Fourier
orders 3 and 5, with tdac.rs's constants (iLSTD(1e-4, 0.99, n_updates 2), alpha 0.002) -- next to k_train_lstd (iLSTD alone, Random behaviour: the
same f64 step without the actor, the yardstick; scripts/lstd_rate.py measures it over more shapes) and k_train_tdac (the TD(0) critic) on the same
shapes.  One JSON line per configuration; vs_ilstd is the rate relative to iLSTD's at the same shape.
    python scripts/tdac_lstd_rate.py [--steps 256] [--warmup 32] [--sizes 262144] [--orders 3,5] [--n-updates 2] [--spl N]"""
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
    ap.add_argument("--sizes", default="262144")
    ap.add_argument("--orders", default="3,5")
    ap.add_argument("--n-updates", type=int, default=2)
    ap.add_argument("--spl", type=int, default=0, help="steps per launch (0: the library's default)")
    a = ap.parse_args()
    agents = (("iLSTD", dict(algo=rsrl_amd.ILSTD, policy=rsrl_amd.RANDOM, alpha=1e-4, gamma=0.99, n_steps=a.n_updates)),
              ("iLSTD ActorCritic", dict(algo=rsrl_amd.ILSTD_ACTOR_CRITIC, policy=rsrl_amd.SOFTMAX, lr=1e-4, gamma=0.99, n_steps=a.n_updates, alpha=0.002, tau=1.0)),
              ("TD ActorCritic", dict(algo=rsrl_amd.TD_ACTOR_CRITIC, policy=rsrl_amd.SOFTMAX, lr=0.01, gamma=0.99, alpha=0.002, tau=1.0)))
    for order in [int(x) for x in a.orders.split(",")]:
        for n in [int(x) for x in a.sizes.split(",")]:
            base = None
            for agent, kw in agents:
                with rsrl_amd.Context(domain=rsrl_amd.MOUNTAIN_CAR, order=order, n_envs=n, max_episode_steps=1000, steps_per_launch=a.spl, **kw) as c:
                    c.reset()
                    c.train(a.warmup, want_stats=False)
                    c.sync()
                    c.timing_enable(True)
                    c.train(a.steps, want_stats=False)
                    ms, launches, name = c.timing_read()
                    us = ms * 1e3 / a.steps
                    rate = n / (us * 1e-6)
                    base = rate if agent == "iLSTD" else base
                    print(json.dumps(dict(agent=agent, kernel=name, order=order, features=c.F, n_envs=n, batch_steps=a.steps, launches=launches,
                                          us_per_batch_step=round(us, 2), env_steps_per_s=rate, vs_ilstd=round(rate / base, 3))), flush=True)


if __name__ == "__main__":
    main()
