"""GradientMC's driver-loop rate: us per batch-step and env-steps/s of k_train_gmc next to k_train_td (the same environment side, draw for draw; one
projection, two dot products and an axpy per step against GradientMC's one projection, one dot product, one axpy and the record's D + 1 stores and
loads), in the same process on the same configuration:
    MountainCar order 3 and order 5, cap 1000 (the learners' episodes end in step with each other: a wave sweeps together)
    CartPole order 1, cap 200               (ragged ends: lanes whose episodes end at different steps serialise the sweep)
Both ctxs are warmed up (every learner past its first episode end), then timed in alternating regions of --steps batch-steps by the library's device
events; the figure is the median region, and every region is listed: GradientMC's grow with the run as episodes fall out of step, and a region
without the common sweep still holds the sweeps of the learners that are out of phase (profiles/gmc_rate.md).  One JSON line per (configuration, steps per launch); vs_td is GradientMC's rate over TD's.
    python scripts/gmc_rate.py [--steps 8192] [--regions 7] [--n 65536] [--spl 0[,1024,...]] [--only mc3,mc5,cp1]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rsrl_amd  # noqa: E402

CONFIGS = {
    "mc3": dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, max_episode_steps=1000),
    "mc5": dict(domain=rsrl_amd.MOUNTAIN_CAR, order=5, max_episode_steps=1000),
    "cp1": dict(domain=rsrl_amd.CART_POLE, order=1, max_episode_steps=200),
}


def region(c, steps):
    c.timing_enable(True)
    c.train(steps, want_stats=False)
    ms, launches, name = c.timing_read()
    c.timing_enable(False)
    return ms * 1e3 / steps, launches, name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8192)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--spl", default="0", help="steps per launch, comma separated (0: the library's default)")
    ap.add_argument("--only", default="mc3,mc5,cp1")
    a = ap.parse_args()
    if a.regions < 5:
        sys.exit("at least five regions")
    for key in a.only.split(","):
        cfg = CONFIGS[key]
        for spl in [int(x) for x in a.spl.split(",")]:
            kw = dict(cfg, n_envs=a.n, policy=rsrl_amd.RANDOM, gamma=0.99, lr=0.001, seed=1, steps_per_launch=spl)
            with rsrl_amd.Context(algo=rsrl_amd.TD, **kw) as td, rsrl_amd.Context(algo=rsrl_amd.GRADIENT_MC, **kw) as mc:
                warm = None
                for c in (td, mc):
                    c.reset()
                    warm = c.train(2 * cfg["max_episode_steps"] + 64)      # every learner has ended an episode: the sweeps are part of the steady state
                    c.sync()
                us = {"td": [], "gmc": []}
                names = {}
                for _ in range(a.regions):                                  # alternating: a drift of the machine lands on both
                    for tag, c in (("td", td), ("gmc", mc)):
                        t, launches, names[tag] = region(c, a.steps)
                        us[tag].append(t)
                med = {k: statistics.median(v) for k, v in us.items()}
                rate = {k: a.n / (v * 1e-6) for k, v in med.items()}
                print(json.dumps(dict(config=key, features=mc.F, n_envs=a.n, cap=cfg["max_episode_steps"], steps_per_launch=spl, batch_steps=a.steps,
                                      regions=a.regions, kernels=names, us_per_batch_step={k: round(v, 3) for k, v in med.items()},
                                      regions_us={k: [round(x, 3) for x in v] for k, v in us.items()},
                                      env_steps_per_s=rate, vs_td=round(rate["gmc"] / rate["td"], 3),
                                      warmup_mean_episode=round(warm["sum_episode_steps"] / max(1, warm["episodes"]), 1))), flush=True)


if __name__ == "__main__":
    main()
