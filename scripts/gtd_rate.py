"""GTD2's and TDC's driver-loop rate: us per batch-step and env-steps/s of k_train_gtd next to k_train_td (the same environment side, draw for draw;
two projections' worth of features held, three dot products and three axpys per step against TD's three dot products and one axpy), in the same
process on the same configuration -- MountainCar order 3 (and 5) at 65 536 learners, cap 1000.  The three ctxs are warmed up, then timed in
alternating regions of --steps batch-steps by the library's device events; the figure is the median region and every region is listed.  One JSON
line per configuration; vs_td is each agent's rate over TD's (profiles/gtd_rate.md).
    python scripts/gtd_rate.py [--steps 8192] [--regions 7] [--n 65536] [--orders 3[,5]]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rsrl_amd  # noqa: E402
from gmc_rate import region  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8192)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--orders", default="3")
    a = ap.parse_args()
    if a.regions < 5:
        sys.exit("at least five regions")
    for order in [int(x) for x in a.orders.split(",")]:
        kw = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=order, max_episode_steps=1000, n_envs=a.n, policy=rsrl_amd.RANDOM, gamma=0.99, lr=0.001, seed=1)
        with rsrl_amd.Context(algo=rsrl_amd.TD, **kw) as td, rsrl_amd.Context(algo=rsrl_amd.GTD2, lr_td=0.002, **kw) as g2, \
                rsrl_amd.Context(algo=rsrl_amd.TDC, lr_td=0.002, **kw) as tc:
            ctxs = (("td", td), ("gtd2", g2), ("tdc", tc))
            for _, c in ctxs:
                c.reset()
                c.train(1024, want_stats=False)
                c.sync()
            us, names = {k: [] for k, _ in ctxs}, {}
            for _ in range(a.regions):                                  # alternating: a drift of the machine lands on all three
                for tag, c in ctxs:
                    t, _, names[tag] = region(c, a.steps)
                    us[tag].append(t)
            med = {k: statistics.median(v) for k, v in us.items()}
            rate = {k: a.n / (v * 1e-6) for k, v in med.items()}
            print(json.dumps(dict(order=order, features=td.F, n_envs=a.n, cap=1000, batch_steps=a.steps, regions=a.regions, kernels=names,
                                  us_per_batch_step={k: round(v, 3) for k, v in med.items()},
                                  regions_us={k: [round(x, 3) for x in v] for k, v in us.items()}, env_steps_per_s=rate,
                                  vs_td={k: round(rate[k] / rate["td"], 3) for k in ("gtd2", "tdc")})), flush=True)


if __name__ == "__main__":
    main()
