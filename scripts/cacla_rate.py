"""CACLA over the Gaussian policy with a TD(0) critic (RSRL_CACLA, k_train_cacla): the measured f32 figure behind the bound of
tests/test_gpu_cacla.py, and the driver loop's rate.

1. The rule figures.  The device against the f64 restatement (tests/cacla_numpy.py: figures) on the GPU tests' own inputs (cacla_numpy.handle_case
   on the device's own projection: 67 learners, three rounds of handle_f32) at the Fourier orders 1 / 2 / 3 / 5: max |d column| / max(1, |column|)
   over the learners whose gate opened, and how many gates opened per round.  The test asserts four times the figure.
2. The rate.  us per batch-step and env-steps/s of k_train_cacla on ContinuousMountainCar at 65 536 learners, Fourier orders 1 / 3 / 5, episodes
   capped at 1 000 steps, with examples/cacla.cpp's constants (TD SGD(0.01), gamma 0.999, CACLA.alpha 0.01) -- next to RSRL_NAC with RSRL_GAUSSIAN
   (k_train_nac_gauss, nac.rs's constants) in ONE process on the same build and the same seeds, the contexts' timed regions alternating after a
   warm-up: the median of seven regions and every region.  From w = 0 and rewards of -1 V first sinks below every target, and which gates open later depends on
   the run, so a second CACLA ctx runs with EVERY gate open: V = -2000 on the constant feature (r + gamma V(s') = -1999 > V(s)) with
   lr = 0 and alpha = 0, so that V and the policy stay where they are while the whole arithmetic of the step runs.  The largest |column| afterwards says which gates opened.
3. The launch depth.  The order-3 CACLA loop at 256 / 1 024 / 4 096 batch-steps per launch (config.steps_per_launch), the same regions.
One JSON line per figure set and per row; --out writes the markdown tables that profiles/cacla_rate.md holds beside its commentary.
    python scripts/cacla_rate.py [--out FILE] [--regions 7] [--steps 8192] [--warmup 512] [--size 65536] [--orders 1,2,3,5] [--rate-orders 1,3,5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import rsrl_amd  # noqa: E402
from tests import cacla_numpy as cn  # noqa: E402
from rate_regions import alternate  # noqa: E402

CMC = rsrl_amd.CONTINUOUS_MOUNTAIN_CAR


def measure(order):
    with rsrl_amd.Context(domain=CMC, order=order, algo=rsrl_amd.CACLA, policy=rsrl_amd.GAUSSIAN, n_envs=67) as probe:
        case = cn.handle_case(order, probe.project)
    p = case["params"]
    with rsrl_amd.Context(domain=CMC, order=order, algo=rsrl_amd.CACLA, policy=rsrl_amd.GAUSSIAN, n_envs=len(case["init"]), seed=5, gamma=p["gamma"], lr=p["lr"],
                          alpha=p["alpha"]) as c:
        fig, arr = cn.figures(c, None, case)
    fig["open_per_round"] = [int(g.sum()) for g in arr["gates"]]
    fig["max_abs_column"] = float(np.max(np.abs(arr["want_cols"][arr["opened"]])))
    return fig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="a file for the markdown tables (default: none, the JSON lines only)")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8192, help="batch-steps per timed region")
    ap.add_argument("--warmup", type=int, default=512)
    ap.add_argument("--size", type=int, default=65536)
    ap.add_argument("--orders", default="1,2,3,5")
    ap.add_argument("--rate-orders", default="1,3,5")
    a = ap.parse_args()
    orders = [int(x) for x in a.orders.split(",")]
    figs = {}
    for order in orders:
        figs[order] = measure(order)
        print(json.dumps(dict(order=order, figures=figs[order])), flush=True)
    common = dict(domain=CMC, policy=rsrl_amd.GAUSSIAN, n_envs=a.size, max_episode_steps=1000, lr=0.01, gamma=0.999, alpha=0.01, seed=0)
    rate_rows = []
    for order in (int(x) for x in a.rate_orders.split(",")):
        rate_rows += alternate([("CACLA, from w = 0", dict(common, algo=rsrl_amd.CACLA, order=order)),
                                ("CACLA, every gate open (V = -2000, lr = alpha = 0)", dict(common, algo=rsrl_amd.CACLA, order=order, lr=0.0, alpha=0.0, v0=-2000.0)),
                                ("NAC, Gaussian policy (nac.rs)", dict(common, algo=rsrl_amd.NAC, order=order, n_steps=100))], a, base=-1)
    depth_rows = alternate([("CACLA, %d steps per launch" % d, dict(common, algo=rsrl_amd.CACLA, order=3, steps_per_launch=d)) for d in (256, 1024, 4096)], a)
    for r in rate_rows + depth_rows:
        print(json.dumps(r), flush=True)
    if a.out is None:
        return
    cell = lambda r: "%.2f (%.2f .. %.2f)" % (r["us_per_batch_step"], min(r["us_per_batch_step_regions"]), max(r["us_per_batch_step_regions"]))      # noqa: E731
    with open(a.out, "w") as f:
        f.write("## The measured f32 maximum (max |d column| / max(1, |column|) over the open-gate learners, against the f64 restatement)\n\n")
        f.write("| order | F | the figure | gates open per round (of 67) | max |column| among them |\n|---|---|---|---|---|\n")
        for o in orders:
            f.write("| %d | %d | %.3e | %s | %.3g |\n" % (o, (o + 1) ** 2, figs[o]["cols"], " / ".join(str(x) for x in figs[o]["open_per_round"]), figs[o]["max_abs_column"]))
        f.write("\n## The driver loop's rate (%d learners, cap 1 000; median of %d regions of %d batch-steps after %d of warm-up, and the range)\n\n" %
                (a.size, a.regions, a.steps, a.warmup))
        f.write("| order | agent | kernel | us per batch-step | env-steps/s | time relative to the Gaussian NAC's | largest |policy column| afterwards, learners with a non-finite column (of the first 256) |\n"
                "|---|---|---|---|---|---|---|\n")
        for r in rate_rows:
            f.write("| %d | %s | `%s` | %s | %.3e | %.3f | %.3g, %d |\n" % (r["order"], r["agent"], r["kernel"], cell(r), r["env_steps_per_s"], r["vs_base"],
                                                                          r["max_abs_policy_column_of_first_256"], r["non_finite_of_first_256"]))
        f.write("\n## The launch depth (order 3, the same regions)\n\n| steps per launch | launches per region | us per batch-step |\n|---|---|---|\n")
        for r in depth_rows:
            f.write("| %s | %d | %s |\n" % (r["agent"].split(", ")[1].split()[0], r["launches_per_region"], cell(r)))


if __name__ == "__main__":
    main()
