"""The continuous TD ActorCritic (RSRL_CONTINUOUS_TD_ACTOR_CRITIC, k_train_tdac_cont) over the Gaussian and the Beta policy: the measured f32
figures behind the bounds of tests/test_gpu_tdac_cont.py and tests/fuzz_tdac_cont.py, and the driver loop's rate.

1. The rule figures.  The device against the f64 restatement (tests/tdac_cont_numpy.py: figures) on the GPU tests' own inputs (handle_case on the
   device's own projection: 67 learners, three rounds of handle_f32) at the Fourier orders 1-5 under both policies: max |d column| /
   max(1, |column|) over ALL learners.  The test asserts four times the figure of its order; the campaign's bound is four times the largest.
2. The rate.  us per batch-step and env-steps/s of k_train_tdac_cont on ContinuousMountainCar at 65 536 learners, Fourier orders 1 / 3 / 5, episodes
   capped at 1 000 steps, with the examples' constants (TD SGD(0.01), gamma 0.999, alpha 0.001) -- the Gaussian kernel next to RSRL_CACLA
   (k_train_cacla: the same layout), the Beta kernel next to RSRL_NAC with RSRL_BETA (k_train_nac_beta: the same sampler) and to
   RSRL_ILSTD_ACTOR_CRITIC with RSRL_BETA (k_train_tdac_beta: the agent it stands beside), each group in ONE process on the same build and the
   same seeds, the contexts' timed regions alternating after a warm-up: the median of seven regions and every region.
3. The launch depth.  The order-3 loops of both policies at 256 / 1 024 / 4 096 batch-steps per launch (config.steps_per_launch), the same regions.
One JSON line per figure set and per row; --out writes the markdown tables that profiles/tdac_cont_rate.md holds beside its commentary.
    python scripts/tdac_cont_rate.py [--out FILE] [--regions 7] [--steps 8192] [--warmup 512] [--size 65536] [--orders 1,2,3,4,5] [--rate-orders 1,3,5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import rsrl_amd  # noqa: E402
from tests import tdac_cont_numpy as tn  # noqa: E402
from rate_regions import alternate  # noqa: E402

CMC, TDAC = rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, rsrl_amd.CONTINUOUS_TD_ACTOR_CRITIC
POLICIES = ((rsrl_amd.GAUSSIAN, "Gaussian"), (rsrl_amd.BETA, "Beta"))


def measure(order, policy):
    with rsrl_amd.Context(domain=CMC, order=order, algo=TDAC, policy=policy, n_envs=67) as probe:
        case = tn.handle_case(order, probe.project, policy)
    p = case["params"]
    with rsrl_amd.Context(domain=CMC, order=order, algo=TDAC, policy=policy, n_envs=len(case["init"]), seed=5, gamma=p["gamma"], lr=p["lr"], alpha=p["alpha"]) as c:
        fig, arr = tn.figures(c, None, case)
    fig["conditions_missed"] = tn.keeps_every_learner_in(case, arr["cs"], arr["xs"], arr["want_w"], arr["want_cols"])
    fig["max_abs_column"] = float(np.max(np.abs(arr["want_cols"])))
    fig["max_move"] = float(np.max(np.abs(arr["want_cols"] - np.stack([W for _, W in case["init"]]))))
    return fig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="a file for the markdown tables (default: none, the JSON lines only)")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8192, help="batch-steps per timed region")
    ap.add_argument("--warmup", type=int, default=512)
    ap.add_argument("--size", type=int, default=65536)
    ap.add_argument("--orders", default="1,2,3,4,5")
    ap.add_argument("--rate-orders", default="1,3,5")
    a = ap.parse_args()
    orders = [int(x) for x in a.orders.split(",")]
    figs = {}
    for policy, name in POLICIES:
        for order in orders:
            figs[(name, order)] = measure(order, policy)
            print(json.dumps(dict(policy=name, order=order, figures=figs[(name, order)])), flush=True)
    common = dict(domain=CMC, n_envs=a.size, max_episode_steps=1000, gamma=0.999, seed=0)
    gauss, beta = dict(common, policy=rsrl_amd.GAUSSIAN), dict(common, policy=rsrl_amd.BETA)
    rate_rows = []
    for order in (int(x) for x in a.rate_orders.split(",")):
        rate_rows += alternate([("TD ActorCritic, Gaussian", dict(gauss, algo=TDAC, order=order, lr=0.01, alpha=0.001)),
                                ("CACLA (Gaussian)", dict(gauss, algo=rsrl_amd.CACLA, order=order, lr=0.01, alpha=0.01))], a)
        rate_rows += alternate([("TD ActorCritic, Beta", dict(beta, algo=TDAC, order=order, lr=0.01, alpha=0.001)),
                                ("NAC, Beta (nac_beta.rs)", dict(beta, algo=rsrl_amd.NAC, order=order, lr=0.01, alpha=0.01, n_steps=100)),
                                ("iLSTD ActorCritic, Beta (tdac_beta.rs)", dict(beta, algo=rsrl_amd.ILSTD_ACTOR_CRITIC, order=order, lr=0.00001, alpha=0.001, n_steps=2))], a)
    depth_rows = []
    for kw, name in ((gauss, "Gaussian"), (beta, "Beta")):
        depth_rows += alternate([("%s, %d steps per launch" % (name, d), dict(kw, algo=TDAC, order=3, lr=0.01, alpha=0.001, steps_per_launch=d)) for d in (256, 1024, 4096)], a)
    for r in rate_rows + depth_rows:
        print(json.dumps(r), flush=True)
    if a.out is None:
        return
    cell = lambda r: "%.2f (%.2f .. %.2f)" % (r["us_per_batch_step"], min(r["us_per_batch_step_regions"]), max(r["us_per_batch_step_regions"]))      # noqa: E731
    with open(a.out, "w") as f:
        f.write("## The measured f32 maxima (max |d column| / max(1, |column|) over all 67 learners after three rounds, against the f64 restatement)\n\n")
        f.write("| policy | order | F | the figure | largest |column|, largest move | conditions of handle_case missed |\n|---|---|---|---|---|---|\n")
        for (name, o), g in figs.items():
            f.write("| %s | %d | %d | %.3e | %.3g, %.3g | %s |\n" % (name, o, (o + 1) ** 2, g["cols"], g["max_abs_column"], g["max_move"], "; ".join(g["conditions_missed"]) or "none"))
        f.write("\n## The driver loop's rate (%d learners, cap 1 000; median of %d regions of %d batch-steps after %d of warm-up, and the range)\n\n" %
                (a.size, a.regions, a.steps, a.warmup))
        f.write("| order | agent | kernel | us per batch-step | env-steps/s | time relative to the group's first row | largest |policy column| afterwards, learners with a non-finite column (of the first 256) |\n"
                "|---|---|---|---|---|---|---|\n")
        for r in rate_rows:
            f.write("| %d | %s | `%s` | %s | %.3e | %.3f | %.3g, %d |\n" % (r["order"], r["agent"], r["kernel"], cell(r), r["env_steps_per_s"], r["vs_base"],
                                                                          r["max_abs_policy_column_of_first_256"], r["non_finite_of_first_256"]))
        f.write("\n## The launch depth (order 3, the same regions)\n\n| policy, steps per launch | launches per region | us per batch-step |\n|---|---|---|\n")
        for r in depth_rows:
            f.write("| %s | %d | %s |\n" % (r["agent"], r["launches_per_region"], cell(r)))


if __name__ == "__main__":
    main()
