"""NAC with the Gaussian policy (RSRL_NAC with RSRL_GAUSSIAN, k_train_nac_gauss): the measured f32 figures behind the bounds of
tests/test_gpu_nac_gaussian.py, and the driver loop's rate.

1. The figures.  The device against the f64 restatement (tests/gaussian_numpy.py: figures) on the GPU tests' own inputs (gaussian_numpy.handle_case:
   67 learners, three rounds of handle_f32) at the Fourier orders 1 / 3 / 5, each max |d x| / max(1, |x|): w, delta, Q, the parameters, the density
   and 64 policy_sample calls.  The tests assert four times each.
2. The rate.  us per batch-step and env-steps/s of k_train_nac_gauss on ContinuousMountainCar at 65 536 learners, Fourier order 3, episodes capped at
   1 000 steps, with nac.rs's constants (critic SGD(0.01), gamma 0.999, NAC.alpha 0.01, the actor's period 100) -- next to RSRL_NAC with RSRL_BETA
   (k_train_nac_beta, nac_beta.rs's constants: the same critic, loop and layout, NAC.alpha 0.1) in ONE process on the same build, the two contexts'
   timed regions alternating: the median region and every region.
One JSON line per figure set and per agent; --out writes the two markdown tables that profiles/nac_gaussian_rate.md holds beside its commentary.
    python scripts/nac_gaussian_rate.py [--out FILE] [--regions 5] [--steps 8192] [--warmup 256] [--size 65536] [--rate-order 3] [--orders 1,3,5]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import rsrl_amd  # noqa: E402
from tests import gaussian_numpy as gn  # noqa: E402
from rate_regions import timed  # noqa: E402

NAMES = ("delta", "w", "q", "mu", "sd", "pdf", "sample")
WHAT = {"delta": "`td_error_out` over the three rounds", "w": "w after the three rounds", "q": "`q_evaluate_f32` (the first round's states; actions -2.5, 1.5 and random in [-1.5, 1.5])",
        "mu": "`policy_params`: mu (`policy_mode_f32` is the same bits)", "sd": "`policy_params`: sd", "pdf": "`policy_pdf` of the first round's actions",
        "sample": "`policy_sample_f32`, 64 calls (4 288 draws)"}


def measure(order):
    case = gn.handle_case(order)
    p = case["params"]
    with rsrl_amd.Context(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, order=order, algo=rsrl_amd.NAC, policy=rsrl_amd.GAUSSIAN, n_envs=len(case["init"]),
                          seed=gn.RULE_SEED, gamma=p["gamma"], lr=p["lr"], alpha=0.1, n_steps=100) as c:
        fig, _ = gn.figures(c, case, gn.RULE_SEED)
    return fig


def rates(a):
    common = dict(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, algo=rsrl_amd.NAC, order=a.rate_order, n_envs=a.size, max_episode_steps=1000, lr=0.01, gamma=0.999,
                  n_steps=100)
    agents = (("NAC, Beta policy (nac_beta.rs)", dict(policy=rsrl_amd.BETA, alpha=0.1)), ("NAC, Gaussian policy (nac.rs)", dict(policy=rsrl_amd.GAUSSIAN, alpha=0.01)))
    ctxs = [rsrl_amd.Context(**dict(common, **kw)) for _, kw in agents]
    rows = []
    try:
        us, meta = timed(ctxs, a.steps, a.regions, a.warmup)
        base = statistics.median(us[0])
        for j, (agent, _) in enumerate(agents):
            med = statistics.median(us[j])
            st = ctxs[j].train(64)                     # (after the timed regions: are the learners still finite?  The first 256 of them say)
            dead = sum(not np.isfinite(ctxs[j].get_weights(i)).all() for i in range(min(256, a.size)))
            rows.append(dict(agent=agent, kernel=meta[j][1], order=a.rate_order, features=ctxs[j].F, n_envs=a.size, batch_steps_per_region=a.steps,
                             launches_per_region=meta[j][0], regions=a.regions, us_per_batch_step=round(med, 3),
                             us_per_batch_step_regions=[round(x, 3) for x in us[j]], env_steps_per_s=a.size / (med * 1e-6),
                             vs_nac_beta=round(base / med, 3), batch_steps_run=int(ctxs[j].step_count),
                             mean_abs_delta_after=st["sum_abs_td_error"] / st["env_steps"], non_finite_of_first_256=int(dead)))
    finally:
        for c in ctxs:
            c.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="a file for the markdown tables (default: none, the JSON lines only)")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8192, help="batch-steps per timed region")
    ap.add_argument("--warmup", type=int, default=256)
    ap.add_argument("--size", type=int, default=65536)
    ap.add_argument("--rate-order", type=int, default=3)
    ap.add_argument("--orders", default="1,3,5")
    a = ap.parse_args()
    orders = [int(x) for x in a.orders.split(",")]
    figs = {}
    for order in orders:
        figs[order] = measure(order)
        print(json.dumps(dict(order=order, figures=figs[order])), flush=True)
    rows = rates(a)
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out is None:
        return
    with open(a.out, "w") as f:
        f.write("## The measured f32 maxima (max |d x| / max(1, |x|) against the f64 restatement)\n\n")
        f.write("| quantity | " + " | ".join("order %d" % o for o in orders) + " |\n|---|" + "---|" * len(orders) + "\n")
        for n in NAMES:
            f.write("| %s | " % WHAT[n] + " | ".join("%.3e" % figs[o][n] for o in orders) + " |\n")
        f.write("\n## The driver loop's rate (%d learners, order %d, cap 1 000, P = 100; median of %d regions of %d batch-steps, and the range)\n\n" %
                (a.size, a.rate_order, a.regions, a.steps))
        f.write("| agent | kernel | us per batch-step | env-steps/s | rate relative to the Beta agent | learners with a non-finite w after %d batch-steps (of the first 256) |\n"
                "|---|---|---|---|---|---|\n" % rows[0]["batch_steps_run"])
        for r in rows:
            f.write("| %s | `%s` | %.2f (%.2f .. %.2f) | %.3e | %.3f | %d |\n" % (r["agent"], r["kernel"], r["us_per_batch_step"], min(r["us_per_batch_step_regions"]),
                                                                               max(r["us_per_batch_step_regions"]), r["env_steps_per_s"], r["vs_nac_beta"],
                                                                               r["non_finite_of_first_256"]))


if __name__ == "__main__":
    main()
