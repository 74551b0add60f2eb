"""NAC over the Gibbs policy (RSRL_GIBBS_NAC, k_train_gibbs_nac): the driver loop's rate at three launch depths.

us per batch-step and env-steps/s at 65 536 MountainCar order-3 learners with examples/nac_softmax.cpp's constants (the critic's SGD(0.01), gamma
0.999, NAC.alpha 0.01, tau 1, the actor's period 100, episodes capped at 1 000 steps) at 256 / 1 024 / 4 096 batch-steps per launch
(config.steps_per_launch) -- next to RSRL_ACTOR_CRITIC (k_train_ac, a2c.cpp's constants) and RSRL_NAC with RSRL_GAUSSIAN (k_train_nac_gauss, nac.cpp's
constants, on ContinuousMountainCar) in ONE process on the same build, the contexts' timed regions alternating after a warm-up
(scripts/rate_regions.py): the median of the regions and their range.  One JSON line per row; --out writes the markdown table that
profiles/gibbs_nac_rate.md holds beside its commentary.
    python scripts/gibbs_nac_rate.py [--out FILE] [--regions 7] [--steps 8192] [--warmup 512] [--size 65536]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import rsrl_amd  # noqa: E402
from rate_regions import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="a file for the markdown table (default: none, the JSON lines only)")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8192, help="batch-steps per timed region")
    ap.add_argument("--warmup", type=int, default=512)
    ap.add_argument("--size", type=int, default=65536)
    a = ap.parse_args()
    mc = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, policy=rsrl_amd.SOFTMAX, n_envs=a.size, max_episode_steps=1000, seed=0)
    gnac = dict(mc, algo=rsrl_amd.GIBBS_NAC, lr=0.01, gamma=0.999, alpha=0.01, tau=1.0, n_steps=100)
    agents = [("NAC over the Gibbs policy, %d steps per launch" % d, dict(gnac, steps_per_launch=d)) for d in (256, 1024, 4096)]
    agents.append(("ActorCritic (a2c.rs), 4096 steps per launch", dict(mc, algo=rsrl_amd.ACTOR_CRITIC, lr=0.001, gamma=1.0, alpha=0.001, tau=1.0)))
    agents.append(("NAC, Gaussian policy (nac.rs), 256 steps per launch",
                   dict(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, order=3, policy=rsrl_amd.GAUSSIAN, algo=rsrl_amd.NAC, n_envs=a.size, max_episode_steps=1000, seed=0,
                        lr=0.01, gamma=0.999, alpha=0.01, n_steps=100)))
    rows = alternate(agents, a, base=3)
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out is None:
        return
    cell = lambda r: "%.2f (%.2f .. %.2f)" % (r["us_per_batch_step"], min(r["us_per_batch_step_regions"]), max(r["us_per_batch_step_regions"]))      # noqa: E731
    with open(a.out, "w") as f:
        f.write("## The driver loop's rate (%d order-3 learners, cap 1 000; median of %d regions of %d batch-steps after %d of warm-up, and the range)\n\n" %
                (a.size, a.regions, a.steps, a.warmup))
        f.write("| agent | kernel | launches per region | us per batch-step | env-steps/s | time relative to k_train_ac's | largest |theta| afterwards, learners with a "
                "non-finite matrix (of the first 256) |\n|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | `%s` | %d | %s | %.3e | %.3f | %.3g, %d |\n" % (r["agent"], r["kernel"], r["launches_per_region"], cell(r), r["env_steps_per_s"], r["vs_base"],
                                                                          r["max_abs_policy_column_of_first_256"], r["non_finite_of_first_256"]))


if __name__ == "__main__":
    main()
