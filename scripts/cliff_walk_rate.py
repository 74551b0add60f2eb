"""CliffWalk over the tabular Q (train_table.hip): the rate of the two driver loops by launch depth.

us per batch-step and env-steps/s at 65 536 learners, QLearning under EpsilonGreedy 0.1, lr 0.5, gamma 0.9, episodes capped at 1 000 steps: the LDS loop
(k_table_train_lds, RSRL_TABLE_MEM=0) at 16 / 256 / 4 096 batch-steps per launch (config.steps_per_launch) and the forced memory loop
(k_table_train_mem, RSRL_TABLE_MEM=1) at 1 / 16 / 256 -- in ONE process on one build, the contexts' timed regions alternating after a warm-up
(scripts/rate_regions.py, device events): the median of the regions and their range.  One JSON line per row; --out writes the markdown table that
profiles/cliff_walk_rate.md holds beside its commentary.
    python scripts/cliff_walk_rate.py [--out FILE] [--regions 7] [--steps 8192] [--warmup 2048] [--size 65536]

Two more modes serve the counter runs (one `rocprofv3 --pmc <counters> -d DIR --output-format csv -- python scripts/cliff_walk_rate.py --pmc-leg lds|mem`
per counter group, counters alone, no tracing):
    --pmc-leg lds|mem     one short call of one loop: reset, then train(64) twice at 64 batch-steps per launch
    --pmc-summary DIR..   the counters of the k_table_train_* dispatches in the CSV files below DIR.., summed per kernel and counter, as JSON"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import rsrl_amd  # noqa: E402
from rate_regions import timed  # noqa: E402


PMC_STEPS = 64


def pmc_leg(leg, size):
    os.environ["RSRL_TABLE_MEM"] = "1" if leg == "mem" else "0"
    with rsrl_amd.Context(domain=rsrl_amd.CLIFF_WALK, basis=rsrl_amd.TABLE, algo=rsrl_amd.QLEARNING, policy=rsrl_amd.EPSILON_GREEDY, epsilon=0.1, lr=0.5,
                          gamma=0.9, n_envs=size, max_episode_steps=1000, seed=0, steps_per_launch=PMC_STEPS) as c:
        c.reset()
        for _ in range(2):
            c.train(PMC_STEPS, want_stats=False)
        c.sync()
        print(json.dumps(dict(leg=leg, n_envs=size, batch_steps_per_dispatch=PMC_STEPS, dispatches=2, checksum=c.checksum()[0])))


def pmc_summary(dirs):
    import csv
    tot = {}
    for d in dirs:
        for root, _, files in os.walk(d):
            for fn in files:
                if not fn.endswith("counter_collection.csv"):
                    continue
                for row in csv.DictReader(open(os.path.join(root, fn))):
                    k = row["Kernel_Name"]
                    if "k_table_train" not in k:
                        continue
                    k = "k_table_train_lds" if "lds" in k else "k_table_train_mem"
                    e = tot.setdefault(k, {}).setdefault(row["Counter_Name"], [0.0, set()])
                    e[0] += float(row["Counter_Value"]); e[1].add((fn, row["Dispatch_Id"]))
    print(json.dumps({k: {c: dict(sum=v[0], dispatches=len(v[1]), per_batch_step=v[0] / (len(v[1]) * PMC_STEPS)) for c, v in cs.items()} for k, cs in tot.items()},
                     indent=1, sort_keys=True))


def main():
    if "--pmc-summary" in sys.argv:
        return pmc_summary(sys.argv[sys.argv.index("--pmc-summary") + 1:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--pmc-leg", default=None, choices=("lds", "mem"))
    ap.add_argument("--out", default=None, help="a file for the markdown table (default: none, the JSON lines only)")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8192, help="batch-steps per timed region (a quarter of it at one batch-step per launch)")
    ap.add_argument("--warmup", type=int, default=2048)
    ap.add_argument("--size", type=int, default=65536)
    a = ap.parse_args()
    if a.pmc_leg:
        return pmc_leg(a.pmc_leg, a.size)
    kw = dict(domain=rsrl_amd.CLIFF_WALK, basis=rsrl_amd.TABLE, algo=rsrl_amd.QLEARNING, policy=rsrl_amd.EPSILON_GREEDY, epsilon=0.1, lr=0.5, gamma=0.9,
              n_envs=a.size, max_episode_steps=1000, seed=0)
    plan = [("0", d) for d in (16, 256, 4096)] + [("1", d) for d in (1, 16, 256)]
    ctxs = []
    try:
        for mem, depth in plan:      # (the switch is read once, when the ctx is created)
            os.environ["RSRL_TABLE_MEM"] = mem
            ctxs.append(rsrl_amd.Context(steps_per_launch=depth, **kw))
        os.environ.pop("RSRL_TABLE_MEM")
        steps = [max(a.steps // 4, 1) if depth == 1 else a.steps for _, depth in plan]
        us, meta = timed(ctxs, steps, a.regions, a.warmup)
        rows = []
        for j, (mem, depth) in enumerate(plan):
            med = statistics.median(us[j])
            rows.append(dict(loop="memory" if mem == "1" else "LDS", kernel=meta[j][1], steps_per_launch=depth, n_envs=a.size, batch_steps_per_region=steps[j],
                             launches_per_region=meta[j][0], regions=a.regions, us_per_batch_step=round(med, 4),
                             us_per_batch_step_regions=[round(x, 4) for x in us[j]], env_steps_per_s=a.size / (med * 1e-6), checksum=ctxs[j].checksum()[0]))
    finally:
        for c in ctxs:
            c.close()
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out is None:
        return
    with open(a.out, "w") as f:
        f.write("## The two driver loops by launch depth (%d learners, QLearning, EpsilonGreedy 0.1, lr 0.5, gamma 0.9, cap 1 000; median of %d regions after "
                "%d batch-steps of warm-up, and the range)\n\n" % (a.size, a.regions, a.warmup))
        f.write("| loop | kernel | batch-steps per launch | batch-steps per region | launches per region | us per batch-step | env-steps/s |\n|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | `%s` | %d | %d | %d | %.4f (%.4f .. %.4f) | %.3e |\n" % (r["loop"], r["kernel"], r["steps_per_launch"], r["batch_steps_per_region"],
                                                                                   r["launches_per_region"], r["us_per_batch_step"], min(r["us_per_batch_step_regions"]),
                                                                                   max(r["us_per_batch_step_regions"]), r["env_steps_per_s"]))


if __name__ == "__main__":
    main()
