"""LSTD's and LSTDLambda's driver-loop rate: us per batch-step and env-steps/s of k_train_lstd_batch next to k_train_lstd (RecursiveLSTD: the same
lane layout and f64 features, an O(F^2) update at every step where the batch agents append a row and pay O(len F^2 + F^3) when the episode ends), in
one process on the same configuration: MountainCar order 3, cap 200, 65 536 learners.  All ctxs are warmed up (every learner past two episode ends),
then timed in alternating regions of --steps batch-steps by the library's device events; the figure is the median region, and every region is listed.
Then, per batch agent, where the time goes: from a reset every episode is in step, so train(cap - 1) holds no episode end (the forward step) and the
train(1) behind it holds every learner's sweep and solve; rsrl_hip_lstd_solve alone (wall clock around the synchronous call, state loaded from and
stored to memory) bounds the solve's part.  One JSON line per measurement.
    python scripts/lstd_batch_rate.py [--steps 2000] [--regions 7] [--n 65536] [--cap 200] [--order 3]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rsrl_amd  # noqa: E402


def region(c, steps):
    c.timing_enable(True)
    c.train(steps, want_stats=False)
    ms, launches, name = c.timing_read()
    c.timing_enable(False)
    return ms * 1e3 / steps, launches, name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--cap", type=int, default=200)
    ap.add_argument("--order", type=int, default=3)
    a = ap.parse_args()
    if a.regions < 5:
        sys.exit("at least five regions")
    kw = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=a.order, max_episode_steps=a.cap, n_envs=a.n, policy=rsrl_amd.RANDOM, gamma=0.99, lam=0.8, seed=1)
    algos = (("recursive_lstd", rsrl_amd.RECURSIVE_LSTD), ("lstd", rsrl_amd.LSTD), ("lstd_lambda", rsrl_amd.LSTD_LAMBDA))
    ctxs = [(tag, rsrl_amd.Context(algo=al, **kw)) for tag, al in algos]
    try:
        warm = {}
        for tag, c in ctxs:
            c.reset()
            warm[tag] = c.train(2 * a.cap + 64)
            c.sync()
        us, names = {tag: [] for tag, _ in ctxs}, {}
        for _ in range(a.regions):                                  # alternating: a drift of the machine lands on all
            for tag, c in ctxs:
                t, _, names[tag] = region(c, a.steps)
                us[tag].append(t)
        med = {k: statistics.median(v) for k, v in us.items()}
        rate = {k: a.n / (v * 1e-6) for k, v in med.items()}
        print(json.dumps(dict(measure="steady", features=ctxs[1][1].F, n_envs=a.n, cap=a.cap, batch_steps=a.steps, regions=a.regions, kernels=names,
                              us_per_batch_step={k: round(v, 3) for k, v in med.items()}, regions_us={k: [round(x, 3) for x in v] for k, v in us.items()},
                              env_steps_per_s=rate, vs_recursive_lstd={k: round(rate[k] / rate["recursive_lstd"], 3) for k in ("lstd", "lstd_lambda")},
                              warmup_mean_episode={k: round(w["sum_episode_steps"] / max(1, w["episodes"]), 1) for k, w in warm.items()})), flush=True)
        for tag, c in ctxs[1:]:
            fwd, end = [], []
            for _ in range(5):
                c.reset()
                fwd.append(region(c, a.cap - 1)[0])                 # no episode can end: the forward step alone
                c.timing_enable(True)
                st = c.train(1)                                     # every learner's episode ends here: 65 536 sweeps of cap rows and solves
                ms, _, _ = c.timing_read()
                c.timing_enable(False)
                assert st["episodes"] >= a.n - a.n // 100, st
                end.append(ms * 1e3)
            c.sync()
            t0 = time.perf_counter()
            for _ in range(20):
                c.lstd_solve()
            solve_us = (time.perf_counter() - t0) * 1e6 / 20
            f, e = statistics.median(fwd), statistics.median(end)
            print(json.dumps(dict(measure="split", agent=tag, n_envs=a.n, cap=a.cap, forward_us_per_batch_step=round(f, 3), episode_end_step_us=round(e, 1),
                                  lstd_solve_call_us=round(solve_us, 1), sweep_and_solve_share=round(e / (e + f * (a.cap - 1)), 3),
                                  solve_call_share_of_end=round(solve_us / e, 3))), flush=True)
    finally:
        for _, c in ctxs:
            c.close()


if __name__ == "__main__":
    main()
