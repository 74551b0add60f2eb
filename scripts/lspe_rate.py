"""LambdaLSPE's driver-loop rate: us per batch-step and env-steps/s of k_train_lspe next to k_train_lstd_batch (LSTD, LSTDLambda: the same lane
layout, record and elimination; LSTDLambda's row work is this agent's -- one f64 feature, one LDS vector, F products per lane), in one process on the
same configuration: MountainCar order 3, cap 200, 65 536 learners.  All ctxs are warmed up (every learner past two episode ends), then timed in
alternating regions of --steps batch-steps by the library's device events; the figure is the median region, and every region is listed.  Then, per
agent, where the time goes: from a reset every episode is in step, so train(cap - 1) holds no episode end (the forward step) and the train(1) behind
it holds every learner's sweep and solve; rsrl_hip_lstd_solve alone is the wall clock around the synchronous call.  Then the solves' tally: a fresh
LambdaLSPE ctx at the run's cap and one at a cap below F run 20 caps from a reset; the abandoned solves are the learners' singular_solves, the row
counts, theta and the counters are read from a checkpoint, and -- every episode of the run being cut at the cap -- the deferred and performed solves
follow from the row rule on the host, which the learners' row counts must confirm.  One JSON line per measurement.
    python scripts/lspe_rate.py [--steps 2000] [--regions 7] [--n 65536] [--cap 200] [--order 3]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rsrl_amd  # noqa: E402


def region(c, steps):
    c.timing_enable(True)
    c.train(steps, want_stats=False)
    ms, launches, name = c.timing_read()
    c.timing_enable(False)
    return ms * 1e3 / steps, launches, name


def tally(kw, cap, n_caps):
    """20 caps of the driver loop from a reset -> the solves' counts and theta's size"""
    with rsrl_amd.Context(algo=rsrl_amd.LAMBDA_LSPE, **dict(kw, max_episode_steps=cap)) as c, tempfile.TemporaryDirectory() as tmp:
        c.reset()
        st = c.train(n_caps * cap)
        path = os.path.join(tmp, "lspe.ckpt")
        c.save_weights(path)
        N, F = c.N, c.F
        raw = open(path, "rb").read()[72:]
        theta = np.frombuffer(raw, dtype=np.float64, count=N * F)
        pair = np.frombuffer(raw, dtype=np.float64, count=2 * N, offset=8 * N * (F + F * F + F)).reshape(N, 2)
        sing = np.frombuffer(raw, dtype=np.uint32, count=N, offset=8 * N * (F + F * F + F + 2))
        out = dict(measure="tally", cap=cap, features=F, batch_steps=n_caps * cap, episodes=st["episodes"], episodes_truncated=st["episodes_truncated"],
                   abandoned_solves=int(sing.sum()), theta_nonfinite=int((~np.isfinite(theta)).sum()),
                   theta_abs_max=float(np.nanmax(np.abs(theta))), theta_abs_median_of_learner_max=float(np.nanmedian(np.abs(theta.reshape(N, F)).max(axis=1))))
        if st["episodes"] == st["episodes_truncated"] == N * n_caps:      # every batch holds `cap` rows: the row rule on the host
            rows, deferred, full = F, 0, 0
            for _ in range(n_caps):
                rows = min(rows + cap, F)
                if rows == F:
                    full, rows = full + 1, 0
                else:
                    deferred += 1
            # a full-row solve that was abandoned keeps its F rows; a performed one leaves 0
            agree = bool(np.all((pair[:, 1] == rows) | ((pair[:, 1] == F) & (sing > 0))))
            out.update(deferred_solves=deferred * N, full_row_solves=full * N, performed_solves=full * N - int(sing.sum()), row_counts_confirm=agree)
        return out


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
    kw = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=a.order, max_episode_steps=a.cap, n_envs=a.n, policy=rsrl_amd.RANDOM, gamma=0.99, lam=0.8, alpha=0.5, seed=1)
    algos = (("lstd", rsrl_amd.LSTD), ("lstd_lambda", rsrl_amd.LSTD_LAMBDA), ("lambda_lspe", rsrl_amd.LAMBDA_LSPE))
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
        print(json.dumps(dict(measure="steady", features=ctxs[0][1].F, n_envs=a.n, cap=a.cap, batch_steps=a.steps, regions=a.regions, kernels=names,
                              us_per_batch_step={k: round(v, 3) for k, v in med.items()}, regions_us={k: [round(x, 3) for x in v] for k, v in us.items()},
                              env_steps_per_s=rate, vs_lstd_lambda={k: round(rate[k] / rate["lstd_lambda"], 3) for k in ("lstd", "lambda_lspe")},
                              warmup_mean_episode={k: round(w["sum_episode_steps"] / max(1, w["episodes"]), 1) for k, w in warm.items()})), flush=True)
        for tag, c in ctxs:
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
                                  us_per_row_of_the_end=round(e / a.cap, 3), lstd_solve_call_us=round(solve_us, 1),
                                  sweep_and_solve_share=round(e / (e + f * (a.cap - 1)), 3))), flush=True)
    finally:
        for _, c in ctxs:
            c.close()
    F = (a.order + 1) ** 2
    for cap in (a.cap, max(1, F - 6)):
        print(json.dumps(tally(kw, cap, 20)), flush=True)


if __name__ == "__main__":
    main()
