"""RecursiveLSTD / iLSTD driver-loop rate: us per batch-step and env-steps/s of k_train_lstd on MountainCar at 65 536 and 262 144 learners, Fourier
orders 3 and 5 -- next to k_train_td (TD(0), the register family's prediction agent) on the same shapes as the yardstick.  One JSON line per
configuration; flop_per_learner_step is the f64 arithmetic DESIGN 4.11 counts (7 F^2 for RecursiveLSTD, (4 + 2 n_updates / F) F^2 for iLSTD).
--spl 1 runs the one-step path (the state streams through memory every batch-step, about 2 * 8 F^2 bytes per learner-step) and prints the
box's measured float4 copy bandwidth (rsrl_hip_measure_copy) to compare it with.
    python scripts/lstd_rate.py [--steps 256] [--warmup 32] [--sizes 65536,262144] [--orders 3,5] [--n-updates 1] [--spl N]"""
import ctypes as C
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rsrl_amd  # noqa: E402
from rsrl_amd import _abi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--sizes", default="65536,262144")
    ap.add_argument("--orders", default="3,5")
    ap.add_argument("--n-updates", type=int, default=1)
    ap.add_argument("--spl", type=int, default=0, help="steps per launch (0: --steps)")
    a = ap.parse_args()
    spl = a.spl or a.steps
    if spl == 1:
        gbps = C.c_double()
        _abi.check(_abi.lib().rsrl_hip_measure_copy(0, 1 << 30, 20, C.byref(gbps)))
        print(json.dumps(dict(copy_gb_per_s=round(gbps.value, 1))), flush=True)
    agents = (("RecursiveLSTD", dict(algo=rsrl_amd.RECURSIVE_LSTD, gamma=0.99)),
              ("iLSTD", dict(algo=rsrl_amd.ILSTD, alpha=0.01, gamma=0.99, n_steps=a.n_updates)),
              ("TD", dict(algo=rsrl_amd.TD, lr=0.01, gamma=0.99)))
    for order in [int(x) for x in a.orders.split(",")]:
        for n in [int(x) for x in a.sizes.split(",")]:
            for agent, kw in agents:
                with rsrl_amd.Context(domain=rsrl_amd.MOUNTAIN_CAR, order=order, n_envs=n, policy=rsrl_amd.RANDOM, max_episode_steps=1000,
                                      steps_per_launch=spl, **kw) as c:
                    c.reset()
                    c.train(a.warmup, want_stats=False)
                    c.sync()
                    c.timing_enable(True)
                    c.train(a.steps, want_stats=False)
                    ms, launches, name = c.timing_read()
                    us = ms * 1e3 / a.steps
                    F = c.F
                    flop = {"RecursiveLSTD": 7 * F * F, "iLSTD": (4 * F + 2 * a.n_updates) * F}.get(agent)
                    row = dict(agent=agent, kernel=name, order=order, features=F, n_envs=n, batch_steps=a.steps, launches=launches,
                               us_per_batch_step=round(us, 2), env_steps_per_s=n / (us * 1e-6))
                    if flop:
                        row.update(flop_per_learner_step=flop, f64_tflops=round(flop * n / (us * 1e-6) / 1e12, 3))
                        if spl == 1:                 # the state in and out once per batch-step: theta, the matrix (and iLSTD's mu)
                            nbytes = 2 * 8 * (F * F + F * (2 if agent == "iLSTD" else 1)) * n
                            row.update(state_bytes=nbytes, state_gb_per_s=round(nbytes / (us * 1e-6) / 1e9, 1))
                    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
