"""The episode counts tests/test_gpu_group_frame.py's Random-policy rows must show, on the CPU: the f32 oracle's domains stepped from the test's
own start_states with the driver loop's draws (BLK_INIT at reset, BLK_STEP per step, BLK_RESET after a cut).  Prints terminal and truncated
episodes for the whole run and on both sides of each cut -- run it before recording EXPECTED; change the starts, not the assertion, if a row
misses.  (The two actor-critics' MountainCar starts end their first step whatever the action, so these counts are theirs too.)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import oracle as orc  # noqa: E402
from tests.test_gpu_group_frame import CAP, CUTS, N, SEED, STEPS, start_states  # noqa: E402

BLK_STEP, BLK_RESET, BLK_INIT = 0, 1, 3
DOMAINS = {"MountainCar": (orc.MOUNTAIN_CAR, 3), "CartPole": (orc.CART_POLE, 2), "Acrobot": (orc.ACROBOT, 3)}


def sample(n_actions, i, t, block):
    return orc.policy_sample(orc.RANDOM, np.zeros(n_actions), orc.draw(SEED, i, t, block))


def main():
    orc.lib()
    for name, (dom, A) in DOMAINS.items():
        restart = np.array(orc.domain_reset(dom, prec="f32"), dtype=np.float32)
        s0, ep0 = start_states(name, np.repeat(restart[:, None], N, axis=1))
        ends = []                                              # (batch-step, 'terminal' | 'truncated')
        for i in range(N):
            s, ep, a = s0[:, i].copy(), int(ep0[i]), sample(A, i, 0, BLK_INIT)
            for t in range(STEPS):
                ns, _, term = orc.domain_step(dom, s, a, prec="f32")
                ep += 1
                a = sample(A, i, t, BLK_STEP)
                if term or ep >= CAP:
                    ends.append((t, "terminal" if term else "truncated"))
                    ns, ep = restart, 0
                    if not term:
                        a = sample(A, i, t, BLK_RESET)
                s = np.array(ns, dtype=np.float32)
        for lo, hi in [(0, STEPS)] + [b for cut in CUTS for b in ((0, cut), (cut, STEPS))]:
            count = {k: sum(1 for t, kind in ends if lo <= t < hi and kind == k) for k in ("terminal", "truncated")}
            print(f"{name:12s} steps {lo:2d}..{hi - 1:2d}: {count['terminal']:3d} terminal, {count['truncated']:3d} truncated")


if __name__ == "__main__":
    main()
