"""NAC's driver-loop rate: us per batch-step and env-steps/s of k_train_nac_beta on ContinuousMountainCar at 65 536 learners, Fourier orders 1 / 3 / 5,
episodes capped at 1 000 steps, with nac_beta.rs's constants (critic SGD(0.01), gamma 0.999, NAC.alpha 0.1, the actor's period 100) -- next to the
Beta-policy iLSTD ActorCritic (k_train_tdac_beta, tdac_beta.rs's constants: the same domain, policy and sampler, one lane group per learner) in ONE
process on the same build, the two contexts' timed regions alternating.  One JSON line per agent and order: the median region and every region;
vs_tdac_beta is the rate relative to k_train_tdac_beta's at the same order.
    python scripts/nac_beta_rate.py [--regions 5] [--steps 8192] [--steps-tdac 2048] [--warmup 256] [--sizes 65536] [--orders 1,3,5] [--spl N]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rsrl_amd  # noqa: E402
from rate_regions import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8192, help="batch-steps per timed region of k_train_nac_beta")
    ap.add_argument("--steps-tdac", type=int, default=2048, help="... of k_train_tdac_beta (its step is far longer)")
    ap.add_argument("--warmup", type=int, default=256)
    ap.add_argument("--sizes", default="65536")
    ap.add_argument("--orders", default="1,3,5")
    ap.add_argument("--spl", type=int, default=0, help="steps per launch (0: the library's default)")
    a = ap.parse_args()
    common = dict(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, policy=rsrl_amd.BETA, max_episode_steps=1000, steps_per_launch=a.spl)
    agents = (("Beta iLSTD ActorCritic", a.steps_tdac, dict(algo=rsrl_amd.ILSTD_ACTOR_CRITIC, lr=1e-5, gamma=0.999, n_steps=2, alpha=0.001)),
              ("NAC (Beta, SCB SARSA critic)", a.steps, dict(algo=rsrl_amd.NAC, lr=0.01, gamma=0.999, alpha=0.1, n_steps=100)))
    for order in [int(x) for x in a.orders.split(",")]:
        for n in [int(x) for x in a.sizes.split(",")]:
            ctxs = [rsrl_amd.Context(order=order, n_envs=n, **dict(common, **kw)) for _, _, kw in agents]
            try:
                us, meta = timed(ctxs, [steps for _, steps, _ in agents], a.regions, a.warmup)
                base = n / (statistics.median(us[0]) * 1e-6)
                for j, (agent, steps, _) in enumerate(agents):
                    med = statistics.median(us[j])
                    rate = n / (med * 1e-6)
                    print(json.dumps(dict(agent=agent, kernel=meta[j][1], order=order, features=ctxs[j].F, n_envs=n, batch_steps_per_region=steps,
                                          launches_per_region=meta[j][0], regions=a.regions, us_per_batch_step=round(med, 3),
                                          us_per_batch_step_regions=[round(x, 3) for x in us[j]], env_steps_per_s=rate,
                                          vs_tdac_beta=round(rate / base, 3))), flush=True)
            finally:
                for c in ctxs:
                    c.close()


if __name__ == "__main__":
    main()
