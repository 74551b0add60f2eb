"""Driver-loop rate of the thread-per-learner agents of the register family: us per batch-step and env-steps/s of each named agent's kernel on
MountainCar at 65 536 and 262 144 learners, Fourier orders 3 and 5.  One JSON line per configuration; every agent by default.  (Replaces
ac_rate.py, tdac_rate.py and reinforce_rate.py, which differed by their agent tables: name the agents a table held to get its rows.)
    python scripts/agent_rate.py [AGENT ...] [--steps 256] [--warmup 32] [--sizes 65536,262144] [--orders 3,5]
--domain / --weight-dtype reach the other kernel families: `TD TDLambda GreedyGQ SARSALambda QLambda QSigma --domain acrobot --orders 7
--sizes 8192 [--weight-dtype bf16]` times the order-7 wave family's memory-sweep kernels (k_wave_aux, k_wave_lambda, k_wave_qsigma)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rsrl_amd  # noqa: E402

EG = dict(policy=rsrl_amd.EPSILON_GREEDY, epsilon=0.1)
PG = dict(policy=rsrl_amd.SOFTMAX, alpha=0.001, gamma=0.99)
AGENTS = {
    "TD": dict(algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM, lr=0.001, gamma=0.99),
    "TDLambda": dict(algo=rsrl_amd.TD_LAMBDA, policy=rsrl_amd.RANDOM, lam=0.7, lr=0.001, gamma=0.99),
    "GTD2": dict(algo=rsrl_amd.GTD2, policy=rsrl_amd.RANDOM, lr=0.001, lr_td=0.002, gamma=0.99),
    "TDC": dict(algo=rsrl_amd.TDC, policy=rsrl_amd.RANDOM, lr=0.001, lr_td=0.002, gamma=0.99),
    "GreedyGQ": dict(algo=rsrl_amd.GREEDY_GQ, lr_td=0.001, lr=0.001, gamma=1.0, **EG),
    "SARSALambda": dict(algo=rsrl_amd.SARSA_LAMBDA, lam=0.7, alpha=0.01, gamma=0.99, **EG),
    "QLambda": dict(algo=rsrl_amd.Q_LAMBDA, lam=0.7, alpha=0.01, gamma=0.99, **EG),
    "QSigma": dict(algo=rsrl_amd.Q_SIGMA, sigma=0.5, n_steps=4, lr=0.001, gamma=0.99, **EG),
    "ActorCritic": dict(algo=rsrl_amd.ACTOR_CRITIC, policy=rsrl_amd.SOFTMAX, alpha=0.001, lr=0.001, gamma=1.0),
    "QActorCritic": dict(algo=rsrl_amd.Q_ACTOR_CRITIC, policy=rsrl_amd.SOFTMAX, alpha=0.001, lr=0.001, gamma=1.0),
    "TDActorCritic": dict(algo=rsrl_amd.TD_ACTOR_CRITIC, policy=rsrl_amd.SOFTMAX, alpha=0.002, lr=0.01, gamma=0.99),
    "REINFORCE": dict(algo=rsrl_amd.REINFORCE, **PG),
    "BaselineREINFORCE": dict(algo=rsrl_amd.BASELINE_REINFORCE, **PG),
}
DOMAINS = {"mountain_car": rsrl_amd.MOUNTAIN_CAR, "cart_pole": rsrl_amd.CART_POLE, "acrobot": rsrl_amd.ACROBOT}
DTYPES = {"f32": rsrl_amd.W_F32, "bf16": rsrl_amd.W_BF16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("agents", nargs="*", metavar="AGENT", help="of: " + " ".join(AGENTS))
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--sizes", default="65536,262144")
    ap.add_argument("--orders", default="3,5")
    ap.add_argument("--domain", choices=list(DOMAINS), default="mountain_car")
    ap.add_argument("--weight-dtype", choices=list(DTYPES), default="f32")
    a = ap.parse_args()
    unknown = [x for x in a.agents if x not in AGENTS]
    if unknown:
        ap.error("unknown agent " + ", ".join(unknown) + " (of: " + " ".join(AGENTS) + ")")
    for order in [int(x) for x in a.orders.split(",")]:
        for n in [int(x) for x in a.sizes.split(",")]:
            for agent in a.agents or AGENTS:
                with rsrl_amd.Context(domain=DOMAINS[a.domain], order=order, n_envs=n, max_episode_steps=1000, steps_per_launch=a.steps,
                                      weight_dtype=DTYPES[a.weight_dtype], **AGENTS[agent]) as c:
                    c.reset()
                    c.train(a.warmup, want_stats=False)
                    c.sync()
                    c.timing_enable(True)
                    c.train(a.steps, want_stats=False)
                    ms, launches, name = c.timing_read()
                    us = ms * 1e3 / a.steps
                    print(json.dumps(dict(agent=agent, kernel=name, order=order, features=c.F, n_envs=n, batch_steps=a.steps, launches=launches,
                                          us_per_batch_step=round(us, 2), env_steps_per_s=n / (us * 1e-6))), flush=True)


if __name__ == "__main__":
    main()
