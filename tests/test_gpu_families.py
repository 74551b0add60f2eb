"""The kernel family rsrl_hip_create picks, pinned by what the driver loop launches: one configuration per AgentFamily value (ctx.hpp), plus the
variants of a family's kernel name (bf16 wave with and without RSRL_WAVE_PK=0; RegStep learner-major, feature-major and four lanes per learner).
Each row names the kernel timing_read() reports after timing_enable(); train(1) at 64 learners."""
import pytest

import rsrl_amd as ra

pytestmark = pytest.mark.gpu

MC, CP, AB = ra.MOUNTAIN_CAR, ra.CART_POLE, ra.ACROBOT
TILE = dict(basis=ra.TILE_CODING, n_tilings=8)
SHARED = dict(weight_mode=ra.W_SHARED)
TDK = dict(policy=ra.RANDOM, lam=0.5)
LAM = dict(lam=0.5)

# (family, environment switches, Context arguments, kernel)
FAMILIES = [
    ("SharedDense", {"RSRL_NO_PERSIST": "1"}, dict(domain=MC, order=3, **SHARED), "k_shared_step"),
    ("SharedTile", {}, dict(domain=MC, **TILE, **SHARED), "k_shared_ca"),
    ("SharedSparseLambda", {}, dict(domain=MC, algo=ra.SARSA_LAMBDA, **LAM, **TILE, **SHARED), "k_sparse_trace_scatter"),
    ("WaveAux", {}, dict(domain=CP, order=7, algo=ra.GREEDY_GQ), "k_wave_aux"),
    ("TdTile", {}, dict(domain=MC, algo=ra.TD, **TDK, **TILE), "k_td_tile"),
    ("TdGeneric", {}, dict(domain=CP, order=2, algo=ra.TD_LAMBDA, **TDK), "k_td_mem"),
    ("TdReg", {}, dict(domain=MC, order=3, algo=ra.TD, **TDK), "k_train_td"),
    ("WaveQSigma", {}, dict(domain=AB, order=7, algo=ra.Q_SIGMA, sigma=0.5, n_steps=2), "k_wave_qsigma"),
    ("QSigmaReg", {}, dict(domain=MC, order=3, algo=ra.Q_SIGMA, sigma=0.5, n_steps=2), "k_train_qsigma"),
    ("QSigmaGeneric", {}, dict(domain=MC, algo=ra.Q_SIGMA, sigma=0.5, n_steps=2, **TILE), "k_train_qsigma"),
    ("GqReg", {}, dict(domain=MC, order=3, algo=ra.GREEDY_GQ, lr_td=0.001), "k_train_gq"),
    ("GqGeneric", {}, dict(domain=CP, order=2, algo=ra.GREEDY_GQ, lr_td=0.001), "k_train_gq_mem"),
    ("LambdaTile", {}, dict(domain=MC, algo=ra.SARSA_LAMBDA, **LAM, **TILE), "k_lambda_tile"),
    ("WaveLambda", {}, dict(domain=AB, order=7, algo=ra.SARSA_LAMBDA, **LAM), "k_wave_lambda"),
    ("LambdaGeneric", {}, dict(domain=CP, order=2, algo=ra.Q_LAMBDA, **LAM), "k_train_lambda_mem"),
    ("LambdaReg", {}, dict(domain=MC, order=3, algo=ra.SARSA_LAMBDA, **LAM), "k_train_lambda"),
    ("WaveControl-f32", {}, dict(domain=CP, order=7), "k_train_wave"),
    ("WaveControl-bf16", {}, dict(domain=CP, order=7, weight_dtype=ra.W_BF16), "k_train_wave_pk"),
    ("WaveControl-bf16-no-pk", {"RSRL_WAVE_PK": "0"}, dict(domain=CP, order=7, weight_dtype=ra.W_BF16), "k_train_wave"),
    ("RegStep-learner-major", {}, dict(domain=MC, order=3, steps_per_launch=1), "k_step_reg_lm"),
    ("RegStep-feature-major", {"RSRL_K1_FEATURE_MAJOR": "1"}, dict(domain=MC, order=3, steps_per_launch=1), "k_step_reg"),
    ("RegStep-quad", {"RSRL_K1_QUAD": "1"}, dict(domain=MC, order=3, steps_per_launch=1), "k_step_reg_q4"),
    ("RegFused", {}, dict(domain=MC, order=3), "k_train_reg"),
    ("Generic-tile", {}, dict(domain=MC, **TILE), "k_train_mem"),
    ("Generic-fourier", {}, dict(domain=CP, order=2), "k_train_mem"),
    ("Hiv", {}, dict(domain=ra.HIV_TREATMENT, order=1), "k_hiv_train"),
    ("AcReg", {}, dict(domain=MC, order=3, algo=ra.ACTOR_CRITIC, policy=ra.SOFTMAX), "k_train_ac"),
]


@pytest.mark.parametrize("env,kw,kernel", [row[1:] for row in FAMILIES], ids=[row[0] for row in FAMILIES])
def test_family_launches_its_kernel(monkeypatch, env, kw, kernel):
    for k, v in env.items():                 # (the switches are read when the ctx is created)
        monkeypatch.setenv(k, v)
    kw = dict(dict(policy=ra.EPSILON_GREEDY), **kw)
    with ra.Context(n_envs=64, seed=3, max_episode_steps=50, **kw) as c:
        c.reset()
        c.timing_enable(True)
        st = c.train(1)
        assert st["env_steps"] == 64
        assert c.timing_read()[2] == kernel
