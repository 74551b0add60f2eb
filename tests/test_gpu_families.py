"""The kernel family rsrl_hip_create picks, pinned by what the driver loop launches: one configuration per AgentFamily value (ctx.hpp), plus the
variants of a family's kernel name (bf16 wave with and without RSRL_WAVE_PK=0; RegStep learner-major, feature-major and four lanes per learner).
Each row names the kernel timing_read() reports after timing_enable(); train(1) at 64 learners.

Two more checks of every row pin what the library reads from its family table (ctx.hpp kFamily) and nothing else holds per family.  The expected values
were taken from the library as it stood BEFORE the table existed (the commit before it, loaded through RSRL_HIP_LIB), not from the table:
  slots     the statistics-slot geometry: 1 100 learners (ragged against 64, 256, 512 and 1 024, more than one slot in every geometry; the LSTD rows at
            order 1), max_episode_steps = 1, train(2) with statistics.  Every step truncates, so episodes == episodes_truncated == sum_episode_steps
            exactly: 2 200 for every row (so no column holds it); a slot array of the wrong size loses counts or reads slots no block wrote.
  launches  the fuse depth: batch-step launches timing_read() counts for train(70) without statistics at 64 learners -- 1 at a depth of 256 or more,
            3 at 32, 5 at 16, 70 where a launch is one batch-step (the shared families, RegStep)."""
import pytest

import rsrl_amd as ra

pytestmark = pytest.mark.gpu

MC, CP, AB = ra.MOUNTAIN_CAR, ra.CART_POLE, ra.ACROBOT
TILE = dict(basis=ra.TILE_CODING, n_tilings=8)
SHARED = dict(weight_mode=ra.W_SHARED)
TDK = dict(policy=ra.RANDOM, lam=0.5)
LAM = dict(lam=0.5)

AC = dict(policy=ra.SOFTMAX)

# (family, environment switches, Context arguments, kernel, launches)
FAMILIES = [
    ("SharedDense", {"RSRL_NO_PERSIST": "1"}, dict(domain=MC, order=3, **SHARED), "k_shared_step", 70),
    ("SharedTile", {}, dict(domain=MC, **TILE, **SHARED), "k_shared_ca", 70),
    ("SharedSparseLambda", {}, dict(domain=MC, algo=ra.SARSA_LAMBDA, **LAM, **TILE, **SHARED), "k_sparse_trace_scatter", 70),
    ("WaveAux", {}, dict(domain=CP, order=7, algo=ra.GREEDY_GQ), "k_wave_aux", 1),
    ("TdTile", {}, dict(domain=MC, algo=ra.TD, **TDK, **TILE), "k_td_tile", 1),
    ("TdGeneric", {}, dict(domain=CP, order=2, algo=ra.TD_LAMBDA, **TDK), "k_td_mem", 1),
    ("TdReg", {}, dict(domain=MC, order=3, algo=ra.TD, **TDK), "k_train_td", 1),
    ("WaveQSigma", {}, dict(domain=AB, order=7, algo=ra.Q_SIGMA, sigma=0.5, n_steps=2), "k_wave_qsigma", 1),
    ("QSigmaReg", {}, dict(domain=MC, order=3, algo=ra.Q_SIGMA, sigma=0.5, n_steps=2), "k_train_qsigma", 1),
    ("QSigmaGeneric", {}, dict(domain=MC, algo=ra.Q_SIGMA, sigma=0.5, n_steps=2, **TILE), "k_train_qsigma", 1),
    ("GqReg", {}, dict(domain=MC, order=3, algo=ra.GREEDY_GQ, lr_td=0.001), "k_train_gq", 1),
    ("GqGeneric", {}, dict(domain=CP, order=2, algo=ra.GREEDY_GQ, lr_td=0.001), "k_train_gq_mem", 1),
    ("LambdaTile", {}, dict(domain=MC, algo=ra.SARSA_LAMBDA, **LAM, **TILE), "k_lambda_tile", 1),
    ("WaveLambda", {}, dict(domain=AB, order=7, algo=ra.SARSA_LAMBDA, **LAM), "k_wave_lambda", 1),
    ("LambdaGeneric", {}, dict(domain=CP, order=2, algo=ra.Q_LAMBDA, **LAM), "k_train_lambda_mem", 1),
    ("LambdaReg", {}, dict(domain=MC, order=3, algo=ra.SARSA_LAMBDA, **LAM), "k_train_lambda", 1),
    ("WaveControl-f32", {}, dict(domain=CP, order=7), "k_train_wave", 1),
    ("WaveControl-bf16", {}, dict(domain=CP, order=7, weight_dtype=ra.W_BF16), "k_train_wave_pk", 1),
    ("WaveControl-bf16-no-pk", {"RSRL_WAVE_PK": "0"}, dict(domain=CP, order=7, weight_dtype=ra.W_BF16), "k_train_wave", 1),
    ("RegStep-learner-major", {}, dict(domain=MC, order=3, steps_per_launch=1), "k_step_reg_lm", 70),
    ("RegStep-feature-major", {"RSRL_K1_FEATURE_MAJOR": "1"}, dict(domain=MC, order=3, steps_per_launch=1), "k_step_reg", 70),
    ("RegStep-quad", {"RSRL_K1_QUAD": "1"}, dict(domain=MC, order=3, steps_per_launch=1), "k_step_reg_q4", 70),
    ("RegFused", {}, dict(domain=MC, order=3), "k_train_reg", 1),
    ("Generic-tile", {}, dict(domain=MC, **TILE), "k_train_mem", 1),
    ("Generic-fourier", {}, dict(domain=CP, order=2), "k_train_mem", 1),
    ("Hiv", {}, dict(domain=ra.HIV_TREATMENT, order=1), "k_hiv_train", 5),
    ("AcReg", {}, dict(domain=MC, order=3, algo=ra.ACTOR_CRITIC, **AC), "k_train_ac", 1),
    ("TdAcReg", {}, dict(domain=MC, order=3, algo=ra.TD_ACTOR_CRITIC, **AC), "k_train_tdac", 1),
    ("ReinforceReg", {}, dict(domain=MC, order=3, algo=ra.REINFORCE, **AC), "k_train_reinforce", 1),
    ("LstdReg-recursive", {}, dict(domain=MC, order=1, algo=ra.RECURSIVE_LSTD, policy=ra.RANDOM), "k_train_lstd", 3),
    ("LstdReg-ilstd", {}, dict(domain=MC, order=1, algo=ra.ILSTD, policy=ra.RANDOM, n_steps=2), "k_train_lstd", 3),
    ("TdAcLstdReg", {}, dict(domain=MC, order=1, algo=ra.ILSTD_ACTOR_CRITIC, n_steps=2, **AC), "k_train_tdac_lstd", 3),
]
IDS = [row[0] for row in FAMILIES]


def context(monkeypatch, env, kw, **more):
    for k, v in env.items():                 # (the switches are read when the ctx is created)
        monkeypatch.setenv(k, v)
    return ra.Context(seed=3, **dict(dict(policy=ra.EPSILON_GREEDY), **kw), **more)


@pytest.mark.parametrize("env,kw,kernel", [row[1:4] for row in FAMILIES], ids=IDS)
def test_family_launches_its_kernel(monkeypatch, env, kw, kernel):
    with context(monkeypatch, env, kw, n_envs=64, max_episode_steps=50) as c:
        c.reset()
        c.timing_enable(True)
        st = c.train(1)
        assert st["env_steps"] == 64
        assert c.timing_read()[2] == kernel


@pytest.mark.parametrize("env,kw", [row[1:3] for row in FAMILIES], ids=IDS)
def test_family_statistics_slots(monkeypatch, env, kw):
    with context(monkeypatch, env, kw, n_envs=1100, max_episode_steps=1) as c:
        c.reset()
        st = c.train(2)
        print("statistics", st)
        assert st["env_steps"] == 2200
        assert (st["episodes"], st["episodes_truncated"], st["sum_episode_steps"]) == (2200, 2200, 2200)


@pytest.mark.parametrize("env,kw,launches", [row[1:3] + row[4:5] for row in FAMILIES], ids=IDS)
def test_family_fuse_depth(monkeypatch, env, kw, launches):
    with context(monkeypatch, env, kw, n_envs=64, max_episode_steps=50) as c:
        c.reset()
        c.timing_enable(True)
        c.train(70, want_stats=False)
        n = c.timing_read()[1]
        print("launches", n)
        assert n == launches
