"""Which configurations rsrl_hip_create admits, pinned without a GPU.  Every admission rule runs before the device query, so on a machine
without a device an admitted configuration returns EHIP ("no device") and a refused one EINVAL.  The sweep (scripts/admission_matrix.py, 133 120
configurations) must admit exactly the configurations of tests/golden/create_admission.json, which that script wrote from the library; its second
grid (the algos numbered 13-19 on the same other axes, 71 680 configurations) those of tests/golden/create_admission_agents.json."""
import importlib.util
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def matrix():
    spec = importlib.util.spec_from_file_location("admission_matrix", os.path.join(ROOT, "scripts", "admission_matrix.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _gfx950_visible():
    try:
        return subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True).stdout.count("gfx950") > 0
    except Exception:
        return False


def test_grid_covers_every_admission_axis(matrix):
    grid = dict(matrix.GRID)
    need = {"domain": {0, 1, 2, 3}, "basis": {0, 1}, "order": {1, 2, 3, 5, 7}, "n_tilings": {4, 8}, "algo": set(range(13)), "policy": {0, 1, 2, 3},
            "weight_mode": {0, 1}, "weight_dtype": {0, 1}, "agent_policy": {-1, 2}, "epsilon_decay": {1.0, 0.99}, "steps_per_launch": {0, 1}}
    for name, vals in need.items():
        assert vals <= set(grid[name]), name
    assert json.load(open(matrix.FIXTURE))["grid"] == [[n, v] for n, v in matrix.GRID], "GRID and the fixture drifted apart"


def test_create_admits_exactly_the_fixture(matrix):
    if _gfx950_visible():
        pytest.skip("GPU present: an admitted configuration would create a real ctx")
    from rsrl_amd import _build
    _build.build()
    res = matrix.sweep()
    assert any(rc == matrix.EHIP and "device" in msg for rc, msg in res.values())
    assert matrix.admitted(res) == json.load(open(matrix.FIXTURE))["admitted"]
    for key, (rc, msg) in res.items():
        if rc != matrix.EHIP:
            assert rc == matrix.EINVAL and msg, (key, rc, msg)


def test_the_two_grids_cover_every_algo_on_the_same_axes(matrix):
    algos = set(dict(matrix.GRID)["algo"]) | set(dict(matrix.GRID_AGENTS)["algo"])
    assert algos >= set(range(20)), sorted(set(range(20)) - algos)
    assert [n for n, _ in matrix.GRID] == [n for n, _ in matrix.GRID_AGENTS]
    assert all(v == w for (n, v), (_, w) in zip(matrix.GRID, matrix.GRID_AGENTS) if n != "algo"), "the second grid's other axes are the first's"
    assert json.load(open(matrix.AGENTS_FIXTURE))["grid"] == [[n, v] for n, v in matrix.GRID_AGENTS], "GRID_AGENTS and its fixture drifted apart"


def test_create_admits_exactly_the_agents_fixture(matrix):
    """the TD ActorCritic, REINFORCE / BaselineREINFORCE and RecursiveLSTD / iLSTD on the configurations their rules admit; 14 and 17 (no algo) nowhere"""
    if _gfx950_visible():
        pytest.skip("GPU present: an admitted configuration would create a real ctx")
    from rsrl_amd import _build
    _build.build()
    res = matrix.sweep(matrix.GRID_AGENTS)
    want = json.load(open(matrix.AGENTS_FIXTURE))["admitted"]
    assert matrix.admitted(res) == want
    algos = dict(matrix.GRID_AGENTS)["algo"]
    ia = [n for n, _ in matrix.GRID_AGENTS].index("algo")
    assert {algos[int(k[ia], 16)] for k in want} == {13, 15, 16, 18, 19}
    for key, (rc, msg) in res.items():
        if rc != matrix.EHIP:
            assert rc == matrix.EINVAL and msg, (key, rc, msg)
        if algos[int(key[ia], 16)] in (14, 17):
            assert rc == matrix.EINVAL and "unknown algo" in msg, (key, rc, msg)


def test_the_campaign_samplers_draw_only_admitted_configurations(matrix):
    """2 000 draws of each random campaign's sampler (tests/fuzz_parity.py, tests/fuzz_agents.py): rsrl_hip_create admits every one (EHIP -- no device
    -- and not EINVAL), so that a sampler that drifts from the admission rules shows up here and not as refused cases on the GPU"""
    if _gfx950_visible():
        pytest.skip("GPU present: an admitted configuration would create a real ctx")
    import sys

    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fuzz_agents
    import fuzz_parity
    import rsrl_amd as ra
    from rsrl_amd import _build
    _build.build()
    for name, draw in (("fuzz_parity", lambda rng: fuzz_parity.sample(rng)[1]), ("fuzz_agents", fuzz_agents.sample)):
        rng = np.random.default_rng(20261016)
        for k in range(2000):
            kw = draw(rng)
            with pytest.raises(ra.RsrlHipError) as e:
                ra.Context(**kw).close()
            assert e.value.code == matrix.EHIP, (name, k, kw, str(e.value))


def test_learner_ids_must_fit_32_bits():
    # n_envs + env_offset == 2^32 is one id too many (the device's gid is a uint32_t and 2^32 - 1 is kept free); one less is admitted -- without a
    # device that shows as EHIP ("no device"), with one as a ctx
    import rsrl_amd as ra
    for n, off in ((130, (1 << 32) - 130), (1, (1 << 32) - 1), (64, 1 << 32), (1, -1)):
        with pytest.raises(ra.RsrlHipError, match="global env ids must fit 32 bits") as e:
            ra.Context(n_envs=n, env_offset=off)
        assert e.value.code == -1, (n, off)
    for n, off in ((130, (1 << 32) - 1 - 130), (130, (1 << 31) - 65)):
        try:
            ra.Context(n_envs=n, env_offset=off).close()
        except ra.RsrlHipError as e:
            assert e.code == -2 and "device" in str(e), (n, off, str(e))


def test_negative_softmax_temperatures_are_refused():
    """tau < 0 is EINVAL wherever a Softmax reads it (the behaviour policy's tau, the agent's own agent_tau; the Gibbs-actor agents require Softmax), with
    the reason; |tau| < 1e-7 keeps the reference's own message; a policy that does not read tau admits any value.  Admitted configurations answer EHIP
    ("no device") without a GPU, or become a ctx with one"""
    import rsrl_amd as ra

    def create(**kw):
        try:
            ra.Context(n_envs=4, **kw).close()
            return 0, ""
        except ra.RsrlHipError as e:
            return e.code, str(e)

    why = "only positive Softmax temperatures are evaluated"
    for kw in (dict(policy=ra.SOFTMAX, tau=-1.0), dict(policy=ra.SOFTMAX, tau=-0.05), dict(policy=ra.SOFTMAX, tau=-1e-7), dict(policy=ra.SOFTMAX, tau=float("-inf")),
               dict(algo=ra.SARSA, policy=ra.EPSILON_GREEDY, agent_policy=ra.SOFTMAX, agent_tau=-0.5),
               dict(algo=ra.EXPECTED_SARSA, policy=ra.SOFTMAX, tau=1.0, agent_policy=ra.SOFTMAX, agent_tau=-2.0),
               dict(order=3, algo=ra.ACTOR_CRITIC, policy=ra.SOFTMAX, tau=-1.0), dict(order=3, algo=ra.TD_ACTOR_CRITIC, policy=ra.SOFTMAX, tau=-1.0),
               dict(order=3, algo=ra.REINFORCE, policy=ra.SOFTMAX, tau=-0.7), dict(order=1, algo=ra.ILSTD_ACTOR_CRITIC, n_steps=2, policy=ra.SOFTMAX, tau=-1.0)):
        rc, msg = create(**kw)
        assert rc == -1 and why in msg and "overflow fp32" in msg, (kw, rc, msg)
        assert ("agent_tau" in msg) == ("agent_tau" in kw), (kw, msg)
    for kw in (dict(policy=ra.SOFTMAX, tau=-1e-8), dict(policy=ra.SOFTMAX, tau=0.0), dict(algo=ra.SARSA, agent_policy=ra.SOFTMAX, agent_tau=-1e-9)):
        rc, msg = create(**kw)
        assert rc == -1 and "Tau parameter in Softmax must be non-zero" in msg, (kw, rc, msg)
    for kw in (dict(policy=ra.SOFTMAX, tau=1e-7), dict(policy=ra.SOFTMAX, tau=1e6), dict(policy=ra.GREEDY, tau=-1.0), dict(policy=ra.EPSILON_GREEDY, tau=-1.0, agent_tau=-1.0),
               dict(algo=ra.SARSA, policy=ra.SOFTMAX, tau=0.5, agent_policy=ra.GREEDY, agent_tau=-3.0)):
        rc, msg = create(**kw)
        assert rc in (0, -2) and (rc == 0 or "device" in msg), (kw, rc, msg)
