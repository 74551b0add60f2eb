"""HIVTreatment without a GPU: the numpy restatement the GPU tests compare against passes the reference's known-answer tests, and the domain
is part of the public interface (header, exports, Python constants)."""
import json
import os
import re

import numpy as np

from tests import hiv_numpy as hv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kat():
    with open(os.path.join(ROOT, "tests", "golden", "hiv_reference_kat.json")) as f:
        return json.load(f)


def test_kat_fixture_is_the_reference_s():
    kat = _kat()
    assert kat["source"] == "reference"
    assert [c["name"] for c in kat["cases"]] == ["test_initial_observation", "test_initial_observation_default", "test_limits"]


def test_numpy_restatement_passes_the_reference_kats():
    for case in _kat()["cases"]:
        obs = hv.observe(np.array(case["state"], dtype=np.float64).reshape(6, 1))[:, 0]
        assert np.max(np.abs(obs - np.array(case["observation"]))) <= 1e-12, case["name"]


def test_default_state_and_actions():
    assert np.array_equal(hv.DEFAULT, np.array(_kat()["cases"][1]["state"]))
    assert hv.DT_STEP == 0.005 and hv.SIM_STEPS == 1000
    assert hv.ALL_ACTIONS.tolist() == [[0.0, 0.0], [0.7, 0.0], [0.0, 0.3], [0.7, 0.3]]


def test_reward_is_taken_from_the_observation():
    obs = hv.observe(hv.DEFAULT.reshape(6, 1))
    r = hv.reward(obs, [3])[0]
    assert r == (1e3 * obs[5, 0] - 0.1 * obs[4, 0] - 2e4 * 0.7 ** 2 - 2e3 * 0.3 ** 2) / 1e5


def test_nan_and_nonpositive_components_clip_as_the_reference():
    y = np.array([np.nan, -1.0, 0.0, np.inf, 1e-300, 1e300]).reshape(6, 1)
    assert hv.observe(y)[:, 0].tolist() == [8.0, 8.0, -5.0, 8.0, -5.0, 8.0]


def test_header_declares_the_domain_and_the_hidden_state_exports():
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_HIV_TREATMENT\s*=\s*3", h)
    assert re.search(r"int rsrl_hip_get_hidden_states\(rsrl_hip_ctx\* ctx, double\* y", h)
    assert re.search(r"int rsrl_hip_set_hidden_states\(rsrl_hip_ctx\* ctx, const double\* y", h)


def test_python_interface():
    import rsrl_amd
    from rsrl_amd import _abi
    assert rsrl_amd.HIV_TREATMENT == 3
    assert "rsrl_hip_get_hidden_states" in _abi.SYMBOLS and "rsrl_hip_set_hidden_states" in _abi.SYMBOLS
    assert callable(rsrl_amd.Context.get_hidden_states) and callable(rsrl_amd.Context.set_hidden_states)
