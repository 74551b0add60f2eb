"""Which configurations rsrl_hip_create admits, pinned without a GPU.  Every admission rule runs before the device query, so on a machine
without a device an admitted configuration returns EHIP ("no device") and a refused one EINVAL.  The sweep (scripts/admission_matrix.py, 133 120
configurations) must admit exactly the configurations of tests/golden/create_admission.json, which that script wrote from the library."""
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
