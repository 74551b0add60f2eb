"""The checkpoint files, byte for byte: every payload layout (aux_kind 0..8, the epsilon schedule's version 4, the weight layouts behind the
accessors) written by the recipe of tests/golden/make_checkpoint_digests.py must have the size and sha256 recorded in
tests/golden/checkpoint_digests.json, and must load into a fresh ctx of the same configuration that then checksums like its writer."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recipe():
    spec = importlib.util.spec_from_file_location("make_checkpoint_digests", os.path.join(ROOT, "tests", "golden", "make_checkpoint_digests.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


RECIPE = _recipe()


def test_fixture_covers_every_case_and_every_aux_kind():
    want = json.load(open(RECIPE.FIXTURE))
    assert sorted(want) == sorted(RECIPE.CASES)
    assert {v["aux_kind"] for v in want.values()} == set(range(9)) and 4 in {v["version"] for v in want.values()}
    for name, (_, _, version, aux_kind) in RECIPE.CASES.items():
        assert (want[name]["version"], want[name]["aux_kind"]) == (version, aux_kind), name


@pytest.mark.parametrize("name", sorted(RECIPE.CASES))
def test_file_is_the_recorded_one_and_loads_back(tmp_path, name):
    import rsrl_amd
    want = json.load(open(RECIPE.FIXTURE))[name]
    got, sums = RECIPE.digests(str(tmp_path), [name])
    print(name, got[name], "recorded:", want)
    assert got[name]["bytes"] == want["bytes"], name
    assert got[name]["sha256"] == want["sha256"], name
    assert (got[name]["version"], got[name]["aux_kind"]) == (want["version"], want["aux_kind"])
    # the reader: a fresh ctx of the same configuration, reset like the writer (the checksum's second word covers the env state, which is
    # not in the file), then trained nothing -- the writer's env state is put back through the setters
    kw, steps, _, _ = RECIPE.CASES[name]
    with rsrl_amd.Context(**kw) as w, rsrl_amd.Context(**kw) as r:
        w.reset()
        w.train(steps, want_stats=False)
        assert w.checksum() == sums[name], "training is not reproducible: the recipe rests on it"
        r.load_weights(os.path.join(str(tmp_path), name + ".ckpt"))
        assert r.step_count == w.step_count
        assert r.checksum()[0] == sums[name][0], name          # the learned state: W, the auxiliary matrix, the f64 least-squares state
        r.states, r.actions, r.episode_steps = w.states, w.actions, w.episode_steps
        assert r.checksum() == sums[name], name


def test_headers_this_library_never_wrote_are_refused(tmp_path):
    import struct
    import rsrl_amd
    name = "sarsa_lambda"                                               # aux_kind 1, written as version 2
    path = os.path.join(str(tmp_path), name + ".ckpt")
    RECIPE.write_case(name, path)
    raw = bytearray(open(path, "rb").read())
    kw = RECIPE.CASES[name][0]
    with rsrl_amd.Context(**kw) as r:
        before = r.checksum()
        for version, needle in ((99, "reads versions 2, 3, 4, 5, 6, 7, 8, 9 and 10"), (3, "not a valid pairing"), (5, "not a valid pairing"), (7, "not a valid pairing")):
            struct.pack_into("<I", raw, 8, version)
            bad = os.path.join(str(tmp_path), f"v{version}.ckpt")
            open(bad, "wb").write(raw)
            with pytest.raises(rsrl_amd.RsrlHipError, match=needle) as ei:
                r.load_weights(bad)
            assert ei.value.code == -1 and r.checksum() == before       # EINVAL, the ctx untouched
        struct.pack_into("<I", raw, 8, 2)
        struct.pack_into("<i", raw, 12 + 10 * 4, 9)                     # an aux_kind beyond the table
        open(bad, "wb").write(raw)
        with pytest.raises(rsrl_amd.RsrlHipError, match="not a valid pairing"):
            r.load_weights(bad)
        assert r.checksum() == before
