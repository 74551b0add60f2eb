"""The random campaigns without a GPU.  (1) What the keyed campaigns draw on the slices the GPU suite runs -- the sampled keywords and the host
inputs built without a device -- is what tests/golden/campaign_cases.json recorded (tests/golden/make_campaign_cases.py: the recipe, and when
regenerating is legitimate).  (2) tests/campaign.py on a fake Context over numpy arrays, as tests/test_agent_contract_cpu.py holds the harness:
the runner's lines, summary and exit code, the read-only loop, and the parts of the self leg against a ctx that is flawed in the way each part
exists to find; the functions that draw consume the generator exactly as the spelled-out copies they replaced did."""
import importlib.util
import json
import os
import zlib

import numpy as np
import pytest

import rsrl_amd as ra
from tests import campaign as cg
from tests.agent_contract import diff, join_shards, snapshot, trait_loop
from tests.test_agent_contract_cpu import FakeCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the samplers
def _recipe():
    spec = importlib.util.spec_from_file_location("make_campaign_cases", os.path.join(ROOT, "tests", "golden", "make_campaign_cases.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


RECIPE = _recipe()
with open(RECIPE.FIXTURE) as _f:
    GOLDEN = json.load(_f)


def test_the_golden_file_covers_every_suite_slice():
    from tests import fuzz_cacla, fuzz_episodic, fuzz_gtd, fuzz_tdac_cont
    assert sorted(GOLDEN) == sorted(RECIPE.slices())
    assert sorted(GOLDEN) == sorted(["fuzz_episodic/GradientMC", "fuzz_episodic/LSTD", "fuzz_episodic/LSTDLambda", "fuzz_beta/BetaActorCritic", "fuzz_beta/NAC",
                                     "fuzz_gtd/GTD2,TDC", "fuzz_cacla/CACLA", "fuzz_tdac_cont/Gaussian,Beta"])
    for name, mod in (("fuzz_episodic/LSTD", fuzz_episodic), ("fuzz_beta/NAC", fuzz_episodic), ("fuzz_gtd/GTD2,TDC", fuzz_gtd), ("fuzz_cacla/CACLA", fuzz_cacla),
                      ("fuzz_tdac_cont/Gaussian,Beta", fuzz_tdac_cont)):
        assert (GOLDEN[name]["seed"], GOLDEN[name]["cases"]) == (mod.SUITE_SEED, mod.SUITE_CASES), name
    assert all(len(d["sha256"]) == d["cases"] and len(set(d["sha256"])) == d["cases"] for d in GOLDEN.values())      # (no two cases alike)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_every_suite_case_draws_what_it_drew_when_the_seeds_were_committed(orc, name):
    seed, n, case = RECIPE.slices()[name]
    assert (seed, n) == (GOLDEN[name]["seed"], GOLDEN[name]["cases"])
    moved = [idx for idx in range(n) if RECIPE.digest(*case(idx)) != GOLDEN[name]["sha256"][idx]]
    assert not moved, "%s: cases %s draw something else now" % (name, moved)


def test_the_digest_sees_one_bit_of_one_array_and_one_keyword():
    kw, io = dict(n_envs=3, lr=0.1), dict(T=2, W=np.zeros((3, 2), np.float32), rounds=[(np.arange(3), 1, [0, 2])], planted=None)
    d = RECIPE.digest(kw, io)
    assert RECIPE.digest(dict(lr=0.1, n_envs=3), io) == d                                 # (the keyword set, not its order)
    assert RECIPE.digest(dict(kw, lr=np.nextafter(0.1, 1.0)), io) != d
    io["W"].view(np.uint32)[2, 1] = 1
    assert RECIPE.digest(kw, io) != d
    assert RECIPE.digest(kw, None) != RECIPE.digest(kw, {})


# ---- 2. the frame on a fake ctx
class Ctx(FakeCtx):
    """FakeCtx with what the campaigns call besides: want_stats, the four integer statistics, a checksum, and a checkpoint that holds the weights
    and the step count but NOT `hidden`, a per-learner array that every handle moves and that feeds the weights: a resume needs it carried.
    flaw "env": an agent other than TD sees other draws"""

    def __init__(self, n_envs, flaw=None, **kw):
        super().__init__(n_envs, flaw=flaw, **kw)
        self.hidden = np.zeros(n_envs, np.float32)
        if flaw == "env" and self.cfg.algo != ra.TD:
            self.ids = self.ids + 1

    step_count = property(lambda self: self.t)

    def handle(self, frm, actions, rew, nxt, term):
        super().handle(frm, actions, rew, nxt, term)
        self.hidden = (self.hidden * np.float32(0.5) + self._draw(5)).astype(np.float32)
        self.W[:, 0, 0] += np.float32(0.01) * self.hidden

    def train(self, k, want_stats=True):
        st = super().train(k)
        st.update(episodes=int((self.episode_steps == 0).sum()), episodes_truncated=0, sum_episode_steps=int(self.episode_steps.sum()))
        return st if want_stats else None

    def checksum(self):
        return zlib.crc32(self.W.tobytes() + self.hidden.tobytes()), zlib.crc32(self.states.tobytes() + self.actions.tobytes() + self.episode_steps.tobytes())

    def save_weights(self, path):
        with open(path, "wb") as f:
            np.save(f, self.W)
            np.save(f, np.array(self.t))

    def load_weights(self, path):
        with open(path, "rb") as f:
            self.W, self.t = np.load(f), int(np.load(f))


KW = dict(n_envs=8, max_episode_steps=5, env_offset=40)
K = 30


def full(c):
    out = snapshot(c)
    out["hidden"] = c.hidden.copy()
    return out


def carry(a, b):
    b.hidden = a.hidden.copy()


def flawed(flaw):
    return lambda **kw: Ctx(flaw=flaw, **kw)


def _run(capsys, run_case, n=3, **kw):
    with pytest.raises(SystemExit) as e:
        cg.run(run_case, n, 7, **kw)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == n + 1 and out[-1].startswith("SUMMARY ")
    return e.value.code, out[:-1], json.loads(out[-1][8:])


def test_the_runner_counts_prints_and_exits_zero_when_nothing_failed(capsys):
    legs = {}

    def run_case(idx):
        cg.count(legs, "self")
        return ("refused", "%d REFUSED" % idx, dict(algo=1)) if idx == 2 else ("ok", "%d ok" % idx, dict(algo=idx))
    code, lines, d = _run(capsys, run_case, names={0: "A", 1: "B"}, extras=lambda failures: {"legs": legs, "worst": {"A": 0.5}})
    assert code == 0 and lines == ["0 ok", "1 ok", "2 REFUSED"]
    assert list(d) == ["cases", "seed", "counts", "per_agent", "legs", "worst", "failures"]                        # (the extra keys before the failures)
    assert d == {"cases": 3, "seed": 7, "counts": {"ok": 2, "refused": 1}, "per_agent": {"A": {"ok": 1}, "B": {"ok": 1, "refused": 1}}, "legs": {"self": 3},
                 "worst": {"A": 0.5}, "failures": []}


def test_the_runner_reports_an_exception_as_an_error_and_exits_one(capsys):
    def run_case(idx):
        if idx == 1:
            raise ValueError("a leg fell over")
        return "ok", "%d ok" % idx, dict(algo=0)
    code, lines, d = _run(capsys, run_case, names={0: "A"})
    assert code == 1 and lines[1] == "   1 ERROR ValueError: a leg fell over" and lines[2] == "2 ok"               # (and the run goes on)
    assert d["counts"] == {"ok": 2, "ERROR": 1} and d["per_agent"] == {"A": {"ok": 2}}
    assert d["failures"] == [{"case": 1, "line": lines[1], "config": None}]


def test_the_runner_exits_one_on_a_mismatch_and_on_a_failure_appended_at_the_end(capsys):
    kw = dict(algo=0, n_envs=3)
    code, lines, d = _run(capsys, lambda idx: cg.verdict("%d tag" % idx, kw, ["self: weights"] if idx == 0 else []))
    assert code == 1 and lines[0] == "0 tag  MISMATCH ['self: weights']" and lines[1] == "1 tag  ok"
    assert "per_agent" not in d and d["counts"] == {"MISMATCH": 1, "ok": 2} and d["failures"] == [{"case": 0, "line": lines[0], "config": kw}]
    code, _, d = _run(capsys, lambda idx: cg.verdict("tag", kw, [], "not finite" if idx == 0 else None))
    assert code == 0 and d["counts"] == {"diverged": 1, "ok": 2}                                                   # (diverged is counted, not failed)
    code, _, d = _run(capsys, lambda idx: ("ok", "ok", kw), finish=lambda failures: failures.append({"case": None, "line": "too many left out", "config": None}),
                      extras=lambda failures: {"failures": failures, "failed": len(failures)})
    assert code == 1 and d["failed"] == 1 and list(d)[-2:] == ["failures", "failed"] and d["failures"][0]["line"] == "too many left out"
    code, _, d = _run(capsys, lambda idx: ("MISMATCH", "x", kw, {"case": idx, "legs": ["f64"]}), n=1)              # (a record of the campaign's own)
    assert code == 1 and d["failures"] == [{"case": 0, "legs": ["f64"]}]


def test_the_arguments_parse_as_every_campaign_parsed_them():
    names = {23: "GradientMC", 25: "LSTD"}
    assert cg.parse_cases([]) == (200, 0) and cg.parse_cases(["agents=LSTD", "24"], 100) == (24, 0) and cg.parse_cases(["24", "agents=25", "9"]) == (24, 9)
    assert cg.parse_agents(["24", "9"], names) is None and cg.parse_agents(["agents=LSTD,23"], names) == (25, 23) and cg.parse_agents(["agents=-1"], names) == (-1,)
    assert cg.top_of_ids(dict(env_offset=cg.TOP_OF_IDS, n_envs=65))["env_offset"] == (1 << 32) - 66
    assert cg.top_of_ids(dict(env_offset=64, n_envs=65))["env_offset"] == 64
    a, b = cg.case_rng(5, 3, 25), np.random.default_rng([5, 3, 25])
    assert a.bit_generator.state == b.bit_generator.state
    assert cg.bits(np.array([-0.0, 1.0])).tolist() == [0x80000000, 0x3F800000]


def _refuse(code):
    def call():
        raise ra.RsrlHipError(code, "refused")
    return call


def test_the_read_only_loop_reports_a_moved_checksum_and_a_foreign_error_code():
    rng = np.random.default_rng(0)
    with Ctx(**KW) as c:
        c.reset()
        assert cg.read_only_calls(c, rng, {"states": lambda: c.states}) == ([], ["states"])

        def moves():
            c.W[3, 1, 0] = np.nextafter(c.W[3, 1, 0], np.float32(1))
        assert cg.read_only_calls(c, rng, {"get_weights": moves}) == (["get_weights moved the checksum"], ["get_weights"])
        for code in cg.REFUSALS:
            assert cg.read_only_calls(c, rng, {"q_evaluate": _refuse(code)}) == ([], ["q_evaluate"])
        bad, made = cg.read_only_calls(c, rng, {"q_evaluate": _refuse(-2)})
        assert made == ["q_evaluate"] and len(bad) == 1 and bad[0].startswith("q_evaluate: rsrl_hip error -2")
        calls = {n: (lambda: None) for n in "abcdefgh"}
        made = [cg.read_only_calls(c, rng, calls)[1] for _ in range(200)]
        assert {len(m) for m in made} == {1, 2, 3, 4} and all(len(set(m)) == len(m) for m in made) and {n for m in made for n in m} == set(calls)


def test_the_functions_that_draw_consume_the_generator_as_the_spelled_out_copies_did():
    a, b = np.random.default_rng(11), np.random.default_rng(11)
    for lo, hi in ((1, 4), (0, 3)):
        cuts = sorted(set(int(x) for x in a.integers(1, K, size=int(a.integers(lo, hi)))))
        want = [y - x for x, y in zip([0] + cuts, cuts + [K])]
        stats = [bool(a.integers(0, 2)) for _ in want]
        seen = []
        calls = cg.draw_calls(b, K, lo, hi)
        _, done = cg.split_run(KW, b, K, calls, full, make=lambda **kw: _Spy(seen, **kw))
        assert done == want and sum(want) == K and seen == list(zip(want, stats))
    names = list("abcdefgh")
    want = [names[int(j)] for j in a.permutation(len(names))[: int(a.integers(1, 5))]]
    with Ctx(**KW) as c:
        assert cg.read_only_calls(c, b, {n: (lambda: None) for n in names})[1] == want
    assert a.bit_generator.state == b.bit_generator.state


class _Spy(Ctx):
    def __init__(self, seen, **kw):
        super().__init__(**kw)
        self.seen = seen

    def train(self, k, want_stats=True):
        self.seen.append((k, want_stats))
        return super().train(k, want_stats)


def test_the_split_part_fails_a_ctx_whose_result_depends_on_the_split():
    rng = np.random.default_rng(1)
    ref = cg.reference_run(KW, K, full, make=Ctx)
    assert np.abs(ref[0]["weights"]).max() > 0 and np.abs(ref[0]["hidden"]).max() > 0 and 0 < ref[0]["episode_steps"].max() < 5
    between = []
    got, calls = cg.split_run(KW, rng, K, [10, 1, 19], full, between=between.append, make=Ctx)
    assert cg.differs(got, ref) == [] and calls == [10, 1, 19] and len(between) == 2                              # (not after the last call)
    got, _ = cg.split_run(KW, rng, K, iter([10, 20]), full, between=between.append, after_last=True, make=Ctx)
    assert cg.differs(got, ref) == [] and len(between) == 4
    bad = flawed("split")
    assert cg.differs(cg.split_run(KW, rng, K, [10, 1, 19], full, make=bad)[0], cg.reference_run(KW, K, full, make=bad)) == ["weights"]
    assert cg.differs((ref[0], (1, 2)), ref) == "checksum" and cg.differs((ref[0], (1, 2)), ref, checksum=False) == []


def test_the_trait_part_runs_the_loop_it_is_given_from_the_start_it_is_given():
    def start(c, off):
        c.reset()
        c.W[:, 1, 1] = np.float32(0.25)
    ref = cg.reference_run(KW, K, full, start, make=Ctx)
    assert cg.differs(cg.trait_run(KW, K, 5, trait_loop, full, start, make=Ctx), ref) == []
    assert cg.differs(cg.trait_run(KW, K, 5, trait_loop, full, make=Ctx), ref) == ["weights"]                     # (the default start is reset alone)
    assert "weights" in cg.differs(cg.trait_run(KW, K, 5, lambda c, k, cap: trait_loop(c, k - 1, cap), full, start, make=Ctx), ref)


def test_the_shard_part_fails_a_ctx_that_ignores_env_offset():
    ref = cg.reference_run(KW, K, full, make=Ctx)
    offs = []

    def start(c, off):
        offs.append((off, c.N))
        c.reset()
    assert diff(join_shards(*cg.shard_run(KW, K, (4, 4), full, start, make=Ctx)), ref[0]) == []
    assert diff(join_shards(*cg.shard_run(KW, K, (3, 5), full, start, make=Ctx)), ref[0]) == [] and offs == [(0, 4), (4, 4), (0, 3), (3, 5)]
    bad = flawed("offset")
    names = diff(join_shards(*cg.shard_run(KW, K, (4, 4), full, make=bad)), cg.reference_run(KW, K, full, make=bad)[0])
    assert "weights" in names and "states" in names


def test_the_checkpoint_part_fails_when_what_the_file_does_not_hold_is_not_carried():
    ref = cg.reference_run(KW, K, full, make=Ctx)
    for overwrite in (True, False):
        assert cg.differs(cg.resume_run(KW, K, 12, full, carry=carry, overwrite=overwrite, make=Ctx), ref) == []
    assert cg.differs(cg.resume_run(KW, K, 12, full, make=Ctx), ref) == ["weights", "hidden"]
    assert cg.twin_resume(KW, 12, 9, full, carry=carry, make=Ctx) == []
    bad = cg.twin_resume(KW, 12, 9, full, make=Ctx)
    assert bad == ["the loaded ctx differs after train(12)", "9 steps after the load: ['weights', 'hidden']"]


def test_the_environment_side_fails_an_agent_that_sees_other_draws_than_td():
    kw = dict(KW, algo=ra.SARSA)
    assert cg.env_side(kw, dict(kw, algo=ra.TD), K, make=Ctx) == []
    bad = cg.env_side(kw, dict(kw, algo=ra.TD), K, make=flawed("env"))
    assert "states after train(30) != RSRL_TD's" in bad and any(b.startswith("sum_episode_steps") or b.startswith("episodes") for b in bad)
