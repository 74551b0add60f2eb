"""A bounded slice of the differential campaign tests/fuzz_parity.py in the GPU suite: 250 random configurations of the whole supported space
(domain x basis x order x agent x policy x weight mode x dtype x fuse depth x episode cap x learner count x env offset, random train() splits), the HIP
path through the C ABI against the oracle's device-order instantiation, bit for bit.  (Round 5: 9 000 cases over eight seeds ran clean after the
campaign's two findings -- the oracle's f32 trace rate, and SARSALambda / QLambda missing on the generic Fourier orders -- were fixed.)"""
import os
import subprocess
import sys
import json

import pytest

from tests.campaign import run_slice

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_random_configurations_bitwise_against_the_oracle():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_parity.py"), "250", "20260929"], capture_output=True, text=True, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith("SUMMARY ")]
    assert line, (p.stdout[-2000:], p.stderr[-2000:])
    d = json.loads(line[0][8:])
    assert p.returncode == 0 and not d["failures"], d["failures"][:3]
    assert d["counts"].get("ok", 0) >= 240 and d["counts"].get("refused", 0) == 0, d["counts"]      # every sampled configuration exists


def test_adversarial_configurations_and_arguments_return_errors():
    # tests/fuzz_abi.py: out-of-range, non-finite and contradictory config fields; null pointers, learner indices and batch sizes out of range,
    # non-finite states, actions outside the action set -- every entry point returns, and a healthy ctx created afterwards trains to the same checksum.
    # (Round 5 findings: a ctx refused for its device ordinal left HIP's sticky last error behind for the next ctx's first launch check; an infinite or
    # huge Acrobot angle handed to set_states would have spun in the reference's wrap! loop on the device.)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_abi.py"), "400", "5"], capture_output=True, text=True, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith("SUMMARY ")]
    assert p.returncode == 0 and line, (p.stdout[-2000:], p.stderr[-2000:])
    d = json.loads(line[0][8:])
    assert not d["failures"] and d["created"] >= 80 and d["refused"] >= 150, d


def test_set_states_refuses_what_would_spin_in_wrap():
    import numpy as np
    import rsrl_amd as ra
    with ra.Context(domain=ra.ACROBOT, order=1, n_envs=8, policy=1) as c:
        c.reset()
        s = c.states
        for bad in (np.inf, -np.inf, np.nan, 1e30, -1e9):
            t = s.copy(); t[0, 3] = bad
            with pytest.raises(ra.RsrlHipError):
                c.states = t
        assert np.array_equal(c.states, s)                       # refused: untouched
        t = s.copy(); t[0, 3] = 100.0                             # far outside [-pi, pi], but a few wraps away: accepted as the reference would
        c.states = t
        c.train(3)
        assert np.all(np.abs(c.states[0]) <= np.float32(np.pi))


def test_random_configurations_against_the_f64_oracle_teacher_forced():
    # tests/fuzz_f64.py: the reference's precision.  Random configurations of every family and agent, the f64 run drives the trajectory, the device learns
    # from the identical transitions through Handler::handle.  Bounds asserted there: per-step TD error 2e-4 (relative to 1 + |td|), final weights 1e-4
    # (relative to max(1, |W|)), Q at the final states 2e-4; measured over 3 278 cases: 2.0e-4 / 1.4e-5 / 1.6e-4 worst (generic Fourier orders), shared
    # weights 1e-6.  Agents with a discrete decision inside handle (GreedyGQ's argmax, ...) may be tipped by a rounding: reported, not failed.
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_f64.py"), "300", "77"], capture_output=True, text=True, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith("SUMMARY ")]
    assert p.returncode == 0 and line, (p.stdout[-2000:], p.stderr[-2000:])
    d = json.loads(line[0][8:])
    assert not d["over"] and d["counts"].get("ok", 0) >= 220 and d["counts"].get("tipped", 0) <= 5, d["counts"]


def test_random_rank_groups_on_one_device():
    # tests/fuzz_ranks.py: G = 2 / 3 / 4 / 8 in-process ranks over one shared approximator (dense basis, tile coding, sparse-trace lambda agents),
    # random learner counts (ragged shards) and step splits: replicas identical, the group equal to the unsharded run (bit for bit where every shard is
    # whole blocks).  (Round 5 finding: eight ranks sharing the device and waiting on a 786 KB delta filled it with waiting blocks -- the exchange
    # kernels' grids are capped now where ranks share a device.)
    env = dict(os.environ, GPU_MAX_HW_QUEUES="32")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_ranks.py"), "40", "9"], capture_output=True, text=True, timeout=900, env=env)
    line = [l for l in p.stdout.splitlines() if l.startswith("SUMMARY ")]
    assert p.returncode == 0 and line, (p.stdout[-3000:], p.stderr[-2000:])
    d = json.loads(line[0][8:])
    assert not d["failures"] and d["counts"].get("ok", 0) >= 36, d["counts"]


def test_random_configurations_of_the_newer_agents():
    # tests/fuzz_agents.py: ActorCritic / QActorCritic, the TD ActorCritic, REINFORCE / BaselineREINFORCE, RecursiveLSTD / iLSTD on every register-family
    # order and the one-step agents on HIVTreatment, at random learner counts, offsets, caps and launch depths: handle on partial batches against the f64
    # rules (learners M..N-1 untouched), REINFORCE's ragged batches, and train against its splits (with queries between them), the trait loop, shards
    # and a checkpoint, bit for bit.
    d = run_slice("fuzz_agents.py", 200, 20261016)
    assert d["exit_code"] == 0 and not d["failures"], d["failures"][:3]
    assert d["counts"].get("refused", 0) == 0, d["counts"]
    per = d["per_agent"]
    for name in ("ActorCritic", "QActorCritic", "TDActorCritic", "REINFORCE", "BaselineREINFORCE", "RecursiveLSTD", "iLSTD"):
        assert per.get(name, {}).get("ok", 0) >= 20, (name, per)
    assert sum(v.get("ok", 0) for k, v in per.items() if k.startswith("HIV/")) >= 20, per


def _campaign_slice(script, agent):
    """one agent's slice of a campaign script as a subprocess -> its SUMMARY; asserts what every slice asserts: exit code 0, no failure, every
    sampled configuration created, at least 20 of the 24 cases ok for the agent, and at most 5 % of the replayed learner-rounds left out"""
    from tests.fuzz_episodic import SUITE_CASES, SUITE_SEED      # (24 cases on one seed: tests/test_fuzz_late_cpu.py checks the same slice's shares)
    d = run_slice(script, SUITE_CASES, SUITE_SEED, agent)
    print(agent, d["counts"], d.get("legs"), d.get("worst"))
    assert d["exit_code"] == 0 and not d["failures"], d["failures"][:3]
    assert d["counts"].get("refused", 0) == 0, d["counts"]
    assert d["per_agent"].get(agent, {}).get("ok", 0) >= 20, d["per_agent"]
    replayed = d.get("replayed", sum(w.get("replayed", 0) for w in d.get("worst", {}).values() if isinstance(w, dict)))
    assert d.get("left_out", 0) <= 0.05 * max(replayed, 1), (d.get("left_out"), replayed)
    return d


@pytest.mark.parametrize("agent", ["GradientMC", "LSTD", "LSTDLambda"])
def test_random_configurations_of_the_episode_record_agents(agent):
    # tests/fuzz_episodic.py: GradientMC, LSTD and LSTDLambda on every register-family order at random learner counts (idle and ragged lane groups),
    # env offsets up to the top of the id range, caps from 1 (every step ends an episode) to 200 (the record never closes) and launch depths:
    # handle_batch / handle_transitions on ragged batches against td_chain (bit for bit) and the f64 rules, lstd_solve against lu_solve bit for bit
    # with crafted matrices planted, train against its splits with read-only calls between them, the host trait loop, shards and a checkpoint with
    # the record carried -- bit for bit, the f64 state and the record included -- and the environment side against RSRL_TD's.
    d = _campaign_slice("fuzz_episodic.py", agent)
    assert d["counts"].get("diverged", 0) == 0, d["counts"]          # (at most 2 % of the LSTD cases: none of 24)
    assert d["legs"]["batch"] >= 20 and d["legs"]["trait"] >= 20 and d["legs"]["ckpt"] >= 20 and d["legs"]["env"] >= 20 and d["legs"].get("shard", 0) >= 3, d["legs"]


def test_random_configurations_of_the_ilstd_actor_critic():
    # tests/fuzz_tdac_lstd.py: the iLSTD ActorCritic (21) on the discrete domains -- handle against the f64 rule and an iLSTD ctx bit for bit,
    # train against its splits, the trait loop, shards and a checkpoint.
    _campaign_slice("fuzz_tdac_lstd.py", "iLSTDActorCritic")


@pytest.mark.parametrize("agent", ["BetaActorCritic", "NAC"])
def test_random_configurations_of_the_beta_policy_agents(agent):
    # tests/fuzz_beta.py: the Beta iLSTD ActorCritic and NAC on ContinuousMountainCar, orders 1-5, with policy columns in every branch of the device's
    # Softplus and actions on the clamp: handle on partial batches (the critic half bit for bit an iLSTD ctx's; the columns, w, delta and Q against the
    # f64 rules), nac_update bit for bit under a random mask and next to the norm's floor, the policy side against the f64 restatement, and train against
    # its splits with read-only calls between them, the host trait loop, shards and a checkpoint, bit for bit.  (Its finding: policy_mode of
    # parameters a few ulps above 1 -- tests/test_gpu_tdac_beta.py test_policy_mode_of_parameters_a_few_ulps_above_one.)
    d = _campaign_slice("fuzz_beta.py", agent)
    assert d["counts"].get("diverged", 0) == 0, d["counts"]
    assert d["legs"]["f64"] >= 20 and d["legs"]["trait"] >= 20 and d["legs"]["ckpt"] >= 20 and d["legs"].get("shard", 0) >= 2, d["legs"]
