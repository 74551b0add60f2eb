"""What every random campaign (tests/fuzz_*.py) does the same way, once -- beside tests/agent_contract.py: "the same bits" is its `diff`, and
what a campaign passes in as `full` and as the trait loop are its snapshot / join_shards / trait_loop or the module's own.  Plain functions, no
fixtures, no pytest settings.  A campaign module keeps its sampler, its host-input builders, its references, bounds and own legs, its case
line and the ORDER of its legs; from here it takes

    the runner            run(run_case, ...): the case loop, ERROR lines, counts / per_agent / failures, the SUMMARY {json} line, exit code 1
    the read-only loop    read_only_calls(c, rng, calls): 1-4 of the module's named calls, the checksum equal around each, REFUSALS
    the self leg's parts  reference_run, split_run, trait_run, shard_run, resume_run (and twin_resume): each runs fresh ctxs and returns what
                          `full` shows (with the checksum); the module compares with `differs` and words its own finding
    the environment side  env_side: states, actions, episode steps and the integer statistics against an RSRL_TD ctx
    run_slice             a campaign's suite slice as a subprocess -> its parsed SUMMARY, for the GPU tests

The draw-order rule: a campaign's generator is consumed in exactly the order it was when its seeds were committed (tests/golden/
campaign_cases.json pins the keyed campaigns' samplers and host inputs).  A function here that draws says so in its docstring, draws the same
numbers at the same point as the copies it replaced, and takes the distribution as an argument where they differed; everything else is drawn by
the module and passed in."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import rsrl_amd as ra
from tests.agent_contract import diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSALS = (-1, -5)      # EINVAL, ESTATE: what a read-only call may refuse with
TOP_OF_IDS = -1          # an env_offset choice: resolved to 2^32 - 1 - n_envs once n_envs is known


# ---- small shared pieces
def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def top_of_ids(kw):
    """kw with TOP_OF_IDS resolved: the shard that ends at the largest learner id a ctx admits"""
    if kw["env_offset"] == TOP_OF_IDS:
        kw["env_offset"] = (1 << 32) - 1 - kw["n_envs"]
    return kw


def case_rng(seed, idx, key):
    """case idx's generator, keyed by the seed, the case and its agent: an agent's slice is not another's with the algo swapped"""
    return np.random.default_rng([seed, idx, key])


def parse_agents(argv, names):
    """the agents= argument: numbers or names, comma separated -> tuple of algo numbers, None when absent"""
    for a in argv:
        if a.startswith("agents="):
            by_name = {v: k for k, v in names.items()}
            return tuple(int(x) if x.lstrip("-").isdigit() else by_name[x] for x in a[7:].split(",") if x)
    return None


def parse_cases(argv, n_cases=200):
    """the positional [n_cases] [seed] -> (n_cases, seed)"""
    pos = [a for a in argv if "=" not in a]
    return int(pos[0]) if len(pos) > 0 else n_cases, int(pos[1]) if len(pos) > 1 else 0


def count(legs, name):
    legs[name] = legs.get(name, 0) + 1


# ---- the runner
def run(run_case, n_cases, seed, names=None, extras=None, finish=None):
    """The body of a campaign's main().  run_case(idx) -> (status, line, kw[, failure record]); an exception is the status ERROR.  MISMATCH and
    ERROR are failures.  names: algo -> agent name for per_agent (None: the summary has none); extras(failures) -> the summary's further
    keys, in their order, before `failures` unless it places that itself; finish(failures) may append an end-of-run failure.  Exits 1 on any"""
    counts, per_agent, failures = {}, {}, []
    for idx in range(n_cases):
        try:
            status, line, kw, *record = run_case(idx)
        except Exception as e:      # noqa: BLE001
            status, line, kw, record = "ERROR", f"{idx:4d} ERROR {type(e).__name__}: {str(e)[:200]}", None, []
        counts[status] = counts.get(status, 0) + 1
        if names is not None and kw is not None:
            count(per_agent.setdefault(names[kw["algo"]], {}), status)
        print(line, flush=True)
        if status in ("MISMATCH", "ERROR"):
            failures.append(record[0] if record else {"case": idx, "line": line, "config": kw})
    if finish is not None:
        finish(failures)
    summary = {"cases": n_cases, "seed": seed, "counts": counts}
    if names is not None:
        summary["per_agent"] = per_agent
    summary.update(extras(failures) if extras is not None else {})
    summary.setdefault("failures", failures)
    print("SUMMARY " + json.dumps(summary, default=str), flush=True)
    sys.exit(1 if failures else 0)


def verdict(tag, kw, bad, why=None):
    """a case's (status, line, kw) from its findings and the reason it diverged, if it did"""
    if bad:
        return "MISMATCH", tag + f"  MISMATCH {bad[:4]}", kw
    if why is not None:
        return "diverged", tag + f"  diverged: {why}", kw
    return "ok", tag + "  ok", kw


def create(tag, kw):
    """-> (the ctx, None), or (None, the refused case's (status, line, kw))"""
    try:
        return ra.Context(**kw), None
    except ra.RsrlHipError as e:
        return None, ("refused", tag + f"  REFUSED: {str(e)[:90]}", kw)


# ---- read-only calls
def read_only_calls(c, rng, calls):
    """Draws a permutation of the names of `calls` (name -> callable, built by the module after its own draws) and how many of them, 1-4, to
    make.  None may change anything: the checksum before and after each is equal, and a call may refuse only with one of REFUSALS
    -> (findings, the calls made)"""
    names, bad, made = list(calls), [], []
    for j in rng.permutation(len(names))[: int(rng.integers(1, 5))]:
        name = names[int(j)]
        made.append(name)
        ck = c.checksum()
        try:
            calls[name]()
        except ra.RsrlHipError as e:
            if e.code not in REFUSALS:
                bad.append(f"{name}: {str(e)[:80]}")
        if c.checksum() != ck:
            bad.append(f"{name} moved the checksum")
    return bad, made


# ---- the parts of the self leg.  full(c): what is compared; start(c, off): how a fresh ctx is prepared, off its env_offset within the unsharded run
def reset(c, off):
    c.reset()


def differs(got, ref, checksum=True):
    """got, ref: (what `full` showed, the checksum) of two runs -> the names that differ, "checksum" where only that does, else nothing"""
    return diff(got[0], ref[0]) or ("checksum" if checksum and got[1] != ref[1] else [])


def draw_calls(rng, K, lo, hi):
    """Draws lo..hi-1 cut points in [1, K) (the number first) -> the lengths of the train calls between them, summing to K"""
    cuts = sorted(set(int(x) for x in rng.integers(1, K, size=int(rng.integers(lo, hi)))))
    return [b - a for a, b in zip([0] + cuts, cuts + [K])]


def reference_run(kw, K, full, start=reset, want_stats=False, make=ra.Context):
    """one uninterrupted train(K)"""
    with make(**kw) as c:
        start(c, 0)
        c.train(K, want_stats=want_stats)
        return full(c), c.checksum()


def split_run(kw, rng, K, calls, full, start=reset, between=None, after_last=False, make=ra.Context):
    """train(k) for k in `calls` (a list, or an iterator that draws each k when asked), drawing want_stats for each call after its k;
    between(c) runs after every call but the last (after_last: after that one too) and may draw -> ((full, checksum), the calls made)"""
    done = []
    with make(**kw) as c:
        start(c, 0)
        for k in calls:
            c.train(k, want_stats=bool(rng.integers(0, 2)))
            done.append(k)
            if between is not None and (after_last or sum(done) < K):
                between(c)
        return (full(c), c.checksum()), done


def trait_run(kw, K, cap, loop, full, start=reset, make=ra.Context):
    """K steps through the trait calls on the host: loop(c, K, cap)"""
    with make(**kw) as c:
        start(c, 0)
        loop(c, K, cap)
        return full(c), c.checksum()


def shard_run(kw, K, sizes, full, start=reset, want_stats=False, make=ra.Context):
    """train(K) on consecutive env_offset shards of the given sizes -> [full(shard)], for tests/agent_contract.join_shards"""
    parts, off = [], 0
    for n in sizes:
        with make(**dict(kw, n_envs=n, env_offset=kw["env_offset"] + off)) as c:
            start(c, off)
            c.train(K, want_stats=want_stats)
            parts.append(full(c))
        off += n
    return parts


def _save_and_load(a, b, k1, td, start, carry, want_stats, overwrite):
    start(a, 0)
    a.train(k1, want_stats=want_stats)
    path = os.path.join(td, "w.ckpt")
    a.save_weights(path)
    if overwrite:
        b.reset()
        b.train(2, want_stats=False)
    b.load_weights(path)
    b.states, b.actions, b.episode_steps = a.states, a.actions, a.episode_steps
    if carry is not None:
        carry(a, b)


def resume_run(kw, K, k1, full, start=reset, carry=None, overwrite=True, want_stats=False, make=ra.Context):
    """save after train(k1), load into a second ctx (overwrite: one that has trained two steps of its own), carry the env side over and, by
    carry(a, b), whatever else the file does not hold, train(K - k1) there -> (full, checksum) for the comparison with reference_run's"""
    with make(**kw) as a, make(**kw) as b, tempfile.TemporaryDirectory() as td:
        _save_and_load(a, b, k1, td, start, carry, want_stats, overwrite)
        b.train(K - k1, want_stats=want_stats)
        return full(b), b.checksum()


def twin_resume(kw, k1, k2, full, start=reset, carry=None, make=ra.Context):
    """save after train(k1), load into a fresh ctx: the same step count, `full` and checksum there and after train(k2) on both -> findings"""
    bad = []
    with make(**kw) as a, make(**kw) as b, tempfile.TemporaryDirectory() as td:
        _save_and_load(a, b, k1, td, start, carry, False, False)
        if b.step_count != a.step_count or diff(full(b), full(a)) or a.checksum() != b.checksum():
            bad.append(f"the loaded ctx differs after train({k1})")
        a.train(k2, want_stats=False)
        b.train(k2, want_stats=False)
        names = diff(full(b), full(a))
        if names or a.checksum() != b.checksum():
            bad.append(f"{k2} steps after the load: {names or 'checksum'}")
    return bad


# ---- the environment side
def env_side(kw, td_kw, K, make=ra.Context):
    """train(K) on kw beside the RSRL_TD ctx td_kw (the same seed, N, cap and domain: both sample Random on the same draws): states, actions,
    episode steps and the integer statistics identical -> findings"""
    bad = []
    with make(**kw) as c, make(**td_kw) as t:
        c.reset()
        t.reset()
        sc, stt = c.train(K), t.train(K)
        for name in ("states", "actions", "episode_steps"):
            if not np.array_equal(getattr(c, name).view(np.uint32), getattr(t, name).view(np.uint32)):
                bad.append(f"{name} after train({K}) != RSRL_TD's")
        for name in ("env_steps", "episodes", "episodes_truncated", "sum_episode_steps"):
            if sc[name] != stt[name]:
                bad.append(f"{name}: {sc[name]} != RSRL_TD's {stt[name]}")
    return bad


# ---- for the GPU tests
def run_slice(script, cases, seed, agents=None):
    """tests/<script> [cases] [seed] [agents=...] as a subprocess -> its parsed SUMMARY, with the process's exit code as "exit_code" """
    argv = [sys.executable, os.path.join(ROOT, "tests", script), str(cases), str(seed)] + (["agents=" + agents] if agents else [])
    p = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith("SUMMARY ")]
    assert line, ("no SUMMARY line", p.stdout[-2000:], p.stderr[-2000:])
    return dict(json.loads(line[0][8:]), exit_code=p.returncode)
