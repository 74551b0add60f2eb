"""What the keyed random campaigns draw on the slices the GPU suite runs, pinned: per case one sha256 over the sampled Context keywords and, where
a campaign builds host inputs without a device (tests/fuzz_episodic.batch_inputs, tests/fuzz_beta.f64_inputs), over every array and scalar of
them.  The suite's conditions on those slices -- at most 5 % of the replayed learner-rounds left out, at most 2 % of the LSTD cases diverged,
legs["shard"] >= 3 -- belong to the committed seeds and case counts; tests/test_campaign_cpu.py recomputes the digests, so an edit that moves a
draw (a reordered sampler, one more rng call before the inputs, a changed key of case_rng) fails there and not as a shifted share on the GPU.

    python tests/golden/make_campaign_cases.py [out.json]            (no GPU; rewrites tests/golden/campaign_cases.json)

Regenerating is legitimate when a sampler, a seed or a case count is MEANT to change, and only after tests/test_fuzz_late_cpu.py has re-checked
the shares of the new slice (and the GPU suite its legs).  A refactor of the campaigns never regenerates: the file is the record of what they drew
before it."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "campaign_cases.json")


def feed(h, x):
    """x into the hash h, by its structure: mappings in their own key order with the keys, sequences in order, arrays as dtype, shape and bytes,
    numbers by repr (a float's repr is exact)"""
    if isinstance(x, dict):
        h.update(b"{")
        for k, v in x.items():
            h.update(str(k).encode() + b":")
            feed(h, v)
        h.update(b"}")
    elif isinstance(x, (list, tuple)):
        h.update(b"[")
        for v in x:
            feed(h, v)
        h.update(b"]")
    elif isinstance(x, np.ndarray):
        h.update(("<%s%s>" % (x.dtype.str, x.shape)).encode() + np.ascontiguousarray(x).tobytes())
    elif isinstance(x, np.generic):
        h.update(("<%s>" % x.dtype.str).encode() + x.tobytes())
    elif x is None or isinstance(x, (bool, int, float, str)):
        h.update((type(x).__name__ + repr(x) + ";").encode())
    else:
        raise TypeError("no serialisation for %r" % type(x))


def digest(kw, io):
    h = hashlib.sha256()
    feed(h, dict(sorted(kw.items())))
    feed(h, io)
    return h.hexdigest()


def slices():
    """-> {name: (seed, cases, case(idx) -> (kw, host inputs or None))}: the command lines tests/test_gpu_fuzz.py, test_gpu_gtd.py, test_gpu_cacla.py
    and test_gpu_tdac_cont.py issue"""
    from tests import fuzz_beta as fb, fuzz_cacla as fc, fuzz_episodic as fe, fuzz_gtd as fg, fuzz_tdac_cont as ft

    def keyed(mod, seed, agents, inputs):
        def case(idx):
            rng = mod.case_rng(seed, idx, agents)
            kw = mod.sample(rng, idx, agents)
            return kw, (inputs(rng, kw) if inputs else None)
        return case

    def single(mod, seed):
        def case(idx):
            return mod.sample(mod.case_rng(seed, idx)), None
        return case

    out = {}
    for mod, inputs in ((fe, fe.batch_inputs), (fb, fb.f64_inputs)):               # (both run at fuzz_episodic's seed and count: _campaign_slice)
        for algo in mod.AGENTS:
            out["%s/%s" % (mod.__name__.split(".")[-1], mod.NAMES[algo])] = (fe.SUITE_SEED, fe.SUITE_CASES, keyed(mod, fe.SUITE_SEED, (algo,), inputs))
    out["fuzz_gtd/GTD2,TDC"] = (fg.SUITE_SEED, fg.SUITE_CASES, keyed(fg, fg.SUITE_SEED, fg.AGENTS, None))
    out["fuzz_cacla/CACLA"] = (fc.SUITE_SEED, fc.SUITE_CASES, single(fc, fc.SUITE_SEED))
    out["fuzz_tdac_cont/Gaussian,Beta"] = (ft.SUITE_SEED, ft.SUITE_CASES, single(ft, ft.SUITE_SEED))
    return out


def compute():
    return {name: {"seed": seed, "cases": n, "sha256": [digest(*case(idx)) for idx in range(n)]} for name, (seed, n, case) in slices().items()}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    got = compute()
    assert got == compute(), "the digests differ between two runs"
    with open(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print({name: (d["seed"], d["cases"]) for name, d in got.items()})
