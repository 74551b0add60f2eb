"""Writes tests/golden/philox_extremes.json: (seed, learner id) pairs whose Philox block at t = 0, block word BLK_API + 256 -- the block the first
policy_sample(states) of a Gaussian ctx draws -- sits on an edge of gauss_normal that random draws do not meet:

  u1_min      (x >> 8) <= 3:            u1 = 2^-24 .. 2^-22, Box-Muller's radius at its maximum (|z| up to 5.77)
  u1_one      (x >> 8) = 2^24 - 1:      u1 = 1, the radius is sqrt(-0)
  u2_zero     (y >> 8) = 0:             the angle is 0
  u2_quarter  |u2 - 1/4| <= 2^-20:      the cosine passes through zero, sincos_cw changes quadrant
  u2_three_quarters  |u2 - 3/4| <= 2^-20

A CPU search with tests/beta_numpy.philox_block over ids 0 .. 2^24 - 1, seed after seed from 1, until every class has at least two hits (or ten
minutes have passed); at most PER_CLASS hits of a class are kept, the first found -- of u1_min the ones with the smallest x >> 8, and the search goes
on until two of them have x >> 8 = 0 (u1 = 2^-24 itself, where |z| can reach 5.77).  Run from the repository root:
    python tests/golden/make_philox_extremes.py
tests/test_continuous_edges_cpu.py re-derives every listed block."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import beta_numpy as bn  # noqa: E402

PER_CLASS, NEED, CHUNK, IDS, BUDGET = 4, 2, 1 << 20, 1 << 24, 600.0
CLASSES = ("u1_min", "u1_one", "u2_zero", "u2_quarter", "u2_three_quarters")


def classify(w):
    """w uint32 (n, 4) -> {class: mask}"""
    x, y = (w[:, 0] >> 8).astype(np.int64), (w[:, 1] >> 8).astype(np.int64)
    return {"u1_min": x <= 3, "u1_one": x == (1 << 24) - 1, "u2_zero": y == 0, "u2_quarter": np.abs(y - (1 << 22)) <= 16,
            "u2_three_quarters": np.abs(y - 3 * (1 << 22)) <= 16}


def main():
    hits = {k: [] for k in CLASSES}
    start, seed = time.time(), 0

    def done():
        return all(len(v) >= NEED for v in hits.values()) and sum(h["words"][0] >> 8 == 0 for h in hits["u1_min"]) >= NEED

    while not done() and time.time() - start < BUDGET:
        seed += 1
        for lo in range(0, IDS, CHUNK):
            ids = np.arange(lo, lo + CHUNK)
            w = bn.philox_block(seed, ids, 0, bn.BLK_API + 256)
            for k, m in classify(w).items():
                for i in np.flatnonzero(m):
                    if len(hits[k]) < PER_CLASS or k == "u1_min":
                        hits[k].append({"seed": seed, "id": int(ids[i]), "words": [int(v) for v in w[i]], "class": k})
        hits["u1_min"] = sorted(hits["u1_min"], key=lambda h: h["words"][0] >> 8)[:PER_CLASS]       # (stable: the first found among equals)
        print("seed %d: %s (%.0f s)" % (seed, {k: len(v) for k, v in hits.items()}, time.time() - start), flush=True)
    out = {"t": 0, "block_word": bn.BLK_API + 256, "ids_searched": IDS, "seeds_searched": seed, "hits": [h for k in CLASSES for h in hits[k]]}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "philox_extremes.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
