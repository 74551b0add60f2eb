"""The timed regions the continuous agents' rate scripts share (cacla_rate.py, tdac_cont_rate.py, nac_gaussian_rate.py, nac_beta_rate.py): several
contexts in ONE process on one build, their regions alternating after a warm-up, so that a drift of the machine falls on all of them."""
import statistics

import numpy as np

import rsrl_amd


def region(c, steps):
    """us per batch-step of one timed train(steps) (device events around the launches: rsrl_hip_timing_read)"""
    c.sync()
    c.timing_enable(True)
    c.train(steps, want_stats=False)
    ms, launches, name = c.timing_read()
    return ms * 1e3 / steps, launches, name


def timed(ctxs, steps, regions, warmup):
    """reset and warm every context up, then `regions` rounds of one region each (steps: one count, or one per context)
    -> (us per batch-step of every region, per context; (launches per region, kernel name) per context)"""
    steps = steps if isinstance(steps, (list, tuple)) else [steps] * len(ctxs)
    for c in ctxs:
        c.reset()
        c.train(warmup, want_stats=False)
        c.sync()
    us, meta = [[] for _ in ctxs], [None] * len(ctxs)
    for _ in range(regions):
        for j, c in enumerate(ctxs):
            u, launches, name = region(c, steps[j])
            us[j].append(u)
            meta[j] = (launches, name)
    return us, meta


def alternate(agents, a, base=0):
    """agents: [(label, Context keywords)] -> one row per agent; vs_base: the median time relative to agent `base`'s.  The keyword v0 is not the
    Context's: V = v0 everywhere before the run (the constant feature is the last one)"""
    ctxs = [rsrl_amd.Context(**{k: v for k, v in kw.items() if k != "v0"}) for _, kw in agents]
    rows = []
    try:
        for c, (_, kw) in zip(ctxs, agents):
            if kw.get("v0"):
                w = np.zeros((c.F, 1), dtype=np.float32)
                w[c.F - 1] = kw["v0"]
                c.set_weights_all(w)
        us, meta = timed(ctxs, a.steps, a.regions, a.warmup)
        ref = statistics.median(us[base])
        for j, (label, kw) in enumerate(agents):
            med = statistics.median(us[j])
            first = range(min(256, a.size))
            dead = sum(not (np.isfinite(ctxs[j].get_weights(i)).all() and np.isfinite(ctxs[j].get_policy_weights(i)).all()) for i in first)
            cols = max(float(np.nanmax(np.abs(ctxs[j].get_policy_weights(i)))) for i in first)
            rows.append(dict(agent=label, kernel=meta[j][1], order=kw["order"], features=ctxs[j].F, n_envs=a.size, batch_steps_per_region=a.steps,
                             launches_per_region=meta[j][0], regions=a.regions, us_per_batch_step=round(med, 3),
                             us_per_batch_step_regions=[round(x, 3) for x in us[j]], env_steps_per_s=a.size / (med * 1e-6), vs_base=round(med / ref, 3),
                             batch_steps_run=int(ctxs[j].step_count), max_abs_policy_column_of_first_256=cols, non_finite_of_first_256=int(dead)))
    finally:
        for c in ctxs:
            c.close()
    return rows
