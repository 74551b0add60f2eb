"""The oracle's own 32-bit edges (CPU only): Run.t installs a batch-step counter -- what a loaded checkpoint does on the device -- and every loop
then draws at orc.draw(seed, id, T0 + k, block); the draws depend on the counter's HIGH word (the whole t past 2^32, the per-step streams' t >> 1 past
2^33) and on every bit of the 32-bit learner id.  tests/test_gpu_counter_edges.py compares the device with these loops at such counters and ids: it
could not fail on a device that truncates if the reference truncated too."""
import numpy as np
import pytest

EDGES = [2 ** 32 - 5, 2 ** 32 - 4, 2 ** 33 - 5, 2 ** 33 - 4]
OFFSETS = [0, 2 ** 31 - 65, 2 ** 32 - 1 - 130]


def test_draws_depend_on_the_counters_high_word(orc):
    for seed, gid in ((1, 0), (77, 2 ** 31 + 3)):
        for k in range(8):
            for blk in (orc.BLK_INIT, orc.BLK_API, 16, 16 + 64 * 2 + 63):           # whole-t blocks: word 1 of the Philox counter is t >> 32
                assert list(orc.draw(seed, gid, k, blk)) != list(orc.draw(seed, gid, 2 ** 32 + k, blk))
            for blk in (orc.BLK_STEP, orc.BLK_RESET, orc.BLK_INNER):                # per-step streams: addressed by t >> 1
                a, b = orc.draw(seed, gid, 2 * k, blk), orc.draw(seed, gid, 2 ** 33 + 2 * k, blk)
                assert list(a[:2]) != list(b[:2])                                   # (the words in use: explore?, pick)
                assert a[0] != b[0] and a[1] != b[1]
                a, b = orc.draw(seed, gid, 2 * k + 1, blk), orc.draw(seed, gid, 2 ** 33 + 2 * k + 1, blk)
                assert a[0] != b[0] and a[1] != b[1]
                # 2^32 is bit 31 of t >> 1: the low counter word, also part of the address
                assert list(orc.draw(seed, gid, k, blk)[:2]) != list(orc.draw(seed, gid, 2 ** 32 + k, blk)[:2])


def test_draws_depend_on_every_bit_of_the_learner_id(orc):
    for t in (0, 5, 2 ** 32 + 1):
        for blk in (orc.BLK_STEP, orc.BLK_INNER, orc.BLK_INIT, 16):
            for gid in (0, 64, 2 ** 31 - 1):
                assert list(orc.draw(3, gid, t, blk)) != list(orc.draw(3, gid + 2 ** 31, t, blk))       # the sign bit
            assert list(orc.draw(3, 2 ** 32 - 2, t, blk)) != list(orc.draw(3, 2 ** 31 - 2, t, blk))
            assert list(orc.draw(3, 2 ** 32 + 7, t, blk)) == list(orc.draw(3, 7, t, blk))               # truncated to 32 bits, as the device's gid


@pytest.mark.parametrize("prec", ["f64", "f32", "f32d"])
@pytest.mark.parametrize("T0", EDGES)
def test_a_run_set_to_t0_draws_at_t0_plus_k(orc, prec, T0):
    # Random policy: the action IS the draw (pick = mulhi(word 1, A)); max_episode_steps = 1: every batch-step ends the episode, so each one
    # samples from the RESET alias of the step stream at the counter's value
    N, seed, off = 9, 11, 1000
    ag = orc.make_agent(policy=orc.RANDOM, seed=seed, env_offset=off, max_episode_steps=1)
    run = orc.Run(ag, N, prec)
    assert run.t == 0
    run.t = T0
    assert run.t == T0
    run.reset()
    assert run.t == T0                                                              # reset keeps the counter and draws the first action at it
    q0 = np.zeros(3, dtype=np.float32)
    want = [orc.policy_sample(orc.RANDOM, q0, orc.draw(seed, off + i, T0, orc.BLK_INIT), prec="f32") for i in range(N)]
    assert list(run.action) == want
    for k in range(10):                                                             # crosses the edge at k = 4 or 5
        run.train(1)
        assert run.t == T0 + k + 1
        want = [orc.policy_sample(orc.RANDOM, q0, orc.draw(seed, off + i, T0 + k, orc.BLK_RESET), prec="f32") for i in range(N)]
        assert list(run.action) == want, k


@pytest.mark.parametrize("method,kw", [("train", {}), ("train_dev", {}), ("train_fast", {}),
                                       ("train_wave", dict(domain=1, order=7, algo=2, policy=2)),
                                       ("train_shared_dev", dict(shared_w=True, lr=1e-4)),
                                       ("train_sparse_lambda", dict(basis=1, algo=3, lam=0.5, shared_w=True, alpha=1e-3))])
def test_every_loop_reads_the_installed_counter(orc, method, kw):
    # the same configuration from T0 and from T0 + 2^33 (same low words everywhere): a loop that dropped a high word would walk the same actions
    N, K, T0 = 48, 12, 2 ** 33 - 5
    kw = dict(dict(policy=orc.EGREEDY, epsilon=0.5, seed=5, max_episode_steps=4), **kw)
    acts = []
    for t0 in (T0, T0 + 2 ** 33, T0):
        run = orc.Run(orc.make_agent(**kw), N, "f32d")
        run.t = t0
        (run.reset_wave if method == "train_wave" else run.reset)()
        hist = [run.action.copy()]
        for k in (3, 1, K - 4):
            getattr(run, method)(k)
            hist.append(run.action.copy())
        assert run.t == t0 + K
        acts.append(np.concatenate(hist))
    assert np.array_equal(acts[0], acts[2])
    assert not np.array_equal(acts[0], acts[1])
    assert not np.array_equal(acts[0][:N], acts[1][:N])                             # already the first action (BLK_INIT takes the whole t)


@pytest.mark.parametrize("off", OFFSETS[1:])
def test_a_slice_at_the_top_of_the_id_space_is_the_slice_of_its_draws(orc, off):
    N, seed = 130, 4
    run = orc.Run(orc.make_agent(policy=orc.RANDOM, seed=seed, env_offset=off, max_episode_steps=1), N, "f32d")
    run.reset()
    run.train_dev(3)
    q0 = np.zeros(3, dtype=np.float32)
    want = [orc.policy_sample(orc.RANDOM, q0, orc.draw(seed, off + i, 2, orc.BLK_RESET), prec="f32") for i in range(N)]
    assert list(run.action) == want
    masked = [orc.policy_sample(orc.RANDOM, q0, orc.draw(seed, (off + i) & 0x7fffffff, 2, orc.BLK_RESET), prec="f32") for i in range(N)]
    assert masked != want                                                           # ids with bit 31 set are not their 31-bit images
