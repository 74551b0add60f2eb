"""What the 32-bit-edge test modules share (tests/test_gpu_counter_edges.py, tests/test_gpu_large_footprint.py): the constants of their case tables,
the checkpoint trick that installs a batch-step counter, and the mapping of Context arguments to the oracle's."""
import os
import struct

import rsrl_amd as ra

MC, CP, AB = ra.MOUNTAIN_CAR, ra.CART_POLE, ra.ACROBOT      # (CartPole pays 0 until it falls: inside a 5-step cap its weights never move)
E32, E33 = 1 << 32, 1 << 33
T_ALL = [E32 - 5, E32 - 4, E33 - 5, E33 - 4]
T_TWO = [E32 - 5, E33 - 4]
OFFSETS = [(1 << 31) - 65, (1 << 32) - 1 - 130]
EG = dict(policy=ra.EPSILON_GREEDY, epsilon=0.3)
SM = dict(policy=ra.SOFTMAX, tau=1.0)
TILE = dict(basis=ra.TILE_CODING, n_tilings=8, tiles_per_dim=6)
SHARED = dict(weight_mode=ra.W_SHARED)
BF16 = dict(weight_dtype=ra.W_BF16)
LAM = (ra.SARSA_LAMBDA, ra.Q_LAMBDA, ra.TD_LAMBDA)


def feats(kw):
    dim = {MC: 2, CP: 4, AB: 4}[kw.get("domain", MC)]
    return kw["n_tilings"] if kw.get("basis") == ra.TILE_CODING else (kw.get("order", 5) + 1) ** dim


def install_counter(c, t0, tmp_path):
    """a fresh ctx's own checkpoint with the header's step_count rewritten -> c.step_count == t0, first action drawn at t0"""
    a, b = os.path.join(str(tmp_path), "fresh.ckpt"), os.path.join(str(tmp_path), "at_t0.ckpt")
    c.save_weights(a)
    raw = bytearray(open(a, "rb").read())
    assert struct.unpack_from("<Q", raw, 64)[0] == 0
    struct.pack_into("<Q", raw, 64, t0)
    with open(b, "wb") as f:
        f.write(raw)
    c.load_weights(b)
    c.reset()
    assert c.step_count == t0


def oracle_kwargs(orc, kw):
    o = {k: v for k, v in kw.items() if k not in ("n_envs", "steps_per_launch", "weight_mode", "weight_dtype", "basis")}
    o["basis"] = orc.TILE if kw.get("basis") == ra.TILE_CODING else orc.FOURIER
    o["shared_w"] = kw.get("weight_mode") == ra.W_SHARED
    return o
