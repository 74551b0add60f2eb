#!/usr/bin/env python3
"""Which configurations rsrl_hip_create admits, asked of the library on a machine WITHOUT a GPU: every admission rule runs before the device
query, so a refused configuration returns EINVAL and an admitted one EHIP ("no device").  Sweeps GRID (133 120 configurations, about 1 s) and
GRID_AGENTS -- the algos numbered after GRID's (13-19) on the same other axes, 71 680 configurations -- and GRID_AGENTS2 (20 and 21, 20 480
configurations) and GRID_AGENTS3 (22 and 23, with max_episode_steps = 200 on every configuration: GradientMC refuses the default 0), each into a
fixture of its own; and GRID_BETA, the continuous axis: MountainCar and ContinuousMountainCar x the policies Softmax, Random, Beta x the algos iLSTD
(19), the iLSTD ActorCritic (21) and the unassigned 27, with agent_policy -1 / Softmax / Beta (15 360 configurations) -> create_admission_beta.json
(tests/test_tdac_beta_cpu.py); and GRID_NAC: ContinuousMountainCar / MountainCar x Softmax / Random / Beta x the algos 21, the unassigned 27 and NAC
(28) x agent_policy -1 / Beta x the Fourier orders 0-6 x n_steps (NAC's period) 0, 1, 100, 65 536, 65 537 (1 260 configurations) ->
create_admission_nac.json (tests/test_nac_beta_cpu.py); and GRID_GTD: GRID's axes with the algos 29 (unassigned), GTD2 (30), TDC (31) and 32 (past
the last) and an lr_td axis 0 / -1 (81 920 configurations) -> create_admission_gtd.json (tests/test_gtd_cpu.py); and GRID_GAUSS: the policies Beta (4),
the unassigned 5, Gaussian (6) and 7 (past the last) x the iLSTD ActorCritic (21) and NAC (28) x MountainCar / ContinuousMountainCar x agent_policy
-1 / Gaussian x the Fourier orders 0-6 x GRID_NAC's n_steps (1 120 configurations) -> create_admission_gauss.json (tests/test_nac_gaussian_cpu.py); and
GRID_CACLA: NAC (28), the unassigned 32, CACLA (33) and 34 (past the last) x the policies Random, Beta, Gaussian x MountainCar / ContinuousMountainCar x
agent_policy -1 / Gaussian x the Fourier orders 0-6 (336 configurations) -> create_admission_cacla.json (tests/test_cacla_cpu.py); and
GRID_TDAC_CONT: CACLA (33), the unassigned 34, the continuous TD ActorCritic (35) and 36 (past the last) x the policies Softmax, Random, Beta, Gaussian x
MountainCar / ContinuousMountainCar x agent_policy -1 / Gaussian x the Fourier orders 0-6 (448 configurations) -> create_admission_tdac_cont.json
(tests/test_tdac_cont_cpu.py); and GRID_LSPE: LambdaLSPE (39) between the unassigned 38 and 40 (past the last) on GRID's other axes, with
max_episode_steps = 200 on every configuration as GRID_AGENTS3 (30 720 configurations) -> create_admission_lspe.json (tests/test_lspe_cpu.py).
    python scripts/admission_matrix.py            writes tests/golden/create_admission.json, create_admission_agents.json,
                                                  create_admission_agents2.json and create_admission_agents3.json
                                                  (tests/test_create_admission_cpu.py, tests/test_tdac_lstd_cpu.py and tests/test_gmc_cpu.py
                                                  hold the library to them)
    python scripts/admission_matrix.py --check    exits 1 if the library and a stored fixture disagree
Each admitted configuration is stored as one character per axis: the index of its value in that axis, in hex."""
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "create_admission.json")
AGENTS_FIXTURE = os.path.join(ROOT, "tests", "golden", "create_admission_agents.json")
AGENTS2_FIXTURE = os.path.join(ROOT, "tests", "golden", "create_admission_agents2.json")
AGENTS3_FIXTURE = os.path.join(ROOT, "tests", "golden", "create_admission_agents3.json")
BETA_FIXTURE = os.path.join(ROOT, "tests", "golden", "create_admission_beta.json")
NAC_FIXTURE = os.path.join(ROOT, "tests", "golden", "create_admission_nac.json")
GTD_FIXTURE = os.path.join(ROOT, "tests", "golden", "create_admission_gtd.json")
GAUSS_FIXTURE = os.path.join(ROOT, "tests", "golden", "create_admission_gauss.json")
CACLA_FIXTURE = os.path.join(ROOT, "tests", "golden", "create_admission_cacla.json")
TDAC_CONT_FIXTURE = os.path.join(ROOT, "tests", "golden", "create_admission_tdac_cont.json")
LSPE_FIXTURE = os.path.join(ROOT, "tests", "golden", "create_admission_lspe.json")
EINVAL, EHIP = -1, -2

# (config field, values): the first axis varies slowest
GRID = [
    ("domain", [0, 1, 2, 3]),
    ("basis", [0, 1]),                       # Fourier, tile coding
    ("order", [1, 2, 3, 5, 7]),
    ("n_tilings", [4, 8]),
    ("algo", list(range(13))),               # 12: no such algo
    ("policy", [0, 1, 2, 3]),
    ("weight_mode", [0, 1]),
    ("weight_dtype", [0, 1]),
    ("agent_policy", [-1, 2]),               # none, Softmax
    ("epsilon_decay", [1.0, 0.99]),
    ("steps_per_launch", [0, 1]),
]
# the TD ActorCritic (13), REINFORCE / BaselineREINFORCE (15, 16), RecursiveLSTD / iLSTD (18, 19) and the unassigned 14 and 17, on GRID's other axes
GRID_AGENTS = [(name, list(range(13, 20)) if name == "algo" else vals) for name, vals in GRID]
# the unassigned 20 and the iLSTD ActorCritic (21), on GRID's other axes
GRID_AGENTS2 = [(name, [20, 21] if name == "algo" else vals) for name, vals in GRID]
# the unassigned 22 and GradientMC (23), on GRID's other axes; FIXED_AGENTS3 is set on every configuration of the grid
GRID_AGENTS3 = [(name, [22, 23] if name == "algo" else vals) for name, vals in GRID]
FIXED_AGENTS3 = {"max_episode_steps": 200}
# the continuous axis: ContinuousMountainCar (4) beside MountainCar, the Beta policy (4) beside Softmax and Random, as behaviour and as agent policy
GRID_BETA = [
    ("domain", [0, 4]),
    ("basis", [0, 1]),
    ("order", [1, 2, 3, 4, 5, 6, 7]),
    ("algo", [19, 21, 27]),                  # 27: no such algo
    ("policy", [2, 3, 4]),
    ("weight_mode", [0, 1]),
    ("weight_dtype", [0, 1]),
    ("agent_policy", [-1, 2, 4]),
    ("epsilon_decay", [1.0, 0.99]),
    ("steps_per_launch", [0, 1]),
    ("n_steps", [2, 33]),
]
# NAC (28) beside the iLSTD ActorCritic and the unassigned 27: its one domain and policy beside the others, its period's range and both ends' neighbours
GRID_NAC = [
    ("domain", [4, 0]),
    ("policy", [2, 3, 4]),
    ("algo", [21, 27, 28]),                  # 27: no such algo
    ("agent_policy", [-1, 4]),
    ("order", [0, 1, 2, 3, 4, 5, 6]),
    ("n_steps", [0, 1, 100, 65536, 65537]),
]
# GTD2 (30) and TDC (31) between the unassigned 29 and 32, on GRID's other axes, with the second column's rate: 0 and a negative one
GRID_GTD = [(name, [29, 30, 31, 32] if name == "algo" else vals) for name, vals in GRID] + [("lr_td", [0.0, -1.0])]
# the Gaussian policy (6) between Beta, the unassigned 5 and 7: under NAC, its one agent, and under the iLSTD ActorCritic, which has Beta only
GRID_GAUSS = [
    ("policy", [4, 5, 6, 7]),                # 5, 7: no such policy
    ("algo", [21, 28]),
    ("domain", [0, 4]),
    ("agent_policy", [-1, 6]),
    ("order", [0, 1, 2, 3, 4, 5, 6]),
    ("n_steps", [0, 1, 100, 65536, 65537]),
]
# CACLA (33) between the unassigned 32 and 34, next to NAC: under the Gaussian policy, its one policy, and under Beta and Random, which it refuses
GRID_CACLA = [
    ("algo", [28, 32, 33, 34]),              # 32, 34: no such algo
    ("policy", [3, 4, 6]),
    ("domain", [0, 4]),
    ("agent_policy", [-1, 6]),
    ("order", [0, 1, 2, 3, 4, 5, 6]),
]
# the continuous TD ActorCritic (35) between the unassigned 34 and 36, next to CACLA: under Beta and Gaussian, its two policies, and under Softmax and
# Random, which it refuses
GRID_TDAC_CONT = [
    ("algo", [33, 34, 35, 36]),              # 34, 36: no such algo
    ("policy", [2, 3, 4, 6]),
    ("domain", [0, 4]),
    ("agent_policy", [-1, 6]),
    ("order", [0, 1, 2, 3, 4, 5, 6]),
]
# LambdaLSPE (39) between the unassigned 38 and 40, on GRID's other axes; FIXED_AGENTS3 on every configuration (the agent records its open episodes)
GRID_LSPE = [(name, [38, 39, 40] if name == "algo" else vals) for name, vals in GRID]
# (grid, fixture, fields set on every configuration)
GRIDS = ((GRID, FIXTURE, {}), (GRID_AGENTS, AGENTS_FIXTURE, {}), (GRID_AGENTS2, AGENTS2_FIXTURE, {}), (GRID_AGENTS3, AGENTS3_FIXTURE, FIXED_AGENTS3),
         (GRID_BETA, BETA_FIXTURE, {}), (GRID_NAC, NAC_FIXTURE, {}), (GRID_GTD, GTD_FIXTURE, {}),
         (GRID_GAUSS, GAUSS_FIXTURE, {}), (GRID_CACLA, CACLA_FIXTURE, {}), (GRID_TDAC_CONT, TDAC_CONT_FIXTURE, {}))
# the grids added since (tests/test_tdac_cont_cpu.py holds GRIDS to its ten entries): swept and checked with them
GRIDS_SINCE = ((GRID_LSPE, LSPE_FIXTURE, FIXED_AGENTS3),)


def sweep(grid=GRID, fixed=None):
    """{index string: (return code, last error)} for every configuration of the grid, the fields of `fixed` set on each."""
    from rsrl_amd import _abi
    L = _abi.lib()
    base = _abi.Config()
    assert L.rsrl_hip_config_init(C.byref(base)) == 0
    for name, val in (fixed or {}).items():
        setattr(base, name, val)
    out = {}
    h = C.c_void_p()
    for idx in itertools.product(*(range(len(v)) for _, v in grid)):
        cfg = _abi.Config.from_buffer_copy(base)
        for (name, vals), i in zip(grid, idx):
            setattr(cfg, name, vals[i])
        rc = L.rsrl_hip_create(C.byref(cfg), C.byref(h))
        out["".join("%x" % i for i in idx)] = (rc, (L.rsrl_hip_last_error() or b"").decode())
    return out


def admitted(results):
    return sorted(k for k, (rc, _) in results.items() if rc == EHIP)


def main():
    ok = True
    for grid, fixture, fixed in GRIDS + GRIDS_SINCE:
        res = sweep(grid, fixed)
        if any(rc == 0 for rc, _ in res.values()):
            sys.exit("a ctx was created: run this on a machine without a GPU")
        bad = sorted({rc for rc, _ in res.values()} - {EINVAL, EHIP})
        if bad:
            sys.exit(f"unexpected return codes {bad}")
        doc = {"grid": [[n, v] for n, v in grid], "admitted": admitted(res)}
        if fixed:
            doc["fixed"] = fixed
        if "--check" in sys.argv:
            same = json.load(open(fixture)) == doc
            print(f"{os.path.relpath(fixture, ROOT)}: " + ("fixture matches" if same else "fixture DIFFERS"))
            ok = ok and same
            continue
        with open(fixture, "w") as f:         # one admitted configuration per line, so that a diff reads
            f.write('{"grid": %s,\n' % json.dumps(doc["grid"]))
            if fixed:
                f.write(' "fixed": %s,\n' % json.dumps(fixed))
            f.write(' "admitted": [\n')
            f.write(",\n".join(json.dumps(k) for k in doc["admitted"]))
            f.write("\n]}\n")
        print(f"{len(doc['admitted'])} of {len(res)} configurations admitted -> {os.path.relpath(fixture, ROOT)}")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
