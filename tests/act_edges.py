"""The inputs of tests/test_gpu_act_edges.py, built once and read-only, and checked on the CPU by
tests/test_act_inputs.py: the activation sweep, the saturating policies, the batches whose grids wrap, the wide
layers and the networks at the neuron form's LDS limit.

The launch geometry the cases are sized by (csrc/trpo_update.hip): both kernel forms launch at most GRID = 1024
blocks; the neuron form puts 4 rows into a block, so it wraps beyond 4096 rows, the lane form 64, so it wraps
beyond 65 536.  A batch whose m L0 + m (2A + 1) doubles (m L0 + m A without samples) fit PIN = 2^18 goes through
the pinned buffer, a larger one is staged.  The neuron form needs 4 (sum of the layer sizes + A + (A & 1)) doubles
of LDS and is refused beyond 64 KiB.
"""
import functools

import numpy as np

import trained as T
from trpo_amd import synth

GRID, NEURON_ROWS, LANE_ROWS = 1024, 4, 64
PIN = 1 << 18
NEURON_LDS = 64 * 1024
NEAR = 70                                 # rows compared with the reference at each end and around each wrap


def pinned(layers, m, sample=True):
    A = layers[-1]
    return m * layers[0] + m * (2 * A + 1 if sample else A) <= PIN


def neuron_lds_bytes(layers):
    A = layers[-1]
    return 8 * NEURON_ROWS * (sum(layers) + A + (A & 1))


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


# --- 1. the activations themselves ---------------------------------------------------------------------------
ACT_LAYERS = [1, 1, 1]


def activation_theta():
    """Both weights 1, LogStd 0 and both biases -0.0: x * 1 + (-0.0) is x for every x, the zeros with their
    signs included (a bias of +0.0 would turn -0.0 into +0.0 before the activation sees it)."""
    return np.array([1.0, -0.0, 1.0, -0.0, 0.0])


@functools.lru_cache(maxsize=None)
def sweep_points():
    """70 031 arguments: every positive one with its negative, then NaN."""
    rng = np.random.default_rng(20261020)
    edges = [np.nextafter(0.55, 0.0), 0.55, np.nextafter(0.55, 1.0), np.nextafter(22.0, 0.0), 22.0,
             np.nextafter(22.0, 23.0), 0.0, 5e-324, 60.0, 700.0, 1e300, np.inf]
    pos = np.concatenate([np.linspace(0.0, 0.55, 16001)[1:], np.linspace(0.55, 25.0, 15001)[1:],
                          10.0 ** rng.uniform(-300.0, -1.0, 4003), edges])
    x = np.concatenate([pos, -pos, [np.nan]])
    x.setflags(write=False)
    return x


# --- 2. saturating, biased policies ---------------------------------------------------------------------------
SAT_SHAPES = [([15, 16, 16, 3], "lttl"), ([20, 13, 16, 5], "lsol"), ([15, 64, 64, 6], "lttl"),
              ([4, 54, 26, 17, 5], "ltsll"), ([12, 32, 1], "ltl"), ([20, 80, 80, 3], "lttl")]
SAT_M = 130


def shape_id(shape):
    return "%s-%s" % ("x".join(map(str, shape[0])), shape[1])


@functools.lru_cache(maxsize=None)
def trained_problem(layers, ac, setting, m, seed=0):
    """theta and obs [m][L0] of tests/trained.py under one of its settings (layers as a tuple)."""
    oscale, gain, bamp = T.SETTINGS[setting]
    L = list(layers)
    return _freeze(dict(layers=L, ac=ac, theta=T.theta(L, gain, bamp, seed), obs=T.obs(m, L[0], oscale, seed)))


def saturating(k, setting):
    layers, ac = SAT_SHAPES[k]
    return trained_problem(tuple(layers), ac, setting, SAT_M)


# --- 3. grids that wrap ---------------------------------------------------------------------------------------
WRAP_SHAPE = ([15, 16, 16, 3], "lttl")
WRAP_SWITCH = 11915                       # the last pinned batch size of WRAP_SHAPE with samples
WRAP_MAX = 65606                          # the lane form's second trip: 70 rows
STRIDED = dict(row0=3, row_stride=7, m=4101)
HANDOFF_NS = [4101, 8197]                 # keep_all's two calls: 2050 + 2051 rows, and 4098 + 4099 (both wrap)


def wrap_problem(m):
    """The first m rows of one batch (setting A), so every size shares its rows with the others."""
    p = trained_problem(tuple(WRAP_SHAPE[0]), WRAP_SHAPE[1], "A", WRAP_MAX)
    return dict(p, obs=p["obs"][:m])


def near_rows(m, period):
    """The first and last NEAR samples and NEAR around each multiple of period below m, ascending."""
    idx = set(range(min(NEAR, m))) | set(range(max(0, m - NEAR), m))
    for c in range(period, m, period):
        idx |= set(range(max(0, c - NEAR // 2), min(m, c + NEAR // 2)))
    return np.array(sorted(idx))


# --- 4. wide layers and many actions ---------------------------------------------------------------------------
# [376,128,64,17] is the reference project's Humanoid policy: 57 634 parameters, beyond the device CG's 32 768, so
# its context serves inference only; [180,128,64,17] has the same hidden layers and the most inputs the solver
# still takes (32 546).  131 actions are 66 pairs: the neuron form's pair loop takes a second trip as well, and
# pair 65 writes the padding slot.
WIDE_SHAPES = [([376, 128, 64, 17], "lttl"), ([10, 80, 130, 67], "ltsl"), ([180, 128, 64, 17], "lttl"),
               ([6, 20, 131], "ltl")]
WIDE_MS = [1, 5, 130]


def wide(k):
    layers, ac = WIDE_SHAPES[k]
    return trained_problem(tuple(layers), ac, "A", max(WIDE_MS))


# --- 5. the neuron form's LDS limit ----------------------------------------------------------------------------
LDS_SHAPES = {"fits": ([2030, 8, 2], "ltl"), "over": ([2040, 8, 2], "ltl")}
LDS_M = 100                               # 100 x 2045 doubles: still a pinned batch


@functools.lru_cache(maxsize=None)
def lds_problem(which):
    """Weights at synth.make_theta's own scale (gain 1, N(0, 1 / fan-in)), biases within 0.5, obs as
    synth.make_obs draws them: 2000 inputs keep the pre-activations of order one."""
    layers, ac = LDS_SHAPES[which]
    return _freeze(dict(layers=layers, ac=ac, theta=T.theta(layers, 1.0, 0.5, 0),
                        obs=synth.make_obs(LDS_M, layers[0], seed=0)))


def reference_cases():
    """(id, problem, the sample indices the GPU test compares) of every case that is held to the long-double
    reference: what tests/test_act_inputs.py checks the oracle's forward pass on."""
    out = []
    for k, shape in enumerate(SAT_SHAPES):
        for s in "ABS":
            out.append(("sat-%s-%s" % (shape_id(shape), s), saturating(k, s), np.arange(SAT_M)))
    out.append(("wrap-neuron-4101", wrap_problem(4101), near_rows(4101, GRID * NEURON_ROWS)))
    out.append(("wrap-pinned-11915", wrap_problem(WRAP_SWITCH), near_rows(WRAP_SWITCH, GRID * NEURON_ROWS)))
    out.append(("wrap-staged-11916", wrap_problem(WRAP_SWITCH + 1), near_rows(WRAP_SWITCH + 1, GRID * NEURON_ROWS)))
    out.append(("wrap-lane-65606", wrap_problem(65606), near_rows(65606, GRID * LANE_ROWS)))
    s = STRIDED
    out.append(("wrap-strided-4101", wrap_problem(65606),
                s["row0"] + s["row_stride"] * near_rows(s["m"], GRID * NEURON_ROWS)))
    for k, shape in enumerate(WIDE_SHAPES):
        out.append(("wide-%s" % shape_id(shape), wide(k), np.arange(max(WIDE_MS))))
    for which in LDS_SHAPES:
        out.append(("lds-%s" % which, lds_problem(which), np.arange(LDS_M)))
    return out
