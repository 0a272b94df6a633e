"""Problems of the wide-policy tests (tests/test_gpu_wide.py) and their CPU references, computed once per
process.  Seeded, so a failure names a reproducible configuration; tools/diag/wide_ritz.py probes the same
table for stalled reference solves."""
import functools

import numpy as np

import oracle
from trpo_amd import synth

# the kernels' own constants (csrc/dev_wide.h): WIDE_TS, the sample rows of one block of the layer kernels,
# and WIDE_SPLIT, the samples one block of the contraction sums
WIDE_TS = 64
WIDE_SPLIT = 512

HUMANOID = ([376, 128, 64, 17], "lttl")

# name -> (layers, activations, n, seed).  Small shapes where the 16-wide tiling can go wrong, sample counts
# that are no multiple of 16; the policy past the default solver's 32 768 parameters.
CASES = {
    "one-tile": ([15, 16, 16, 3], "lttl", 333, 1),          # every width one tile or less
    "past-tile": ([17, 33, 65, 5], "ltsl", 1001, 1),        # every width one past a tile edge
    "thin": ([3, 130, 20, 1], "ltll", 47, 2),               # one output, L0 < 4, n below any sample tile
    "depth3": ([8, 24, 6], "ltl", 200, 4),
    "depth5": ([6, 20, 12, 9, 2], "ltstl", 150, 29),
    "humanoid": (HUMANOID[0], HUMANOID[1], 257, 6),         # P = 57 634
}
EDGE_SHAPE = ([17, 33, 65, 5], "ltsl", 7)                   # layers, activations, seed of the sample-split edges
# synth.make_obs draws observations in (-0.17, 0.19): the hidden activations then hardly differ between
# samples, F is 0.1 I plus about 2 A large eigenvalues, and a 10-iteration solve of a policy with few outputs
# converges to rounding -- a stalled reference solve at every seed (tools/diag/wide_ritz.py).  Scaled to
# about (-2, 2.3) the spectrum spreads and the seeds below keep every solve's Ritz residual >= 1e-13.
OBS_SCALE = 12.0
EDGE_N = sorted({1} | {t + d for t in (WIDE_TS, WIDE_SPLIT) for d in (-1, 0, 1)})


def make(layers, acts, n, seed):
    """theta with non-zero biases and LogStd, sigma != 1, a direction, a right-hand side and a rollout."""
    rng = np.random.default_rng(seed)
    A = layers[-1]
    th = synth.make_theta(layers, seed=100 + seed)
    pos = 0
    for i in range(len(layers) - 1):
        pos += layers[i] * layers[i + 1]
        th[pos:pos + layers[i + 1]] = rng.normal(0.0, 0.3, layers[i + 1])
        pos += layers[i + 1]
    th[pos:] = rng.uniform(-0.5, 0.3, A)
    obs = OBS_SCALE * synth.make_obs(n, layers[0], seed=200 + seed)
    std = rng.uniform(0.5, 1.6, size=A)
    P = synth.num_params(layers)
    mean, action, adv = synth.make_rollout(layers, acts, th, obs, std, seed=500 + seed)
    return dict(layers=layers, acts=acts, n=n, theta=th, obs=obs, std=std, P=P, v=synth.make_v(P, seed=300 + seed),
                b=synth.make_b(P, seed=400 + seed), mean=mean, action=action, adv=adv)


@functools.lru_cache(maxsize=None)
def case(name):
    layers, acts, n, seed = CASES[name]
    return make(layers, acts, n, seed)


@functools.lru_cache(maxsize=None)
def reference(name):
    """oracle FVP, 10-iteration CG (threshold 0), policy gradient and full update of a case"""
    p = case(name)
    a = (p["layers"], p["acts"], p["theta"], p["obs"])
    z, _ = oracle.fvp(*a, p["std"], p["v"])
    cg = oracle.cg(*a, p["std"], p["b"], 10, 0.0)
    pg, _ = oracle.policy_grad(*a, p["mean"], p["action"], p["adv"])
    upd = oracle.update(*a, p["mean"], p["action"], p["adv"], p["std"], 0.1)
    iters = oracle.cg(*a, p["std"], pg, 10, 1e-10)["iters"]       # the update's own solve, threshold 1e-10
    return dict(z=z, x=cg["x"], pg=pg, update=upd, update_iters=iters)


def _plain_cg(F, b, maxiter, resth):
    """the reference's recurrence (src/TRPO_CG.c) in fp64: its alpha_k and beta_k (tools/diag/ritz_probe.py)"""
    x, r, p = np.zeros_like(b), b.copy(), b.copy()
    rr = r @ r
    al, be = [], []
    for _ in range(maxiter):
        if rr < resth:
            break
        z = F(p)
        a = rr / (p @ z)
        x += a * p
        r = r - a * z
        nr = r @ r
        al.append(a)
        be.append(nr / rr)
        p = r + nr / rr * p
        rr = nr
    return np.array(al), np.array(be)


def ritz_min(al, be):
    """smallest relative Ritz residual over the Lanczos matrices T_1 .. T_k of a solve's coefficients"""
    best = np.inf
    for k in range(1, len(al) + 1):
        T = np.zeros((k, k))
        for j in range(k):
            T[j, j] = 1.0 / al[j] + (be[j - 1] / al[j - 1] if j > 0 else 0.0)
            if j + 1 < k:
                T[j, j + 1] = T[j + 1, j] = np.sqrt(be[j]) / al[j]
        w, S = np.linalg.eigh(T)
        res = np.sqrt(be[k - 1]) / al[k - 1] * np.abs(S[-1, :]) / np.max(np.abs(w))
        best = min(best, float(res.min()))
    return best


def ritz_of(p, b, maxiter, resth):
    F = lambda q: oracle.fvp(p["layers"], p["acts"], p["theta"], p["obs"], p["std"], q, 0.1)[0]  # noqa: E731
    return ritz_min(*_plain_cg(F, b, maxiter, resth))
