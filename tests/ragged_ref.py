"""The numpy reference of the ragged advantage stage (tests/test_advantage_ragged_abi.py pins its baseline
forward to the CPU oracle; tests/test_gpu_advantage_ragged.py compares the device with it).

Written from the definitions: per episode e of len steps, with Vb = the baseline at [boot_observ[e],
len / horizon] where the episode is truncated and 0 otherwise,
    ret[t] = sum_k gamma^k reward[t+k] + gamma^(len-t) Vb
    d[t]   = reward[t] + gamma V[t+1] - V[t],  V[len] = Vb
    A[t]   = sum_k (gamma lam)^k d[t+k]
as direct sums (np.power), a two-pass mean and variance over all samples, and the episodes' raw reward sums.
"""
import functools

import numpy as np

from trpo_amd import synth

BASE = (16, 16, 16, 1)
AC = "lttl"
COEFFS = [(0.995, 0.98), (1.0, 1.0), (0.0, 0.5), (0.9, 0.0)]     # tests/test_gpu_advantage.py's

# where the 64-step chunked walk can go wrong; the last has more episodes than the scan's 1024 x 4 waves
LENGTHS = {
    "1-2": (1, 2),
    "63-64-65": (63, 64, 65),
    "1-128-129-200-7": (1, 128, 129, 200, 7),
    "20x150": (150,) * 20,
    "1x5-64": (1,) * 5 + (64,),
    "4100x1-2-3": tuple(1 + e % 3 for e in range(4100)),
}
BOOTS = ("none", "all", "alternate")


def boot_flags(mode, num_ep):
    """None (no truncation) or the uint8 flags of one of BOOTS; "last": the last episode alone
    (tests/test_gpu_update_scratch.py)."""
    if mode == "none":
        return None
    if mode == "all":
        return np.ones(num_ep, np.uint8)
    if mode == "last":
        return (np.arange(num_ep) == num_ep - 1).astype(np.uint8)
    return (np.arange(num_ep) % 2 == 0).astype(np.uint8)


def forward(layers, ac, x, rows):
    """The baseline's prediction for input rows [m][layers[0]]: weights W[in][out] then biases B per
    layer in x, 't' tanh / 'l' linear (ac[0] belongs to the input layer)."""
    y, at = np.asarray(rows, np.float64), 0
    for i in range(len(layers) - 1):
        a, b = layers[i], layers[i + 1]
        W = x[at:at + a * b].reshape(a, b)
        B = x[at + a * b:at + a * b + b]
        at += a * b + b
        z = y @ W + B
        y = np.tanh(z) if ac[i + 1] == "t" else z
    return y[:, 0]


def time_feature(lens, horizon):
    return np.concatenate([np.arange(L, dtype=np.float64) for L in lens]) / float(horizon)


@functools.lru_cache(maxsize=None)
def inputs(lens, layers=BASE, seed=7):
    """x, observ [n][O], reward [n] drawn as tests/test_gpu_advantage.py::inputs draws them, then the
    observations after each episode's last step, boot_observ [num_ep][O]."""
    rng = np.random.default_rng(seed)
    n, O = int(sum(lens)), layers[0] - 1
    npar = synth.num_params(list(layers)) - layers[-1]
    reward = -np.abs(rng.normal(1.0, 0.7, n))
    observ = rng.normal(0.0, 1.0, (n, O))
    x = 0.3 * rng.normal(0.0, 1.0, npar)
    boot_observ = rng.normal(0.0, 1.0, (len(lens), O))
    for a in (reward, observ, x, boot_observ):
        a.setflags(write=False)
    return x, observ, reward, boot_observ


@functools.lru_cache(maxsize=None)
def values(lens, horizon, layers=BASE, ac=AC, seed=7):
    """V [n] and the bootstrap value of every episode [num_ep] (whether truncated or not)."""
    x, observ, _, boot_observ = inputs(lens, layers, seed)
    V = forward(layers, ac, x, np.column_stack([observ, time_feature(lens, horizon)]))
    Vb = forward(layers, ac, x, np.column_stack([boot_observ, np.asarray(lens, np.float64) / float(horizon)]))
    V.setflags(write=False)
    Vb.setflags(write=False)
    return V, Vb


def discounted(x, c):
    """y[e, t] = sum_k c^k x[e, t + k], as direct sums."""
    T = x.shape[1]
    k = np.arange(T)[None, :] - np.arange(T)[:, None]            # [t, j] -> j - t
    M = np.where(k >= 0, np.power(float(c), np.maximum(k, 0)), 0.0)
    return (x[:, None, :] * M[None, :, :]).sum(axis=2)


@functools.lru_cache(maxsize=None)
def reference(lens, horizon, mode, gamma, lam, layers=BASE, ac=AC, seed=7):
    x, observ, reward, _ = inputs(lens, layers, seed)
    V, Vb_all = values(lens, horizon, layers, ac, seed)
    lens_a = np.asarray(lens)
    num_ep, n = lens_a.size, int(lens_a.sum())
    flags = boot_flags(mode, num_ep)
    Vb = Vb_all * flags if flags is not None else np.zeros(num_ep)
    off = np.concatenate([[0], np.cumsum(lens_a)[:-1]])
    ret, A, R = np.zeros(n), np.zeros(n), np.zeros(num_ep)
    for L in sorted(set(lens)):                                  # the episodes of one length at a time
        eps = np.flatnonzero(lens_a == L)
        idx = off[eps][:, None] + np.arange(L)[None, :]
        r, v, vb = reward[idx], V[idx], Vb[eps]
        vn = np.concatenate([v[:, 1:], vb[:, None]], axis=1)
        delta = r + gamma * vn - v
        tail = np.power(float(gamma), L - np.arange(L))[None, :] * vb[:, None]     # gamma^(len - t) Vb
        ret[idx] = discounted(r, gamma) + tail
        A[idx] = discounted(delta, gamma * lam)
        R[eps] = r.sum(axis=1)
    am = A.sum() / n
    asd = np.sqrt(((A - am) ** 2).sum() / n)
    rm = R.sum() / num_ep
    rsd = np.sqrt(((R - rm) ** 2).sum() / num_ep)
    out = dict(ret=ret, adv=(A - am) / asd, A=A, V=V, Vb=Vb, off=off, ep_rew_mean=rm, ep_rew_std=rsd, adv_mean=am,
               adv_std=asd, conditioning=asd / np.abs(A).max())
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# every parity case: (length set, horizon or None = the longest episode, truncation mode); with the default
# horizon a truncated longest episode has the bootstrap time feature exactly 1.0
PARITY_CASES = [(name, None, mode) for name in LENGTHS for mode in BOOTS] + [("63-64-65", 100, "alternate"),
                                                                              ("1-128-129-200-7", 1000, "all")]


def horizon_of(name, horizon):
    return max(LENGTHS[name]) if horizon is None else horizon
