"""numpy reference of the observation filter (include/trpo_mi355x.h, "The observation filter"),
written from the definitions: Welford (1962) for what the moments are, Chan, Golub and LeVeque (1983) for how two
sets of them merge.

normalise() uses exactly the operations the contract lists -- numpy's fp64 subtract, multiply, maximum and minimum
are the same IEEE operations, so the GPU tests compare bit for bit.  The statistics are chained the way the
contract chains them (one batch per record call, merged by the formula) but in np.longdouble and with two-pass
batch moments, so they stand for the exact values; tests/test_obsnorm_abi.py checks them against one direct
two-pass computation over all rows.
"""
import functools

import numpy as np

LD = np.longdouble


def derived(count, mean, m2, eps):
    """(shift, scale) of live statistics, fp64"""
    mean, m2 = np.asarray(mean, np.float64), np.asarray(m2, np.float64)
    if count < 2:
        return np.zeros_like(mean), np.ones_like(mean)
    return mean.copy(), 1.0 / (np.sqrt(m2 / (count - 1.0)) + eps)


def normalise(x, shift, scale, clip):
    """the contract's operations in the contract's order, fp64; x [m][L0] (fp32 input is widened exactly first)"""
    y = (np.asarray(x).astype(np.float64) - shift) * scale
    return np.minimum(np.maximum(y, -clip), clip)


def batch_moments(x):
    """(m, mean_b, M2_b) of the rows x [m][L0], two passes, long double"""
    x = np.asarray(x).astype(LD)
    mean = x.sum(axis=0) / LD(x.shape[0])
    return x.shape[0], mean, ((x - mean) ** 2).sum(axis=0)


def merge(p, b):
    """(n_p, mean_p, M2_p) merged with the batch (m, mean_b, M2_b) by the contract's formula, long double"""
    (n_p, mean_p, m2_p), (m, mean_b, m2_b) = p, b
    if m == 0:
        return p
    n = n_p + m
    d = mean_b - mean_p
    return n, mean_p + d * (LD(m) / LD(n)), m2_p + m2_b + d * d * (LD(n_p) * LD(m) / LD(n))


def empty(L0):
    return 0, np.zeros(L0, LD), np.zeros(L0, LD)


class Filter:
    """the state machine of the contract: record() adds a call's raw rows to pending, fold() merges pending into
    live, begin() empties pending"""

    def __init__(self, L0):
        self.L0 = L0
        self.live, self.pending = empty(L0), empty(L0)

    def record(self, x):
        self.pending = merge(self.pending, batch_moments(np.asarray(x).reshape(-1, self.L0)))

    def fold(self):
        self.live = merge(self.live, self.pending)
        self.pending = empty(self.L0)

    def begin(self):
        self.pending = empty(self.L0)


def direct(x):
    """(n, mean, M2) of all rows at once, two passes, long double"""
    return batch_moments(x)


def one_pass_m2(x):
    """sum x^2 - (sum x)^2 / n in fp64: what the two passes are there to avoid"""
    x = np.asarray(x, np.float64)
    return (x * x).sum(axis=0) - x.sum(axis=0) ** 2 / x.shape[0]


def assert_one_pass_loses(x, at_least=1e-6):
    """the one-pass sum of squares is off by at_least, relative, in some column of x (rows of ill_conditioned()
    with 70 columns: offset / spread reaches 1e5, and eps * 1e10 is 1e-6): the failure the statistics' 1e-12
    bound exists to catch must be there to be caught"""
    loss = rel_err(one_pass_m2(x), direct(x)[2])
    assert loss >= at_least, loss
    return loss


def rel_err(got, want):
    """per element, relative to the reference's own magnitude"""
    got, want = np.asarray(got).astype(LD), np.asarray(want).astype(LD)
    return float(np.max(np.abs(got - want) / np.abs(want)))


@functools.lru_cache(maxsize=None)
def ill_conditioned(m, L0, seed=0):
    """rows whose column k has offset 10^(k mod 4) and spread 10^(-2 + k mod 5): read-only"""
    k = np.arange(L0)
    x = 10.0 ** (k % 4) + 10.0 ** (-2 + k % 5) * np.random.default_rng(1000 + seed).normal(size=(m, L0))
    x.setflags(write=False)
    return x


def device_order_moments(x, chunk):
    """(mean_b, M2_b) of one call in fp64 in the documented order: compensated chunk sums in row order from 0,
    the chunk sums compensated in chunk order from 0 (the device feeds the square into its step's fma unrounded;
    here it is rounded first)"""
    x = np.asarray(x).astype(np.float64)
    m = x.shape[0]

    def step(s, e, v):
        y = v - e
        t = s + y
        return t, (t - s) - y

    def two_level(v):
        tot, te = np.zeros(v.shape[1]), np.zeros(v.shape[1])
        for r0 in range(0, m, chunk):
            s, e = np.zeros(v.shape[1]), np.zeros(v.shape[1])
            for row in v[r0:r0 + chunk]:
                s, e = step(s, e, row)
            tot, te = step(tot, te, s)
        return tot
    mean = two_level(x) / m
    d = x - mean
    return mean, two_level(d * d)


def merge64(p, b):
    """merge() as the device runs it: every operation in fp64, rounded on its own"""
    (n_p, mean_p, m2_p), (m, mean_b, m2_b) = p, b
    if m == 0:
        return p
    n = float(n_p + m)
    d = mean_b - mean_p
    return n_p + m, mean_p + d * (m / n), m2_p + m2_b + d * d * (n_p * m / n)
