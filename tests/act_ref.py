"""The numpy fp64 reference of device policy inference (trpo_ctx_act; tests/test_gpu_act.py compares the
device with it).

Written from the definitions in include/trpo_mi355x.h: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel
random numbers: as easy as 1, 2, 3", SC'11) in integer arithmetic -- bit-exact --, the two 53-bit uniforms of
a block, the Box-Muller pair, the action and the Gaussian log-density.  The mean is synth.policy_mean in act(),
a long-double forward pass in act_ld() (tests/test_gpu_act_edges.py: saturating policies, the activations).
"""
import numpy as np

from trpo_amd import synth

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (broadcast together) of 32-bit words -> output words [..., 4] (uint64
    arrays holding 32-bit values)."""
    c = np.asarray(counter, np.uint64)
    k = np.asarray(key, np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        p0, p1 = M0 * c0, M1 * c2                      # 32 x 32 -> 64 bits: exact in uint64
        kr0 = (k0 + np.uint64((W0 * r) & 0xFFFFFFFF)) & _LO
        kr1 = (k1 + np.uint64((W1 * r) & 0xFFFFFFFF)) & _LO
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ kr0, p1 & _LO, (p0 >> _S32) ^ c3 ^ kr1, p0 & _LO
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def uniforms(o):
    """(u1 in (0, 1], u2 in [0, 1)) from output words [..., 4]: 53 bits each, exact."""
    o = np.asarray(o, np.uint64)
    a = (o[..., 0] << np.uint64(21)) | (o[..., 1] >> np.uint64(11))
    b = (o[..., 2] << np.uint64(21)) | (o[..., 3] >> np.uint64(11))
    return (a + np.uint64(1)).astype(np.float64) * 2.0 ** -53, b.astype(np.float64) * 2.0 ** -53


def normals(seed, step, rows, A):
    """z [len(rows)][A]: pair j = a // 2 of row r from the block with key (seed lo, seed hi) and counter
    (r lo, r hi, step lo, (step >> 32) << 16 | j)."""
    rows = np.asarray(rows, np.uint64).reshape(-1)
    npair = (A + 1) // 2
    j = np.arange(npair, dtype=np.uint64)
    ctr = np.empty((rows.size, npair, 4), np.uint64)
    ctr[..., 0] = (rows & _LO)[:, None]
    ctr[..., 1] = (rows >> _S32)[:, None]
    ctr[..., 2] = np.uint64(step & 0xFFFFFFFF)
    ctr[..., 3] = np.uint64((step >> 32) << 16) | j[None, :]
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    u1, u2 = uniforms(philox4x32_10(ctr, key))
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.empty((rows.size, 2 * npair))
    z[:, 0::2] = r * np.cos(2.0 * np.pi * u2)
    z[:, 1::2] = r * np.sin(2.0 * np.pi * u2)
    return z[:, :A]


def logp(z, logstd):
    """-1/2 sum z^2 - sum LogStd - (A/2) ln(2 pi), sums over a ascending."""
    z = np.asarray(z, np.float64)
    sz2, sls = np.zeros(z.shape[0]), 0.0
    for a in range(z.shape[1]):
        sz2 = sz2 + z[:, a] * z[:, a]
        sls = sls + logstd[a]
    return -0.5 * sz2 - sls - 0.5 * z.shape[1] * np.log(2.0 * np.pi)


def act(layers, acfunc, theta, obs, seed, step=0, row0=0, row_stride=1):
    """(mean, action, logp, z) of trpo_ctx_act for obs [m][L0], sample i being row row0 + i * row_stride."""
    obs = np.asarray(obs, np.float64).reshape(-1, layers[0])
    A = layers[-1]
    mean = synth.policy_mean(list(layers), acfunc, theta, obs)
    z = normals(seed, step, row0 + row_stride * np.arange(obs.shape[0]), A)
    logstd = np.asarray(theta, np.float64)[-A:]
    return mean, mean + np.exp(logstd) * z, logp(z, logstd), z


# ---------------------------------------------------------------------------
# The long-double reference (tests/test_gpu_act_edges.py): synth.policy_mean's continued-fraction tanh is good
# for |x| < 4 only, so saturating policies and the activation sweep take numpy's extended-precision functions.
# ---------------------------------------------------------------------------
LD = np.longdouble


def tanh_ld(x):
    return np.tanh(np.asarray(x, np.float64).astype(LD))


def logistic_ld(x):
    with np.errstate(over="ignore"):
        return LD(1) / (LD(1) + np.exp(-np.asarray(x, np.float64).astype(LD)))


def forward_ld(layers, acfunc, theta, obs):
    """The policy mean [m][A] in np.longdouble: y @ W + B, np.tanh, 1 / (1 + exp(-x)), 0.1 x."""
    th = np.asarray(theta, np.float64).astype(LD)
    y = np.asarray(obs, np.float64).reshape(-1, layers[0]).astype(LD)
    pos = 0
    for i in range(len(layers) - 1):
        fin, out = layers[i], layers[i + 1]
        x = y @ th[pos:pos + fin * out].reshape(fin, out) + th[pos + fin * out:pos + fin * out + out]
        pos += fin * out + out
        a = acfunc[i + 1]
        if a == "t":
            y = np.tanh(x)
        elif a == "s":
            with np.errstate(over="ignore"):
                y = LD(1) / (LD(1) + np.exp(-x))
        elif a == "o":
            y = LD(1) / LD(10) * x
        else:
            y = x
    return y


def act_ld(layers, acfunc, theta, obs, seed, step=0, row0=0, row_stride=1, samples=None):
    """act() with the mean from forward_ld (rounded to float64 once).  samples: the sample indices i the rows
    of obs belong to (default 0 .. m-1), so a test can take the reference on a few rows of a large batch."""
    obs = np.asarray(obs, np.float64).reshape(-1, layers[0])
    A = layers[-1]
    i = np.arange(obs.shape[0]) if samples is None else np.asarray(samples)
    mean = forward_ld(layers, acfunc, theta, obs).astype(np.float64)
    z = normals(seed, step, row0 + row_stride * i, A)
    logstd = np.asarray(theta, np.float64)[-A:]
    return mean, mean + np.exp(logstd) * z, logp(z, logstd), z


# tanh64 (csrc/trpo_common.h) and act_y64's logistic (csrc/trpo_update.hip) as numpy float64 expressions,
# products and sums rounded one by one (no fma): what the formulas cost against long double on the host
_TANH64_Q = (6.76744223569079683e-05, -2.34387837673838705e-04, 5.93821938760988777e-04, -1.45812091104440249e-03,
             3.59269513652666532e-03, -8.86331213798425936e-03, 2.18694943489975979e-02, -5.39682542017260666e-02,
             1.33333333337541271e-01, -3.33333333333355408e-01)


def tanh64_np(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        a, u = np.abs(x), x * x
        q = np.full_like(x, _TANH64_Q[0])
        for c in _TANH64_Q[1:]:
            q = q * u + c
        small = (a * u) * q + a
        big = np.where(a > 22.0, 1.0, 1.0 - 2.0 / (np.exp(2.0 * a) + 1.0))
    return np.copysign(np.where(a < 0.55, small, big), x)


def logistic_np(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))
