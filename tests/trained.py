"""Biased, saturating policies for the kernel tests, and a plain numpy emulation of the FVP and of CG.

synth.make_theta has zero biases and a zero LogStd, and with synth.make_obs no hidden pre-activation passes
0.6, so neither the hardware-exponential branch of the tile kernels' tanh_fast (|x| >= 0.625) nor any bias
slot of the packed layouts sees a live value.  theta() / obs() scale the same seeded streams (exact
arithmetic: bit-identical on every host) into the range of a trained policy:

    setting   obs scale   weight gain   bias amplitude
    A         6           1.5           0.5               both tanh_fast branches populated
    B         10          2.5           1.0               mostly the exponential branch, max |x| 5 .. 15
    S         40          3.0           1.0               saturated: first hidden layer |x| >= 40

std is always exp(LogStd).  ROWS is the case table of tests/test_gpu_trained_policy.py, checked on the CPU by
tests/test_trained_inputs.py.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle
from trpo_amd import synth

N = 777                                   # 49 tiles of 16, the last one holding 9 live rows
SETTINGS = {"A": (6.0, 1.5, 0.5), "B": (10.0, 2.5, 1.0), "S": (40.0, 3.0, 1.0)}
BRANCH = 0.625                            # tanh_fast's switch between the polynomial and exp2 / rcp

NO_VALU_OFF = {"TRPO_NO_VALU_MIN_TILES": "1000000"}
NO_VALU_ON = {"TRPO_NO_VALU_MIN_TILES": "0"}
ONE_WAVE = {"TRPO_COOP": "0"}


def _row(family, layers, ac, env, has, lacks=(), ends=None, saturated=False):
    return dict(family=family, layers=layers, ac=ac, env=env, has=tuple(has), lacks=tuple(lacks), ends=ends,
                saturated=saturated)


# family, layers, activations, the environment that forces the kernel, and what ctx.kernel_name must hold;
# saturated: the family's row that also runs under setting S
ROWS = [
    _row("twin-mfma", [15, 16, 16, 3], "lttl", NO_VALU_OFF, ["no-mfma"], saturated=True),
    _row("twin-mfma", [12, 9, 14, 2], "lstt", NO_VALU_OFF, ["no-mfma"]),
    _row("twin-mfma", [16, 16, 16, 4], "lots", NO_VALU_OFF, ["no-mfma"]),
    _row("twin-valu", [15, 16, 16, 3], "lttl", NO_VALU_ON, ["no-valu"], saturated=True),
    _row("twin-valu", [12, 9, 14, 2], "lstt", NO_VALU_ON, ["no-valu"]),
    _row("twin-valu", [16, 16, 16, 4], "lots", NO_VALU_ON, ["no-valu"]),
    _row("out16-T0=2", [31, 16, 16, 6], "lttl", {}, ["mfma-mlp3 2x1x1x1"], ["no-"]),
    _row("out16-T0=2", [20, 13, 16, 5], "lsol", {}, ["mfma-mlp3 2x1x1x1"], ["no-"], saturated=True),
    _row("one-wave", [15, 32, 32, 5], "lttl", ONE_WAVE, [], ["coop"], saturated=True),
    _row("one-wave", [20, 64, 64, 6], "lstl", ONE_WAVE, [], ["coop"]),
    _row("coop", [15, 64, 64, 6], "lttl", {}, [], ["no4"], ends=" coop", saturated=True),
    _row("coop", [30, 48, 48, 5], "ltol", {}, [], ["no4"], ends=" coop"),
    _row("coop-no4", [15, 64, 64, 3], "lttl", {}, ["no4 coop"], saturated=True),
    _row("coop-no4", [20, 32, 32, 4], "lstl", {}, ["no4 coop"]),
    _row("generic", [4, 54, 26, 17, 5], "ltsll", {}, ["generic"]),
    _row("generic", [12, 32, 1], "ltl", {}, ["generic"], saturated=True),
    _row("generic", [20, 80, 80, 3], "lttl", {}, ["generic"]),
    _row("generic", [33, 16, 16, 6], "lttl", {}, ["generic"]),           # 33 inputs are three tiles: no tile kernel
]
FAMILIES = list(dict.fromkeys(r["family"] for r in ROWS))


def cases():
    """(row index, setting) of every case: each row under A and B, one row per family under S."""
    out = [(i, s) for i in range(len(ROWS)) for s in "AB"]
    return out + [(i, "S") for i, r in enumerate(ROWS) if r["saturated"]]


def case_id(c):
    r = ROWS[c[0]]
    return "%s-%s-%s-%s" % (r["family"], "x".join(map(str, r["layers"])), r["ac"], c[1])


def theta(layers, gain, bamp, seed):
    """synth.make_theta(seed) with every weight times gain, biases ~ U[-bamp, bamp], LogStd ~ U[-1, 0.3]."""
    th = synth.make_theta(layers, seed=seed)
    pos = 0
    for i in range(len(layers) - 1):
        fin, out = layers[i], layers[i + 1]
        th[pos:pos + fin * out] *= gain
        pos += fin * out
        th[pos:pos + out] = synth.uniform(seed + 50 + i, synth.STREAM_W, out, -bamp, bamp)
        pos += out
    th[pos:] = synth.uniform(seed + 99, synth.STREAM_W, layers[-1], -1.0, 0.3)
    return th


def obs(n, dim, oscale, seed):
    return oscale * synth.make_obs(n, dim, seed=seed)


def _split(layers, vec):
    """[(W [in][out], B [out])] per layer and the LogStd block of a flat parameter vector."""
    parts, pos = [], 0
    for i in range(len(layers) - 1):
        fin, out = layers[i], layers[i + 1]
        parts.append((vec[pos:pos + fin * out].reshape(fin, out), vec[pos + fin * out:pos + fin * out + out]))
        pos += fin * out + out
    return parts, vec[pos:]


def tanh_fast_np(x):
    """The tile kernels' tanh_fast (csrc/trpo_kernels.hip) in numpy float32: both branches, same constants."""
    f = np.float32
    x = np.asarray(x, f)
    with np.errstate(over="ignore", invalid="ignore"):      # the branch not taken may overflow
        ax, u = np.abs(x), x * x
        q = u * f(-0.006104945205152035) + f(0.021003639325499535)
        q = u * q + f(-0.05385249853134155)
        q = u * q + f(0.13332782685756683)
        q = u * q + f(-0.333333283662796)
        ts = ax * u * q + ax
        e = np.exp2(ax * f(2.8853900817779268))
    tb = f(1.0) - f(2.0) / (e + f(1.0))
    return np.copysign(np.where(ax < f(BRANCH), ts, tb), x).astype(f)


def _act(a, x, fast):
    """(y, dy/dx) of one layer; fast: the fp32 kernels' tanh_fast and the plain logistic."""
    one = x.dtype.type(1.0)
    if a == "t":
        y = tanh_fast_np(x) if fast else np.tanh(x)
        return y, one - y * y
    if a == "s":
        with np.errstate(over="ignore"):
            y = one / (one + np.exp(-x))
        return y, y * (one - y)
    if a == "o":
        return x.dtype.type(0.1) * x, np.full_like(x, 0.1)
    return x, np.ones_like(x)


def preact(layers, ac, th, obs):
    """Per weight layer, the pre-activations [n][out] of the float64 forward pass."""
    parts, _ = _split(layers, np.asarray(th, np.float64))
    y, out = np.asarray(obs, np.float64), []
    for i, (W, B) in enumerate(parts):
        x = y @ W + B
        out.append(x)
        y = _act(ac[i + 1], x, False)[0]
    return out


def fvp_np(layers, ac, th, obs, std, v, dtype, damping=0.1):
    """(F + damping I) v as the header of csrc/trpo_kernels.hip states it: forward, R-forward and R-backward
    per sample in dtype, the sums over samples in float64.  float32 takes tanh_fast's two-branch formula."""
    dt = np.dtype(dtype).type
    fast = dt is np.float32
    Wb, _ = _split(layers, np.asarray(th, dt))
    Vb, _ = _split(layers, np.asarray(v, dt))
    v = np.asarray(v, np.float64)
    std = np.asarray(std, dt)
    y = np.asarray(obs, dt)
    n = y.shape[0]
    ry = np.zeros_like(y)
    ys, ds = [y], []
    for i, ((W, B), (VW, VB)) in enumerate(zip(Wb, Vb)):
        x = y @ W + B
        rx = ry @ W + y @ VW + VB
        y, d = _act(ac[i + 1], x, fast)
        ry = rx * d
        ys.append(y)
        ds.append(d)
    g = ry / std / std
    blocks = []
    for i in range(len(layers) - 2, -1, -1):
        g = g * ds[i]
        g64 = g.astype(np.float64)
        blocks = [(ys[i].astype(np.float64).T @ g64).ravel(), g64.sum(axis=0)] + blocks
        g = g @ Wb[i][0].T
    A = layers[-1]
    out = np.concatenate(blocks + [np.zeros(A)]) / n
    out[-A:] = 2.0 * v[-A:]
    return out + damping * v


def cg_np(F, b, k, resth=0.0):
    """At most k steps of the reference's CG recurrences (src/TRPO_CG.c) in float64 on the product F, from
    x = 0; like the reference it stops before a step once rdotr < resth."""
    b = np.asarray(b, np.float64)
    x, r, p = np.zeros_like(b), b.copy(), b.copy()
    rdotr = float(r @ r)
    for _ in range(k):
        if rdotr < resth:
            break
        z = np.asarray(F(p), np.float64)
        alpha = rdotr / float(p @ z)
        x = x + alpha * p
        r = r - alpha * z
        nr = float(r @ r)
        p = r + (nr / rdotr) * p
        rdotr = nr
    return x


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def problem(row, setting, seed=0, n=N):
    """The inputs of one case, built once and read-only: theta, obs, std = exp(LogStd), the FVP direction v,
    the CG right-hand side b, a rollout (Mean = the policy's own output, from the oracle's forward pass) and
    the line-search direction fs of tests/test_gpu_surrogate.py."""
    r = ROWS[row]
    L, ac = r["layers"], r["ac"]
    oscale, gain, bamp = SETTINGS[setting]
    th = theta(L, gain, bamp, seed)
    ob = obs(n, L[0], oscale, seed)
    A, P = L[-1], synth.num_params(L)
    std = np.exp(th[-A:])
    mean = oracle.forward(L, ac, th, ob)
    action = mean + std * synth.normal(seed + 500, synth.STREAM_ACT, n * A).reshape(n, A)
    adv = synth.normal(seed + 500, synth.STREAM_ADV, n)
    fs = 0.05 * np.random.default_rng(5).standard_normal(P) * np.abs(th).mean()
    p = dict(layers=L, ac=ac, theta=th, obs=ob, std=std, v=synth.make_v(P, seed=seed + 300),
             b=synth.make_b(P, seed=seed + 400), mean=mean, action=action, adv=adv, fs=fs)
    for a in p.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return p


def kl_closed_form(L, ac, th_k, ob, mean_old, std):
    """tests/test_gpu_trust.py's closed form of the mean KL(old || candidate); the candidate's means come
    from the oracle's forward pass (libm tanh: synth.policy_mean's continued fraction is for |x| < 4)."""
    A = L[-1]
    mu = oracle.forward(L, ac, th_k, ob)
    ls = th_k[-A:]
    w = np.exp(-2.0 * ls)
    q = 0.0
    for i in range(A):
        d = mean_old[:, i] - mu[:, i]
        q += float(np.sum(d * d)) * w[i]
    sig = 0.0
    for i in range(A):
        sig += ls[i] - np.log(std[i]) + std[i] * std[i] / (2.0 * np.exp(2.0 * ls[i])) - 0.5
    return sig, q / (2.0 * ob.shape[0])


def mfma_surrogate(L):
    """Whether the line-search sums of this shape take the fp64 MFMA kernel (csrc/trpo_update.hip,
    surr_mfma_shape) unless TRPO_SURR_GENERIC=1 sends them to the register or one-lane kernel."""
    if len(L) != 4 or L[0] > 32 or L[3] > 16 or L[1] > 64 or L[2] > 64:
        return False
    return -(-L[1] // 16) == -(-L[2] // 16)


def decision_margin(ref, accept=0.1, rel=1e-3):
    """Whether the oracle's line search decided every candidate it evaluated with a relative margin rel:
    the accepted one's ratio above accept (1 + rel) with a positive improvement, every one before it (all of
    them when none was accepted) below accept (1 - rel) or with an improvement below -rel |expected|."""
    for k in range(ref["evaluated"]):
        a, e, r = ref["actual"][k], ref["expected"][k], ref["ratio"][k]
        if k == ref["accepted"]:
            if not (r >= accept * (1.0 + rel) and a >= rel * abs(e)):
                return False
        elif not (r <= accept * (1.0 - rel) or a <= -rel * abs(e)):
            return False
    return True


CG_ITERS, CG32_GATE, CG64_GATE = 10, 1e-5, 1e-6


@functools.lru_cache(maxsize=None)
def gates(row, setting, seed=0):
    """The oracle's results for one case and the gates that say where CG and the update are compared.

    sens64:   relative L2 between oracle.cg on the rows as given and on the rows reversed: the reference's own
              sensitivity to the order of its sums.  The fp64 mode is compared when sens64 <= 1e-6, at
              max(1e-9, 100 sens64).
    cg32:     plain float64 CG recurrences on the float32 emulation of the FVP against oracle.cg.  The fp32 solve
              is compared (at the project's 1e-4) when cg32 <= 1e-5: plain float32 without reorthogonalisation
              is ten times inside the bound, so a miss is the kernel's.
    upd32:    the same for the update's own solve: its right-hand side is the policy gradient and it stops
              at rdotr < 1e-10.  The update is compared when cg32 and upd32 are <= 1e-5 and the oracle's line
              search decided with a margin (decision_margin)."""
    p = problem(row, setting, seed)
    L, ac, th, ob, std = p["layers"], p["ac"], p["theta"], p["obs"], p["std"]
    zr, _ = oracle.fvp(L, ac, th, ob, std, p["v"])
    xr = oracle.cg(L, ac, th, ob, std, p["b"], CG_ITERS, 0.0)["x"]
    xrev = oracle.cg(L, ac, th, np.ascontiguousarray(ob[::-1]), std, p["b"], CG_ITERS, 0.0)["x"]
    bref, _ = oracle.policy_grad(L, ac, th, ob, p["mean"], p["action"], p["adv"])
    upd = oracle.update(L, ac, th, ob, p["mean"], p["action"], p["adv"], std, 0.1)

    def F32(q):
        return fvp_np(L, ac, th, ob, std, q, np.float32)

    g = dict(zr=zr, xr=xr, bref=bref, upd=upd, sens64=rel_l2(xrev, xr),
             cg32=rel_l2(cg_np(F32, p["b"], CG_ITERS), xr),
             upd32=rel_l2(cg_np(F32, bref, CG_ITERS, 1e-10), upd["x"]), margin=decision_margin(upd))
    g["cmp64"] = g["sens64"] <= CG64_GATE
    g["cmp32"] = g["cg32"] <= CG32_GATE
    g["cmp_upd"] = g["cmp32"] and g["upd32"] <= CG32_GATE and g["margin"]
    return g


# the cases whose fp32 CG and update comparisons the GPU test relies on (tests/test_trained_inputs.py asserts
# that the gates admit them): every family has some.  All at seed 0; measured values in profiles/trained_policy.md
RELY_CG32 = {
    "twin-mfma": [(0, "B"), (0, "S"), (2, "A"), (2, "B")],
    "twin-valu": [(3, "B"), (3, "S"), (5, "A"), (5, "B")],
    "out16-T0=2": [(6, "B")],
    "one-wave": [(8, "A"), (8, "B"), (8, "S")],
    "coop": [(10, "A"), (10, "B"), (10, "S"), (11, "B")],
    "coop-no4": [(12, "A"), (12, "B"), (12, "S")],
    "generic": [(15, "A"), (15, "B"), (15, "S"), (16, "A"), (16, "B"), (17, "A"), (17, "B")],
}
RELY_UPDATE = {
    "twin-mfma": [(0, "B"), (0, "S"), (2, "A"), (2, "B")],
    "twin-valu": [(3, "B"), (3, "S"), (5, "A"), (5, "B")],
    "out16-T0=2": [(6, "B")],
    "one-wave": [(8, "B"), (8, "S")],
    "coop": [(10, "A"), (10, "B"), (10, "S")],
    "coop-no4": [(12, "B"), (12, "S")],
    "generic": [(15, "A"), (15, "B"), (15, "S"), (16, "A"), (16, "B"), (17, "B")],
}
