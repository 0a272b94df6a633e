"""The value-baseline kernels off the [16,16,16,1] lane path: the case table of tests/test_gpu_baseline_forms.py
and its host references, checked on the CPU by tests/test_baseline_forms_inputs.py.

The one-sample-per-lane kernels (baseline_kernel, baseline_predict_kernel, vfit_kernel, vfit_cand_kernel) are
compiled in up to three forms, chosen by rows_plan (csrc/upd_host.h) from 8 rows 65 bytes (+ 8 theta) against
the 160 KiB of LDS.  With S the sum of the layer widths and P the weights and biases:

    user                       rows                                          theta staged
    evaluate                   2 S + 2                                       P
    predict (advantage stage)  S, or evaluate's stride when that is scratch   P
    Gauss-Newton product       3 S + 2                                       2 P
    candidates                 S                                             -

ROWS names, per shape, the form each user must report through Baseline.kernel_name ("lane": the lane-parallel
kernels of [L0, L1, L2, 1] nets with widths <= 16; the prediction pass has no lane form).  Inputs come from
vfit_ref.problem at two settings of the weights' scale: 0.3 (the suite's) and 1.0, at which the first-layer
pre-activations of the wide shapes reach |z| = 17 .. 21 and tanh units saturate.
"""
import functools

import numpy as np

import oracle
import vfit_ref as R

SCALES = {"small": 0.3, "sat": 1.0}
EPS, K, TH, LAM, NK = 0.01, 10, 1e-10, 1e-3, 4           # tests/test_gpu_vfit.py's fit settings
FIT_GATE = 1e-9                                          # ... and its rule for an end-to-end comparison
ADV_COEFFS = [(0.995, 0.98), (0.0, 0.5)]
ADV_GATE = 0.05                                          # tests/test_gpu_advantage.py's conditioning rule
TABLE_BATCHES = ((1, 130), (2, 65))                      # two full 64-sample passes and a third of two
BIG = (1, 65606)                                         # 1024 blocks, then a second grid-stride trip of 70


def _row(layers, ac, ev, predict, gnvp, cand, batches=TABLE_BATCHES, why="", seed=11):
    name = "eval=%s predict=%s gnvp=%s cand=%s" % (ev, predict, gnvp, cand)
    return dict(layers=tuple(layers), ac=ac, forms=dict(eval=ev, predict=predict, gnvp=gnvp, cand=cand), name=name,
                batches=tuple(batches), why=why, seed=seed)


T, Y, G, LANE = "lds+theta", "lds", "scratch", "lane"
ROWS = [
    _row([16, 40, 40, 1], "lttl", T, T, Y, Y, why="vfit_kernel<true,false>"),
    _row([16, 64, 64, 1], "lttl", Y, T, G, Y, why="baseline_kernel<true,false>, vfit_kernel<false,false>"),
    _row([16, 128, 16, 1], "lttl", G, G, G, Y,
         why="baseline_kernel<false,false>, baseline_predict_kernel<false,false> at evaluate's stride"),
    _row([16, 300, 1], "ltl", G, G, G, G, why="vfit_cand_kernel<false>"),
    _row([5, 7, 13, 6, 1], "ltttl", T, T, T, Y, why="remainder loops forward and backward, odd widths"),
    _row([4, 6, 5, 7, 3, 6, 2, 1], "ltttttll", T, T, T, Y, why="nl = MAXL"),
    _row([6, 7, 3, 1], "lttl", LANE, T, LANE, LANE, why="narrow lane widths, L1 != L2"),
    _row([16, 5, 16, 1], "ltll", LANE, T, LANE, LANE, why="lane widths, L1 < L2"),
    _row([2, 3, 1, 1], "lttl", LANE, T, LANE, LANE, batches=((1, 17),), why="lane width 1",
         seed=12),                                       # seed 11 is no case for a fit: fit_reorder_distance
    _row([5, 1], "ll", T, T, T, Y, batches=(BIG,), why="evaluate's second grid-stride trip"),
    _row([3, 4, 1], "ltl", T, T, T, Y, batches=(BIG,), why="evaluate's second grid-stride trip"),
]
WIDE, DEEP, LANES, BIGS = (0, 1, 2, 3), (4, 5), (6, 7, 8), (9, 10)
ADV_ROWS = WIDE + DEEP                                   # the advantage stage's rows, at 2 x 65
ADV_BATCH = (2, 65)

# every form of every one-sample-per-lane kernel the host can select (ROWS_FORM, csrc/upd_host.h).  The
# prediction pass has no "lds": theta always fits behind its S rows when evaluate's 2 S + 2 rows fit at all
# (predict_plan, csrc/trpo_update.hip); the candidates stage no theta.
SELECTABLE = {"eval": {T, Y, G}, "predict": {T, G}, "gnvp": {T, Y, G}, "cand": {Y, G}}

# (row, batch, setting) whose end-to-end fit the GPU test relies on; tests/test_baseline_forms_inputs.py asserts
# that the gate admits each and that they cover every product form, every candidates form and both settings
RELY_FIT = [
    (0, (2, 65), "small"), (0, (2, 65), "sat"),
    (2, (2, 65), "sat"),
    (3, (2, 65), "small"), (3, (2, 65), "sat"),
    (4, (2, 65), "sat"), (5, (2, 65), "sat"),
    (6, (2, 65), "sat"), (7, (2, 65), "small"), (7, (2, 65), "sat"), (8, (1, 17), "small"),
]
# Outside the gate (sensitivity): [5,7,13,6,1] small 4e-3, [4,6,5,7,3,6,2,1] small 4e-6, [6,7,3,1] small 2e-2:
# small deep or narrow nets whose ten CG steps do not converge.  Each of those rows is relied on under its other
# setting; their products and evaluations are compared under both.


def cases(rows=None, big=True):
    """(row, (num_ep, ep_len), setting) of every case of the given rows."""
    rows = range(len(ROWS)) if rows is None else rows
    return [(i, b, s) for i in rows for b in ROWS[i]["batches"] if big or b != BIG for s in SCALES]


def case_id(c):
    r = ROWS[c[0]]
    return "%s-%s-%dx%d-%s" % ("x".join(map(str, r["layers"])), r["ac"], c[1][0], c[1][1], c[2])


def parse_name(name):
    """Baseline.kernel_name as a dict user -> form."""
    return dict(f.split("=") for f in name.split())


@functools.lru_cache(maxsize=None)
def case(row, batch, setting):
    """The inputs of one case, read-only, in the shape tests/test_gpu_vfit.py's helpers take; x is phi
    zero-padded to a multiple of 16 (the L-BFGS caller's PaddedParams)."""
    r = ROWS[row]
    num_ep, ep_len = batch
    phi, observ, y = R.problem(r["layers"], num_ep, ep_len, r["seed"], SCALES[setting])
    X = R.rows(observ, num_ep, ep_len)
    x = np.zeros((phi.size + 15) // 16 * 16)
    x[:phi.size] = phi
    for a in (X, x):
        a.setflags(write=False)
    return dict(layers=r["layers"], ac=r["ac"], phi=phi, x=x, observ=observ, y=y, X=X, num_ep=num_ep, ep_len=ep_len)


@functools.lru_cache(maxsize=None)
def evaluate_ref(row, batch, setting):
    """(f, g, predictions) of the CPU oracle at the padded x."""
    c = case(row, batch, setting)
    f, g, pred = oracle.baseline_evaluate(list(c["layers"]), c["ac"], c["x"], c["observ"], c["y"], c["num_ep"],
                                          c["ep_len"])
    g.setflags(write=False)
    pred.setflags(write=False)
    return f, g, pred


def evaluate_longdouble(layers, ac, phi, X, y):
    """The objective in numpy.longdouble from its definition: forward pass, output seed 0.02 d with
    d = V - y, backward pass, g = sum / N + 0.002 phi, f = 0.01 sum d^2 / N + 0.001 |phi|^2."""
    ld = np.longdouble
    phi, X, y = np.asarray(phi, ld), np.asarray(X, ld), np.asarray(y, ld)
    N = X.shape[0]
    ys, Ws, at = [X], [], 0
    for i in range(len(layers) - 1):
        a, b = layers[i], layers[i + 1]
        W, B = phi[at:at + a * b].reshape(a, b), phi[at + a * b:at + a * b + b]
        at += a * b + b
        z = _ld_matmul(ys[-1], W) + B
        ys.append(np.tanh(z) if ac[i + 1] == "t" else z)
        Ws.append(W)
    V = ys[-1][:, 0]
    d = V - y
    delta = (ld(0.02) * d)[:, None]
    blocks = []
    for i in range(len(layers) - 2, -1, -1):
        if ac[i + 1] == "t":
            delta = delta * (ld(1.0) - ys[i + 1] ** 2)
        blocks.append((_ld_matmul(ys[i].T, delta).ravel(), delta.sum(axis=0)))
        delta = _ld_matmul(delta, Ws[i].T)
    g = np.concatenate([v for gw, gb in reversed(blocks) for v in (gw, gb)]) / ld(N) + ld(0.002) * phi
    f = ld(0.01) * (d * d).sum() / ld(N) + ld(0.001) * (phi * phi).sum()
    return f, g, V


def _ld_matmul(A, B):
    """A @ B in long double, the inner index in chunks (numpy has no BLAS for it; memory stays bounded)."""
    out = np.zeros((A.shape[0], B.shape[1]), np.longdouble)
    step = max(1, (1 << 22) // max(1, A.shape[0] * B.shape[1]))
    for k in range(0, A.shape[1], step):
        out += (A[:, k:k + step, None] * B[None, k:k + step, :]).sum(axis=1)
    return out


def rel_l2(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.sqrt(((a - b) ** 2).sum()) / np.sqrt((b ** 2).sum()))


def preact_max(row, batch, setting):
    """Largest first-layer |z| of a case (how far its tanh units are driven)."""
    c = case(row, batch, setting)
    a, b = c["layers"][0], c["layers"][1]
    return float(np.abs(c["X"] @ c["phi"][:a * b].reshape(a, b) + c["phi"][a * b:a * b + b]).max())


@functools.lru_cache(maxsize=None)
def jacobian(row, batch, setting):
    c = case(row, batch, setting)
    J = R.forward_jac(c["layers"], c["ac"], c["phi"], c["X"])[1]
    J.setflags(write=False)
    return J


FIT_ARGS = (EPS, K, TH, LAM, NK, np.inf)


@functools.lru_cache(maxsize=None)
def fit_sensitivity(row, batch, setting):
    """vfit_ref.sensitivity of a case at the module's fit settings."""
    c = case(row, batch, setting)
    return R.sensitivity(c["layers"], c["ac"], c["phi"], c["X"], c["y"], *FIT_ARGS)[0]


@functools.lru_cache(maxsize=None)
def fit_reorder_distance(row, batch, setting, trials=2):
    """vfit_ref.distance between the reference fit and itself under seeded random orders of the samples.
    Reversing 17 samples changes almost no bit of a sum, so vfit_ref.sensitivity can come out far below what
    another order of summation does to the fit: [2,3,1,1] at seed 11 and scale 0.3 reverses to 7e-14 while
    random orders move it by 5e-11 (its CG takes |r| down by 1e7 in four steps, and a long-double solve lies
    7e-10 from the float64 reference itself).  A case is relied on only if the bound it will be compared at,
    max(1e-12, 100 x sensitivity), holds between the reference and its own reorderings."""
    c = case(row, batch, setting)
    fwd = R.fit(c["layers"], c["ac"], c["phi"], c["X"], c["y"], *FIT_ARGS)
    rng, worst = np.random.default_rng(0), 0.0
    for _ in range(trials):
        got = R.fit(c["layers"], c["ac"], c["phi"], c["X"], c["y"], *FIT_ARGS, perm=rng.permutation(c["X"].shape[0]))
        if got["cg_iters"] != fwd["cg_iters"] or got["accepted"] != fwd["accepted"]:
            return np.inf
        worst = max(worst, R.distance(got, fwd)[0])
    return worst


@functools.lru_cache(maxsize=None)
def reward(num_ep, ep_len, seed=7):
    r = -np.abs(np.random.default_rng(seed).normal(1.0, 0.7, num_ep * ep_len))
    r.setflags(write=False)
    return r


def discounted(x, c):
    """y[e, t] = sum_k c^k x[e, t + k], as direct sums."""
    T_ = x.shape[1]
    k = np.arange(T_)[None, :] - np.arange(T_)[:, None]
    M = np.where(k >= 0, np.power(float(c), np.maximum(k, 0)), 0.0)
    return (x[:, None, :] * M[None, :, :]).sum(axis=2)


@functools.lru_cache(maxsize=None)
def advantage_ref(row, setting, gamma, lam, batch=ADV_BATCH):
    """tests/test_gpu_advantage.py::reference's construction on a case of this table: direct sums, a two-pass
    mean and variance, V from the CPU oracle; `conditioning` = std A / max |A|."""
    num_ep, ep_len = batch
    V = evaluate_ref(row, batch, setting)[2].reshape(num_ep, ep_len)
    r = reward(num_ep, ep_len).reshape(num_ep, ep_len)
    Vn = np.concatenate([V[:, 1:], np.zeros((num_ep, 1))], axis=1)
    delta = r + gamma * Vn - V
    ret = discounted(r, gamma).ravel()
    A = discounted(delta, gamma * lam).ravel()
    am = A.sum() / A.size
    asd = np.sqrt(((A - am) ** 2).sum() / A.size)
    Rs = r.sum(axis=1)
    rm = Rs.sum() / Rs.size
    rsd = np.sqrt(((Rs - rm) ** 2).sum() / Rs.size)
    out = dict(ret=ret, adv=(A - am) / asd, A=A, ep_rew_mean=rm, ep_rew_std=rsd, adv_mean=am, adv_std=asd,
               conditioning=asd / np.abs(A).max())
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# the ragged case: [16,128,16,1], every episode truncated, so the prediction pass runs n + 3 rows in scratch
RAGGED_ROW, RAGGED_LENS, RAGGED_HORIZON = 2, (63, 64, 65), 65
