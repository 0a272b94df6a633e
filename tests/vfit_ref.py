"""The numpy fp64 reference of the device trust-region value fit (trpo_baseline_fit_tr, trpo_baseline_gnvp;
tests/test_gpu_vfit.py compares the device with it).

Written from the definitions in include/trpo_mi355x.h: the explicit per-sample Jacobian J [N][P] of the
baseline's prediction, the explicit H = J^T J / N + lambda I, the CG recurrences as written, the candidates
phi + alpha0 0.5^k s with their loss and shift, and the acceptance rule.  `perm` reorders the samples before
anything is summed, so the reference can report its own sensitivity to the order of summation
(`sensitivity`): the device sums in yet another, fixed, order.
"""
import functools

import numpy as np

from trpo_amd import synth


def num_params(layers):
    return synth.num_params(list(layers)) - layers[-1]


def rows(observ, num_ep, ep_len):
    """trpo_baseline_set_data's input rows [observ[s], (s mod ep_len) / ep_len]."""
    n = num_ep * ep_len
    t = (np.arange(n) % ep_len) / float(ep_len)
    return np.column_stack([np.asarray(observ, np.float64).reshape(n, -1), t])


def forward_jac(layers, ac, phi, X, want_jac=True):
    """V [N] and J [N][P], J[s] = grad_phi V_phi(X[s]); weights W[in][out] then biases per layer in phi,
    't' tanh / 'l' linear (ac[0] belongs to the input layer)."""
    X = np.asarray(X, np.float64)
    ys, Ws, at = [X], [], 0
    for i in range(len(layers) - 1):
        a, b = layers[i], layers[i + 1]
        W = phi[at:at + a * b].reshape(a, b)
        B = phi[at + a * b:at + a * b + b]
        at += a * b + b
        z = ys[-1] @ W + B
        ys.append(np.tanh(z) if ac[i + 1] == "t" else z)
        Ws.append(W)
    V = ys[-1][:, 0]
    if not want_jac:
        return V, None
    N = X.shape[0]
    blocks = []
    delta = np.ones((N, 1))
    for i in range(len(layers) - 2, -1, -1):
        if ac[i + 1] == "t":
            delta = delta * (1.0 - ys[i + 1] ** 2)
        gw = ys[i][:, :, None] * delta[:, None, :]             # [N][in][out]
        blocks.append((gw.reshape(N, -1), delta))
        delta = delta @ Ws[i].T
    cols = []
    for gw, gb in reversed(blocks):
        cols += [gw, gb]
    return V, np.concatenate(cols, axis=1)


@functools.lru_cache(maxsize=None)
def problem(layers, num_ep, ep_len, seed=11, scale=0.3, noise=0.5):
    """phi, observ [n][O], target [n] of one case (read-only arrays)."""
    rng = np.random.default_rng(seed)
    n, O = num_ep * ep_len, layers[0] - 1
    phi = scale * rng.normal(0.0, 1.0, num_params(layers))
    observ = rng.normal(0.0, 1.0, (n, O))
    w = rng.normal(0.0, 1.0, O) / np.sqrt(max(O, 1))
    target = np.tanh(observ @ w) + 0.5 * (np.arange(n) % ep_len) / float(ep_len) + noise * rng.normal(0.0, 1.0, n)
    for a in (phi, observ, target):
        a.setflags(write=False)
    return phi, observ, target


def gnvp(layers, ac, phi, X, v, damping):
    """J^T (J v) / N + damping v with the explicit Jacobian."""
    _, J = forward_jac(layers, ac, phi, X)
    return J.T @ (J @ v) / X.shape[0] + damping * v


def fit(layers, ac, phi, X, y, eps, cg_max_iter, th, damping, max_backtracks, shift_cap, perm=None):
    """The fit as the header states it.  Returns a dict of s, rdotr (cg_iters + 1 values), cg_iters,
    loss_before, gnorm, shs, alpha_tr, alpha0, loss, shift (max_backtracks values each), accepted, x_out."""
    X, y = np.asarray(X, np.float64), np.asarray(y, np.float64)
    if perm is not None:
        X, y = X[perm], y[perm]
    N, P = X.shape[0], phi.size
    V0, J = forward_jac(layers, ac, phi, X)
    d = V0 - y
    sig2 = (d * d).sum() / N
    g = J.T @ d / N
    H = J.T @ J / N + damping * np.eye(P)
    s, r = np.zeros(P), -g
    p = r.copy()
    rr = r @ r
    rdotr = [rr]
    iters = 0
    for _ in range(cg_max_iter):
        if not rr > 0.0:
            break
        z = H @ p
        a = rr / (p @ z)
        s = s + a * p
        r = r - a * z
        rn = r @ r
        rdotr.append(rn)
        iters += 1
        if rn < th:
            break
        p = r + (rn / rr) * p
        rr = rn
    q = s @ (H @ s)
    with np.errstate(divide="ignore"):
        alpha_tr = np.sqrt(2.0 * eps * sig2 / q) if q > 0.0 else np.inf
    alpha0 = min(1.0, alpha_tr)
    loss, shift = np.zeros(max_backtracks), np.zeros(max_backtracks)
    accepted = -1
    for k in range(max_backtracks):
        Vk, _ = forward_jac(layers, ac, phi + alpha0 * 0.5 ** k * s, X, want_jac=False)
        loss[k] = ((Vk - y) ** 2).sum() / N
        shift[k] = ((Vk - V0) ** 2).sum() / N / (2.0 * sig2)
        if accepted < 0 and loss[k] < sig2 and shift[k] <= shift_cap:
            accepted = k
    x_out = phi.copy() if accepted < 0 else phi + alpha0 * 0.5 ** accepted * s
    return dict(s=s, rdotr=np.array(rdotr), cg_iters=iters, loss_before=sig2, gnorm=np.sqrt(g @ g), shs=0.5 * q,
                alpha_tr=alpha_tr, alpha0=alpha0, loss=loss, shift=shift, accepted=accepted, x_out=x_out, g=g)


def vec_err(a, b):
    """max |a - b| relative to max |b| (vectors whose entries share a scale)."""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def each_err(a, b):
    """largest element-wise relative difference (entries of their own scales; all of b non-zero)."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return float((np.abs(a - b) / np.abs(b)).max())


def distance(got, ref):
    """The one figure a fit is compared by: the largest of the errors of s, x_out and the residual norms
    sqrt(rdotr[0 .. cg_iters]) (vec_err) and of alpha_tr, loss[] and shift[] (each_err).  The residual
    history is compared as norms relative to the first: once CG has converged (the linear model does within
    P iterations) the later r are rounding residue of size u |r_0|, which no two summation orders share
    element by element.  got and ref are dicts as `fit` returns."""
    n = ref["cg_iters"] + 1
    figs = dict(s=vec_err(got["s"], ref["s"]), x_out=vec_err(got["x_out"], ref["x_out"]),
                rdotr=vec_err(np.sqrt(got["rdotr"][:n]), np.sqrt(ref["rdotr"][:n])),
                alpha_tr=each_err(got["alpha_tr"], ref["alpha_tr"]),
                loss=each_err(got["loss"], ref["loss"]), shift=each_err(got["shift"], ref["shift"]))
    return max(figs.values()), figs


def sensitivity(layers, ac, phi, X, y, *args):
    """The reference's own difference between forward and reversed sample order, by `distance`."""
    fwd = fit(layers, ac, phi, X, y, *args)
    rev = fit(layers, ac, phi, X, y, *args, perm=np.arange(X.shape[0])[::-1])
    if fwd["cg_iters"] != rev["cg_iters"] or fwd["accepted"] != rev["accepted"]:
        return np.inf, fwd
    return distance(rev, fwd)[0], fwd
