"""MI355X tests of the device trust-region value fit (trpo_baseline_gnvp, trpo_baseline_fit_tr).

The yardstick is tests/vfit_ref.py: numpy fp64, the explicit per-sample Jacobian, the explicit H, the CG
recurrences as written.  Bounds:
  * the Gauss-Newton product: relL2 <= 1e-12, the bound the baseline gradient is held to;
  * a whole fit (s, the residual history, alpha_tr, loss[], shift[], x_out -- vfit_ref.distance): per case
    max(1e-12, 100 x the reference's own difference between forward and reversed sample order); a case is
    compared end to end only when that sensitivity is <= 1e-9 (asserted).
The end-to-end comparisons run max_backtracks = 4: shift[k] is a squared difference of predictions that lie
0.5^k alpha0 |J s| apart, so the number format's own error in it grows as 2^k u |V| / |dV| and passes 1e-12 near
k = 9 whatever the summation order; at k < 4 it stays two orders below the bound.  The decisions of the search
are tested at the trainer's 10.

Grids (csrc/trpo_update.hip): the lane form runs min(ceil(N / 16), 256) blocks of 16 sample groups, so N = 4113
gives a second grid-stride trip of 17 samples (block 1 holds one); the generic form min(ceil(N / 64), 1024)
blocks of 64 lanes, so N = 65606 gives a second trip of 70 (block 1 holds six).

Not tested: the refusal of a fit while an evaluation is in flight.  The library refuses it (the device
object's started flag), but the public interface has no call that leaves an evaluation in flight.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ragged_ref
import trpo_amd
import vfit_ref as R
from trpo_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-12
TRPO_E_INVALID = -1
EPS, K, TH, LAM, NK = 0.01, 10, 1e-10, 1e-3, 4          # the comparisons' settings
LANE = [((16, 16, 16, 1), "lttl"), ((6, 7, 3, 1), "lttl"), ((16, 16, 16, 1), "ltll"), ((6, 7, 3, 1), "ltll")]
GENERIC = [((5, 1), "ll"), ((12, 32, 1), "ltl"), ((4, 8, 8, 8, 1), "ltttl")]
BATCHES = [(1, 1), (1, 17), (20, 15)]
BIG = [((16, 16, 16, 1), "lttl", 1, 4113), ((6, 7, 3, 1), "lttl", 1, 4113), ((5, 1), "ll", 1, 65606)]


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def case(layers, ac, num_ep, ep_len, seed=11):
    phi, observ, y = R.problem(layers, num_ep, ep_len, seed)
    X = R.rows(observ, num_ep, ep_len)
    X.setflags(write=False)
    return dict(layers=layers, ac=ac, phi=phi, observ=observ, y=y, X=X, num_ep=num_ep, ep_len=ep_len)


@functools.lru_cache(maxsize=None)
def jacobian(layers, ac, num_ep, ep_len, seed=11):
    c = case(layers, ac, num_ep, ep_len, seed)
    J = R.forward_jac(layers, ac, c["phi"], c["X"])[1]
    J.setflags(write=False)
    return J


def baseline(c):
    b = trpo_amd.Baseline(list(c["layers"]), c["ac"])
    b.set_data(c["observ"], c["y"], c["num_ep"], c["ep_len"])
    return b


def as_dict(x_out, step, info, nk):
    """A device fit in the shape vfit_ref.fit returns."""
    return dict(s=step, x_out=x_out, rdotr=np.array(info.rdotr[:info.cg_iters + 1]), cg_iters=int(info.cg_iters),
                loss_before=info.loss_before, gnorm=info.gnorm, shs=info.shs, alpha_tr=info.alpha_tr,
                alpha0=info.alpha0, loss=np.array(info.loss[:nk]), shift=np.array(info.shift[:nk]),
                accepted=info.accepted)


def dev_fit(b, phi, eps=EPS, k=K, th=TH, lam=LAM, nk=NK, cap=np.inf):
    return as_dict(*b.fit_tr(phi, eps, k, th, lam, nk, cap), nk)


def compare(b, c, X=None, **kw):
    """One end-to-end comparison under the module's bound; returns the device fit and the reference."""
    args = dict(eps=EPS, k=K, th=TH, lam=LAM, nk=NK, cap=np.inf)
    args.update(kw)
    X = c["X"] if X is None else X
    pos = (args["eps"], args["k"], args["th"], args["lam"], args["nk"], args["cap"])
    sens, ref = R.sensitivity(c["layers"], c["ac"], c["phi"], X, c["y"], *pos)
    assert sens <= 1e-9, "ill-conditioned case: not one for an end-to-end comparison"
    bound = max(TOL, 100.0 * sens)
    got = dev_fit(b, c["phi"], **args)
    fig, figs = R.distance(got, ref)
    print("%s %s N=%d: device %.3e  bound %.3e  (reference sensitivity %.3e)  %s" % (
        c["layers"], c["ac"], X.shape[0], fig, bound, sens, {k_: "%.1e" % v for k_, v in figs.items()}))
    assert got["cg_iters"] == ref["cg_iters"]
    assert got["accepted"] == ref["accepted"]
    assert fig <= bound
    for name in ("loss_before", "gnorm", "shs", "alpha0"):
        assert abs(got[name] - ref[name]) <= bound * abs(ref[name]), name
    return got, ref, bound


# 1. the Gauss-Newton product
@pytest.mark.parametrize("layers,ac,num_ep,ep_len",
                         [(l, a, ne, el) for l, a in LANE + GENERIC for ne, el in BATCHES] + BIG)
def test_gnvp(layers, ac, num_ep, ep_len):
    c, J = case(layers, ac, num_ep, ep_len), jacobian(layers, ac, num_ep, ep_len)
    N, P = J.shape
    rng = np.random.default_rng(3)
    u, v = rng.normal(0.0, 1.0, P), rng.normal(0.0, 1.0, P)
    with baseline(c) as b:
        Hv, Hu = b.gnvp(c["phi"], v, LAM), b.gnvp(c["phi"], u, LAM)
        e = np.zeros(P)
        e[-1] = 1.0
        He = b.gnvp(c["phi"], e, 0.0)
        padded = b.gnvp(np.concatenate([c["phi"], np.ones(3)]), np.concatenate([v, np.ones(3)]), LAM)
    err = max(rel_l2(Hv, J.T @ (J @ v) / N + LAM * v), rel_l2(Hu, J.T @ (J @ u) / N + LAM * u))
    print("%s %s N=%d: gnvp relL2 %.3e" % (layers, ac, N, err))
    assert err <= TOL
    # symmetric: each side is within TOL |u| |Hv| of the exact bilinear form
    assert abs(u @ Hv - v @ Hu) <= 2 * TOL * max(np.linalg.norm(u) * np.linalg.norm(Hv),
                                                 np.linalg.norm(v) * np.linalg.norm(Hu))
    assert v @ Hv >= LAM * (v @ v)
    # no damping, the unit vector of the (linear) output bias: j . e = 1, the product is the mean Jacobian row
    assert rel_l2(He, J.sum(axis=0) / N) <= TOL
    np.testing.assert_array_equal(padded[:P], Hv)
    np.testing.assert_array_equal(padded[P:], 0.0)


# 2. the fit against the reference
@pytest.mark.parametrize("layers,ac,num_ep,ep_len", [
    ((16, 16, 16, 1), "lttl", 20, 15), ((12, 32, 1), "ltl", 1, 65), ((5, 1), "ll", 1, 40),
    ((16, 16, 16, 1), "ltll", 20, 15), ((16, 16, 16, 1), "lttl", 1, 1), ((5, 1), "ll", 1, 1),
    ((12, 32, 1), "ltl", 1, 17), ((16, 16, 16, 1), "lttl", 1, 4113), ((5, 1), "ll", 1, 65606)])
def test_fit_against_reference(layers, ac, num_ep, ep_len):
    c = case(layers, ac, num_ep, ep_len)
    with baseline(c) as b:
        compare(b, c)


def test_ragged_batch_keeps_bootstrap_rows_out():
    """A ragged advantage stage with truncated episodes leaves its bootstrap rows behind the samples; data set
    with set_data_ragged afterwards is fitted on the n sample rows alone."""
    lens, horizon = ragged_ref.LENGTHS["1-128-129-200-7"], 200
    x, observ, reward, boot_observ = ragged_ref.inputs(lens)
    n = int(sum(lens))
    rng = np.random.default_rng(5)
    y = np.tanh(observ[:, 0]) + 0.5 * rng.normal(0.0, 1.0, n)
    X = np.column_stack([observ, ragged_ref.time_feature(lens, horizon)])
    c = dict(layers=ragged_ref.BASE, ac=ragged_ref.AC, phi=x, y=y)
    J = R.forward_jac(c["layers"], c["ac"], x, X)[1]
    v = rng.normal(0.0, 1.0, x.size)
    with trpo_amd.Baseline(list(ragged_ref.BASE), ragged_ref.AC) as b:
        b.advantage_ragged(x, observ, reward, lens, horizon, boot_observ=boot_observ,
                           boot=ragged_ref.boot_flags("all", len(lens)))
        b.set_data_ragged(observ, y, lens, horizon)
        Hv = b.gnvp(x, v, LAM)
        err = rel_l2(Hv, J.T @ (J @ v) / n + LAM * v)
        print("ragged N=%d: gnvp relL2 %.3e" % (n, err))
        assert err <= TOL
        compare(b, c, X=X)


# 3. the model linear in phi
def test_linear_model_reaches_least_squares():
    layers, ac = (5, 1), "ll"
    c = case(layers, ac, 1, 40)
    P = c["phi"].size
    with baseline(c) as b:
        got, ref, bound = compare(b, c, eps=1e9, k=P + 2, th=0.0, lam=0.0, nk=1)
    A = np.column_stack([c["X"], np.ones(40)])
    best = np.linalg.lstsq(A, c["y"], rcond=None)[0]
    rms = ((A @ best - c["y"]) ** 2).sum() / 40
    print("least squares: x_out %.3e  loss %.3e  bound %.3e" % (
        R.vec_err(got["x_out"], best), abs(got["loss"][0] - rms) / rms, bound))
    assert got["alpha0"] == 1.0 and got["accepted"] == 0
    assert R.vec_err(got["x_out"], best) <= bound
    assert abs(got["loss"][0] - rms) <= bound * rms


# 4. the search's decisions ([6, 7, 3, 1] at N = 17, seed 5: the full Gauss-Newton step overshoots)
DEC = ((6, 7, 3, 1), "lttl", 1, 17, 5)
MARGIN = 1e-3


def test_first_candidate_refused_on_the_loss():
    c = case(*DEC)
    ref = R.fit(c["layers"], c["ac"], c["phi"], c["X"], c["y"], 1e9, K, TH, LAM, 10, np.inf)
    s2 = ref["loss_before"]
    assert ref["alpha0"] == 1.0
    assert ref["loss"][0] > s2 * (1 + MARGIN) and ref["loss"][1] < s2 * (1 - MARGIN)
    with baseline(c) as b:
        got = dev_fit(b, c["phi"], eps=1e9, nk=10)
    print("loss refusal: loss_before %.4g loss[:2] %s accepted %d" % (got["loss_before"], got["loss"][:2],
                                                                     got["accepted"]))
    assert got["loss"][0] > got["loss_before"] > got["loss"][1]
    assert got["accepted"] == 1
    np.testing.assert_array_equal(got["x_out"], c["phi"] + got["alpha0"] * 0.5 * got["s"])


def test_first_candidate_refused_on_the_shift_cap():
    c = case(*DEC)
    cap = 0.015
    ref = R.fit(c["layers"], c["ac"], c["phi"], c["X"], c["y"], EPS, K, TH, LAM, 10, cap)
    s2 = ref["loss_before"]
    assert ref["loss"][0] < s2 * (1 - MARGIN) and ref["loss"][1] < s2 * (1 - MARGIN)
    assert ref["shift"][0] > cap * (1 + MARGIN) and ref["shift"][1] < cap * (1 - MARGIN)
    with baseline(c) as b:
        got = dev_fit(b, c["phi"], nk=10, cap=cap)
        free = dev_fit(b, c["phi"], nk=10)
    print("cap refusal: shift[:2] %s accepted %d (uncapped %d)" % (got["shift"][:2], got["accepted"],
                                                                  free["accepted"]))
    assert got["shift"][0] > cap >= got["shift"][1]
    assert got["accepted"] == 1 and free["accepted"] == 0


def test_all_candidates_refused_returns_x():
    c = case(*DEC)
    ref = R.fit(c["layers"], c["ac"], c["phi"], c["X"], c["y"], 1e9, K, TH, LAM, 1, np.inf)
    assert ref["loss"][0] > ref["loss_before"] * (1 + MARGIN) and ref["accepted"] == -1
    x = np.concatenate([c["phi"], np.full(5, 7.0)])            # L-BFGS padding behind the parameters
    with baseline(c) as b:
        x_out, step, info = b.fit_tr(x, 1e9, K, TH, LAM, 1, np.inf)
    assert info.accepted == -1 and info.evaluated == 1
    assert x_out[:c["phi"].size].tobytes() == c["phi"].tobytes()
    np.testing.assert_array_equal(x_out[c["phi"].size:], 0.0)
    np.testing.assert_array_equal(step[c["phi"].size:], 0.0)
    assert np.abs(step).max() > 0.0


# 5. early CG stop
def test_early_cg_stop():
    c = case((16, 16, 16, 1), "lttl", 20, 15)
    full = R.fit(c["layers"], c["ac"], c["phi"], c["X"], c["y"], EPS, K, 0.0, LAM, NK, np.inf)["rdotr"]
    th = float(np.sqrt(full[3] * full[4]))
    assert full[1:4].min() > th * (1 + MARGIN) and full[4] < th * (1 - MARGIN)
    with baseline(c) as b:
        got, ref, _ = compare(b, c, th=th)
        info = b.fit_tr(c["phi"], EPS, K, th, LAM, NK, np.inf)[2]
    assert got["cg_iters"] == ref["cg_iters"] == 4 < K
    assert all(v > 0.0 for v in info.rdotr[:5])
    assert all(v == 0.0 for v in info.rdotr[5:])               # zero beyond cg_iters, as the header says


# 6. repeatability and state
def test_repeatable_and_leaves_the_object_alone():
    c = case((16, 16, 16, 1), "lttl", 20, 15)
    g = case((12, 32, 1), "ltl", 1, 65)
    for cc in (c, g):
        with baseline(cc) as b:
            f0 = b.evaluate(cc["phi"], want_predict=True)
            r1 = b.fit_tr(cc["phi"], EPS, K, TH, LAM, 10, 0.015)
            r2 = b.fit_tr(cc["phi"], EPS, K, TH, LAM, 10, 0.015)
            h1, h2 = b.gnvp(cc["phi"], r1[1], LAM), b.gnvp(cc["phi"], r1[1], LAM)
            f1 = b.evaluate(cc["phi"], want_predict=True)
        assert r1[0].tobytes() == r2[0].tobytes() and r1[1].tobytes() == r2[1].tobytes()
        assert bytes(r1[2]) == bytes(r2[2])
        assert h1.tobytes() == h2.tobytes()
        assert f0[0] == f1[0]
        np.testing.assert_array_equal(f0[1], f1[1])
        np.testing.assert_array_equal(f0[2], f1[2])
        assert r1[2].accepted >= 0 and not np.array_equal(r1[0], cc["phi"])


def test_advantages_survive_a_fit():
    """The paper's order: advantages from the old V, then the fit, then the hand-off of the same bits."""
    layers, num_ep, ep_len = [15, 16, 16, 3], 20, 15
    n = num_ep * ep_len
    lens = (ep_len,) * num_ep
    x, observ, reward, _ = ragged_ref.inputs(lens)
    th = synth.make_theta(layers)
    obs = synth.make_obs(n, layers[0])
    std = np.ones(layers[-1])
    mean, action, _ = synth.make_rollout(layers, "lttl", th, obs, std)
    with trpo_amd.Baseline(list(ragged_ref.BASE), ragged_ref.AC) as bl:
        adv, _, _ = bl.advantage(x, observ, reward, num_ep, ep_len)
        x_new, _, info = bl.fit_tr(x, EPS, K, TH, LAM, 10, 0.015)
        assert info.accepted >= 0
        with trpo_amd.Context(layers, "lttl", th, obs, std, 0.1) as ctx:
            ctx.set_rollout_from(bl, mean, action)
            r = ctx.update()
    with trpo_amd.Context(layers, "lttl", th, obs, std, 0.1) as host:
        host.set_rollout(mean, action, adv)
        s = host.update()
    for k_ in ("theta", "b", "x"):
        np.testing.assert_array_equal(r[k_], s[k_])


def expect_invalid(fn):
    with pytest.raises(trpo_amd.TRPOError) as e:
        fn()
    assert e.value.code == TRPO_E_INVALID
    assert trpo_amd.last_error()
    return e.value


@pytest.mark.parametrize("layers,ac,num_ep,ep_len", [((16, 16, 16, 1), "lttl", 20, 15), ((12, 32, 1), "ltl", 1, 65)])
def test_zero_loss_is_refused_with_x_back(layers, ac, num_ep, ep_len):
    c = case(layers, ac, num_ep, ep_len)
    with baseline(c) as b:
        pred = b.evaluate(c["phi"], want_predict=True)[2]
        b.set_data(c["observ"], pred, num_ep, ep_len)
        err = expect_invalid(lambda: b.fit_tr(c["phi"], EPS, K, TH, LAM, 10, 0.015))
        assert err.x_out.tobytes() == c["phi"].tobytes()
        assert err.info.loss_before == 0.0 and err.info.accepted == -1
        # the object still works
        b.set_data(c["observ"], c["y"], num_ep, ep_len)
        assert b.fit_tr(c["phi"], EPS, K, TH, LAM, 10, 0.015)[2].accepted >= 0


def test_argument_refusals():
    c = case((6, 7, 3, 1), "lttl", 1, 17)
    phi = c["phi"]
    with trpo_amd.Baseline(list(c["layers"]), c["ac"]) as b:
        expect_invalid(lambda: b.fit_tr(phi))                                  # no data
        expect_invalid(lambda: b.gnvp(phi, phi, 0.0))
        b.set_data(c["observ"], c["y"], 1, 17)
        b.fit_tr(phi)
        for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=np.nan), dict(damping=-1e-3), dict(damping=np.nan),
                   dict(shift_cap=0.0), dict(shift_cap=-1.0), dict(shift_cap=np.nan), dict(cg_max_iter=0),
                   dict(cg_max_iter=trpo_amd.VFIT_MAX_CG + 1), dict(max_backtracks=0), dict(max_backtracks=33)):
            expect_invalid(lambda: b.fit_tr(phi, **kw))
        expect_invalid(lambda: b.fit_tr(phi[:-1]))                             # n < NumParams
        expect_invalid(lambda: b.gnvp(phi, phi, -1.0))
        b.fit_tr(phi, cg_max_iter=trpo_amd.VFIT_MAX_CG, max_backtracks=32)     # the limits themselves pass
        out = np.zeros(phi.size)
        L = trpo_amd.lib()
        assert L.trpo_baseline_fit_tr(b._h, None, phi.size, EPS, K, TH, LAM, 10, 0.015, out.ctypes.data, None,
                                      None) == TRPO_E_INVALID
        assert L.trpo_baseline_fit_tr(b._h, phi.ctypes.data, phi.size, EPS, K, TH, LAM, 10, 0.015, None, None,
                                      None) == TRPO_E_INVALID
        # step_out and info may be NULL
        assert L.trpo_baseline_fit_tr(b._h, phi.ctypes.data, phi.size, EPS, K, TH, LAM, 10, 0.015, out.ctypes.data,
                                      None, None) >= 0


# 7. INFINITY cap and eps
def test_infinite_cap_and_eps_scaling():
    c = case((16, 16, 16, 1), "lttl", 20, 15)
    with baseline(c) as b:
        free = b.fit_tr(c["phi"], EPS, K, TH, LAM, 10, np.inf)
        loose = b.fit_tr(c["phi"], EPS, K, TH, LAM, 10, 1e6)
        twice = b.fit_tr(c["phi"], 2 * EPS, K, TH, LAM, 10, np.inf)
    assert max(free[2].shift[:10]) < 1e6
    assert free[0].tobytes() == loose[0].tobytes() and free[1].tobytes() == loose[1].tobytes()
    assert bytes(free[2]) == bytes(loose[2])
    assert free[2].alpha_tr < 1.0 and twice[2].alpha_tr < 1.0
    assert free[2].alpha0 == free[2].alpha_tr
    # one sqrt and one multiplication by 2 apart: a few ulp
    assert abs(twice[2].alpha0 / free[2].alpha0 - np.sqrt(2.0)) <= 1e-15 * 4
