"""MI355X tests of the value-baseline kernels off the [16,16,16,1] lane path: every form of baseline_kernel,
baseline_predict_kernel, vfit_kernel and vfit_cand_kernel that the host can select (Y and theta in LDS, Y in
LDS, Y in a global scratch), the lane kernels at narrow and unequal widths, nets of MAXL layers and of odd widths,
evaluate beyond its 1024-block grid, and the one scratch buffer the users share.

The case table and the references are tests/baseline_forms.py, checked on the CPU by
tests/test_baseline_forms_inputs.py.  Every case asserts the form Baseline.kernel_name reports, runs under the
suite's 0.3 N(0, 1) weights and under 1.0 N(0, 1) (saturating tanh units), and prints its figures before it
asserts them.  Bounds, each the one the suite already holds that quantity to: f 1e-13, g and predictions relL2
1e-12 (tests/test_gpu_baseline.py); the Gauss-Newton product relL2 1e-12 and the fit by vfit_ref.distance at
max(1e-12, 100 x the reference's sensitivity) (tests/test_gpu_vfit.py, whose `compare` runs here); the advantage
stage 1e-12 and the gamma = 0 identity 1e-13 (tests/test_gpu_advantage.py).
"""
import numpy as np
import pytest

import baseline_forms as F
import ragged_ref
import trpo_amd
import vfit_ref as R
from test_gpu_vfit import compare

pytestmark = pytest.mark.gpu

TOL = 1e-12
STATS = ("ep_rew_mean", "ep_rew_std", "adv_mean", "adv_std")


def baseline(c, row):
    """A fresh object holding the case's batch, its reported forms asserted."""
    b = trpo_amd.Baseline(list(c["layers"]), c["ac"])
    b.set_data(c["observ"], c["y"], c["num_ep"], c["ep_len"])
    assert b.kernel_name == F.ROWS[row]["name"], b.kernel_name
    return b


# 1. the forms
@pytest.mark.parametrize("row", range(len(F.ROWS)))
def test_forms(row):
    r = F.ROWS[row]
    c = F.case(row, r["batches"][0], "small")
    with trpo_amd.Baseline(list(r["layers"]), r["ac"]) as b:
        assert b.kernel_name == ""
        b.set_data(c["observ"], c["y"], c["num_ep"], c["ep_len"])
        name = b.kernel_name
    print("%s %s: %s" % (r["layers"], r["ac"], name))
    assert name == r["name"]


def test_every_selectable_form_is_run():
    """Every form of every one-sample-per-lane kernel that the host can select is reported by a row of the
    table (and every row's cases assert their form before they compare)."""
    seen = {user: set() for user in F.SELECTABLE}
    for row, r in enumerate(F.ROWS):
        c = F.case(row, r["batches"][0], "small")
        with trpo_amd.Baseline(list(r["layers"]), r["ac"]) as b:
            b.set_data(c["observ"], c["y"], c["num_ep"], c["ep_len"])
            for user, form in F.parse_name(b.kernel_name).items():
                seen[user].add(form)
    for user, forms in F.SELECTABLE.items():
        assert seen[user] - {F.LANE} == forms, (user, seen[user])


# 2. evaluate
@pytest.mark.parametrize("c", F.cases(), ids=F.case_id)
def test_evaluate(c):
    cs = F.case(*c)
    fr, gr, pr = F.evaluate_ref(*c)
    with baseline(cs, c[0]) as b:
        f, g, pred = b.evaluate(cs["x"], want_predict=True)
        npar = b.np
    e_f, e_g, e_p = abs(f - fr) / abs(fr), F.rel_l2(g, gr), F.rel_l2(pred, pr)
    print("%s: f %.2e g %.2e predict %.2e" % (F.case_id(c), e_f, e_g, e_p))
    assert e_f <= 1e-13
    assert e_g <= TOL
    assert e_p <= TOL
    assert g.size == cs["x"].size and np.all(g[npar:] == 0.0)


@pytest.mark.parametrize("c", F.cases(F.LANES), ids=F.case_id)
def test_lane_rows_match_the_one_lane_kernel(c, monkeypatch):
    """tests/test_gpu_baseline.py::test_lane_kernel_matches_one_lane_kernel's rule at narrow and unequal widths:
    the same per-sample bits, only the order of the sums over samples differs."""
    cs = F.case(*c)
    out = {}
    for lane in ("1", "0"):
        monkeypatch.setenv("TRPO_BASELINE_LANE", lane)
        with trpo_amd.Baseline(list(cs["layers"]), cs["ac"]) as b:
            b.set_data(cs["observ"], cs["y"], cs["num_ep"], cs["ep_len"])
            assert F.parse_name(b.kernel_name)["eval"] == (F.LANE if lane == "1" else F.T), b.kernel_name
            out[lane] = b.evaluate(cs["x"], want_predict=True)
    e_f, e_g = abs(out["1"][0] - out["0"][0]) / abs(out["0"][0]), F.rel_l2(out["1"][1], out["0"][1])
    print("%s: lane vs one-lane f %.2e g %.2e" % (F.case_id(c), e_f, e_g))
    np.testing.assert_array_equal(out["1"][2], out["0"][2])
    assert e_f <= 1e-14
    assert e_g <= 1e-13


# 3. the Gauss-Newton product
@pytest.mark.parametrize("c", F.cases(big=False), ids=F.case_id)
def test_gnvp(c):
    cs, J = F.case(*c), F.jacobian(*c)
    N, P = J.shape
    rng = np.random.default_rng(3)
    u, v = rng.normal(0.0, 1.0, P), rng.normal(0.0, 1.0, P)
    with baseline(cs, c[0]) as b:
        Hv, Hu = b.gnvp(cs["phi"], v, F.LAM), b.gnvp(cs["phi"], u, F.LAM)
    err = max(F.rel_l2(Hv, J.T @ (J @ v) / N + F.LAM * v), F.rel_l2(Hu, J.T @ (J @ u) / N + F.LAM * u))
    sym = abs(u @ Hv - v @ Hu) / max(np.linalg.norm(u) * np.linalg.norm(Hv), np.linalg.norm(v) * np.linalg.norm(Hu))
    print("%s: gnvp relL2 %.3e symmetry %.3e" % (F.case_id(c), err, sym))
    assert err <= TOL
    assert sym <= 2 * TOL
    assert v @ Hv >= F.LAM * (v @ v)


# 4. the fit
@pytest.mark.parametrize("c", F.RELY_FIT, ids=F.case_id)
def test_fit(c):
    cs = F.case(*c)
    with baseline(cs, c[0]) as b:
        compare(b, cs, eps=F.EPS, k=F.K, th=F.TH, lam=F.LAM, nk=F.NK, cap=np.inf)


# 5. the advantage stage
def check_advantage(adv, ret, info, ref, what):
    e_ret = np.abs(ret - ref["ret"]).max() / np.abs(ref["ret"]).max()
    e_adv = np.abs(adv - ref["adv"]).max()
    e_st = {k: abs(info[k] - ref[k]) / abs(ref[k]) for k in STATS}
    print("%s: ret %.3e adv %.3e stats %s" % (what, e_ret, e_adv, {k: "%.2e" % v for k, v in e_st.items()}))
    assert e_ret <= TOL
    assert e_adv <= TOL
    for k in STATS:
        assert abs(info[k] - ref[k]) <= TOL * abs(ref[k]), k


@pytest.mark.parametrize("gamma,lam", F.ADV_COEFFS)
@pytest.mark.parametrize("c", [(i, F.ADV_BATCH, s) for i in F.ADV_ROWS for s in F.SCALES], ids=F.case_id)
def test_advantage(c, gamma, lam):
    row, (num_ep, ep_len), setting = c
    cs = F.case(*c)
    ref = F.advantage_ref(row, setting, gamma, lam)
    assert ref["conditioning"] >= F.ADV_GATE
    reward = F.reward(num_ep, ep_len)
    with trpo_amd.Baseline(list(cs["layers"]), cs["ac"]) as b:
        adv, ret, info = b.advantage(cs["x"], cs["observ"], reward, num_ep, ep_len, gamma, lam)
        assert b.kernel_name == F.ROWS[row]["name"], b.kernel_name
        V = b.evaluate(cs["x"], want_predict=True)[2]
    check_advantage(adv, ret, info, ref, "%s (%g, %g)" % (F.case_id(c), gamma, lam))
    if gamma == 0.0:
        # ret = reward exactly and A = reward - V: the prediction pass against baseline_kernel's forward
        np.testing.assert_array_equal(ret, reward)
        want = reward - V
        err = np.abs(adv * info["adv_std"] + info["adv_mean"] - want).max() / np.abs(want).max()
        print("%s: raw advantage vs reward - evaluate's predictions %.3e" % (F.case_id(c), err))
        assert err <= 1e-13


@pytest.mark.parametrize("gamma,lam", F.ADV_COEFFS)
def test_ragged_bootstrap_rows_in_scratch(gamma, lam):
    """[16,128,16,1], every episode truncated: the prediction pass runs n + 3 rows in the scratch form."""
    r = F.ROWS[F.RAGGED_ROW]
    lens, horizon = F.RAGGED_LENS, F.RAGGED_HORIZON
    x, observ, reward, boot_observ = ragged_ref.inputs(lens, r["layers"])
    ref = ragged_ref.reference(lens, horizon, "all", gamma, lam, r["layers"], r["ac"])
    assert ref["conditioning"] >= F.ADV_GATE
    with trpo_amd.Baseline(list(r["layers"]), r["ac"]) as b:
        adv, ret, info = b.advantage_ragged(x, observ, reward, lens, horizon, gamma, lam, boot_observ=boot_observ,
                                            boot=ragged_ref.boot_flags("all", len(lens)))
        assert b.kernel_name == r["name"], b.kernel_name
    check_advantage(adv, ret, info, ref, "ragged %s (%g, %g)" % (lens, gamma, lam))


# 6. one scratch buffer, several users
def same(a, b):
    """Bit-identity of two results: arrays, floats, dicts, ctypes blocks and tuples of them."""
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(p, q) for p, q in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.tobytes() == b.tobytes()
    if isinstance(a, trpo_amd.VFitInfo):
        skip = trpo_amd.VFitInfo.accepted.offset + 4               # (.seconds is a Python attribute, not a field)
        return bytes(a)[:skip] == bytes(b)[:skip]
    return a == b


@pytest.mark.parametrize("row", [2, 3])
def test_one_scratch_buffer_serves_every_user(row):
    """evaluate, gnvp, fit_tr and the advantage stage re-ensure the one scratch buffer with their own row
    counts and grids; on one object, across a growing and a shrinking batch, every result has the bits of the
    same call on a fresh object that has seen that batch alone."""
    r = F.ROWS[row]
    small, big = F.case(row, (1, 17), "sat"), F.case(row, (2, 65), "sat")
    reward = F.reward(2, 65)
    v = np.random.default_rng(3).normal(0.0, 1.0, small["phi"].size)
    phi = small["phi"]
    assert phi.tobytes() == big["phi"].tobytes()

    def put(b, c):
        b.set_data(c["observ"], c["y"], c["num_ep"], c["ep_len"])

    def evaluate(b):
        return b.evaluate(phi, want_predict=True)

    def gnvp(b):
        return b.gnvp(phi, v, F.LAM)

    def fit(b):
        return b.fit_tr(phi, F.EPS, F.K, F.TH, F.LAM, F.NK, np.inf)

    def advantage(b):
        return b.advantage(phi, big["observ"], reward, 2, 65, 0.995, 0.98)

    def fresh(prepare, call):
        with trpo_amd.Baseline(list(r["layers"]), r["ac"]) as b:
            prepare(b)
            return call(b)

    with trpo_amd.Baseline(list(r["layers"]), r["ac"]) as b:
        got = []
        put(b, small)
        got += [evaluate(b), gnvp(b)]
        put(b, big)                                                 # the grid grows from 1 block to 3
        got += [evaluate(b), fit(b), advantage(b), evaluate(b)]
        put(b, small)
        got += [evaluate(b), gnvp(b)]
        assert b.kernel_name == r["name"]
    ret = got[4][1]
    want = [fresh(lambda o: put(o, small), evaluate), fresh(lambda o: put(o, small), gnvp),
            fresh(lambda o: put(o, big), evaluate), fresh(lambda o: put(o, big), fit),
            fresh(lambda o: None, advantage),
            fresh(lambda o: o.set_data(big["observ"], ret, 2, 65), evaluate)]
    want += want[:2]
    steps = ("evaluate 1x17", "gnvp 1x17", "evaluate 2x65", "fit_tr 2x65", "advantage 2x65", "evaluate after it",
             "evaluate 1x17 again", "gnvp 1x17 again")
    for step, g_, w_ in zip(steps, got, want):
        print("%s %s: %s" % (r["layers"], step, "same bits" if same(g_, w_) else "DIFFERENT"))
    for step, g_, w_ in zip(steps, got, want):
        assert same(g_, w_), step
    assert got[3][2].accepted >= 0


# 7. repeatability on the forms without theta in LDS
@pytest.mark.parametrize("row", [0, 1, 2, 3])
def test_repeatable(row):
    cs = F.case(row, (2, 65), "sat")
    with baseline(cs, row) as b:
        r1 = b.fit_tr(cs["phi"], F.EPS, F.K, F.TH, F.LAM, 10, 0.015)
        r2 = b.fit_tr(cs["phi"], F.EPS, F.K, F.TH, F.LAM, 10, 0.015)
        h1, h2 = b.gnvp(cs["phi"], r1[1], F.LAM), b.gnvp(cs["phi"], r1[1], F.LAM)
    assert r1[0].tobytes() == r2[0].tobytes() and r1[1].tobytes() == r2[1].tobytes()
    assert bytes(r1[2]) == bytes(r2[2])
    assert h1.tobytes() == h2.tobytes()
    assert np.abs(r1[1]).max() > 0.0
