"""MI355X: the one-sample-per-lane kernels of the update path with their activation rows Y in GLOBAL SCRATCH.

A block of these kernels keeps `rows` rows of 65 doubles; up to 160 KB they live in LDS, beyond that in a global
scratch of rows x 65 x blocks doubles (csrc/trpo_update.hip and its sections: rows_plan).  Every other shape
of the suite that reaches these kernels through the baseline object fits LDS, so this file holds the shapes that
do not, small enough to take a second each: 130 samples are two full 64-sample passes and one of 2, three blocks.

  * the baseline object [12, 160, 1]: evaluate keeps 2 x 173 + 2 = 348 rows, the trust-region fit 3 x 173 + 2 = 521
    (the limit is 315), and nl = 3 keeps the lane form out.  The advantage stage's predict kernel needs 173 rows
    only, but follows the evaluate's choice: it runs in scratch too;
  * the policy [10, 112, 112, 3] under TRPO_UPDATE_GENERIC=1 and TRPO_SURR_GENERIC=1: the policy gradient keeps
    2 x 237 + 4 = 478 rows (scratch), the surrogate 237 (LDS); [10, 168, 168, 3] puts the surrogate's 349 rows in
    scratch as well.  Inference in the lane form keeps 237 rows on the first shape (LDS; its scratch case is
    tests/test_gpu_act_edges.py::test_network_beyond_the_neuron_forms_lds).

The row counts are computed from the layers below and asserted against the limit, so a later change of shapes
cannot move the cases back into LDS unnoticed.  References and bounds are those of the files that test the same
entry points in LDS: tests/test_gpu_baseline.py (1e-13, 1e-12, 1e-12), tests/test_gpu_advantage*.py (1e-12),
tests/test_gpu_vfit.py (1e-12, and its end-to-end bound), tests/test_gpu_update.py (the generic policy gradient,
1e-12), tests/test_gpu_surrogate.py (1e-12), tests/test_gpu_trust.py (1e-10 ref + 1e-14) and
tests/test_gpu_act_edges.py.  Every case prints what it measured before it asserts.
"""
import numpy as np
import pytest

import act_ref
import cases
import oracle
import ragged_ref
import test_gpu_act as GA
import test_gpu_act_edges as GE
import test_gpu_advantage as GADV
import test_gpu_advantage_ragged as GRAG
import test_gpu_trust as GT
import test_gpu_vfit as GV
import trpo_amd
from trpo_amd import synth

pytestmark = pytest.mark.gpu

LDS_ROWS = 160 * 1024 / (8 * 65)                 # rows of 65 doubles that fit the 160 KB of LDS: 315.08

BASE, BASE_AC = (12, 160, 1), "ltl"
NUM_EP, EP_LEN = 2, 65
N = NUM_EP * EP_LEN
RAGGED = (1, 64, 65)                             # 130 samples again; the last episode is the truncated one

POLICY, POLICY_WIDE, POLICY_AC = (10, 112, 112, 3), (10, 168, 168, 3), "lttl"
GENERIC = {"TRPO_UPDATE_GENERIC": "1", "TRPO_SURR_GENERIC": "1"}


def eval_rows(layers):
    return 2 * sum(layers) + 2


def fit_rows(layers):
    return 3 * sum(layers) + 2


def pg_rows(layers):
    return 2 * sum(layers) + layers[-1] + 1


def surr_rows(layers):
    return sum(layers)


def test_the_shapes_leave_lds():
    assert N == sum(RAGGED) == 130 and -(-N // 64) == 3
    assert eval_rows(BASE) == 348 > LDS_ROWS and fit_rows(BASE) == 521 > LDS_ROWS
    assert len(BASE) != 4                                       # the lane form does not apply
    assert pg_rows(POLICY) == 478 > LDS_ROWS
    assert surr_rows(POLICY) == 237 <= LDS_ROWS                 # this one stays: the wide shape below is its case
    assert surr_rows(POLICY_WIDE) == 349 > LDS_ROWS
    assert synth.num_params(list(POLICY_WIDE)) <= 32768         # both within the device CG's limit


# --- the baseline object ----------------------------------------------------------------------------------------
def padded(x):
    out = np.zeros((x.size + 15) // 16 * 16)
    out[:x.size] = x
    return out


def check_evaluate(tag, got, x, observ, target, num_ep, ep_len):
    f, g, pred = got
    fr, gr, pr = oracle.baseline_evaluate(list(BASE), BASE_AC, x, observ, target, num_ep, ep_len)
    print("scratch evaluate %s: f %.2e g %.2e predict %.2e" % (tag, abs(f - fr) / abs(fr), cases.rel_l2(g, gr),
                                                               cases.rel_l2(pred, pr)))
    assert abs(f - fr) <= 1e-13 * abs(fr)
    assert cases.rel_l2(g, gr) <= 1e-12
    assert cases.rel_l2(pred, pr) <= 1e-12


def test_evaluate():
    assert eval_rows(BASE) > LDS_ROWS
    c = GV.case(BASE, BASE_AC, NUM_EP, EP_LEN)
    x = padded(c["phi"])
    with trpo_amd.Baseline(list(BASE), BASE_AC) as b:
        b.set_data(c["observ"], c["y"], NUM_EP, EP_LEN)
        got = b.evaluate(x, want_predict=True)
        assert b.np == c["phi"].size
        np.testing.assert_array_equal(b.evaluate(x)[1], got[1])
    assert np.all(got[1][c["phi"].size:] == 0.0)
    check_evaluate("130", got, x, c["observ"], c["y"], NUM_EP, EP_LEN)


@pytest.mark.parametrize("gamma,lam", GADV.COEFFS)
def test_advantage(gamma, lam):
    assert eval_rows(BASE) > LDS_ROWS                           # the predict kernel follows the evaluate's choice
    x, observ, reward = GADV.inputs(NUM_EP, EP_LEN, BASE)
    ref = GADV.reference(NUM_EP, EP_LEN, gamma, lam, BASE, BASE_AC)
    with trpo_amd.Baseline(list(BASE), BASE_AC) as b:
        adv, ret, info = b.advantage(x, observ, reward, NUM_EP, EP_LEN, gamma, lam)
    GADV.check_against_reference(adv, ret, info, ref)


@pytest.mark.parametrize("gamma,lam", ragged_ref.COEFFS)
def test_advantage_ragged(gamma, lam):
    assert eval_rows(BASE) > LDS_ROWS
    horizon = max(RAGGED)
    ref = ragged_ref.reference(RAGGED, horizon, "last", gamma, lam, BASE, BASE_AC)
    assert ref["conditioning"] >= 0.05, "ill-conditioned case: change its seed"
    x, observ, reward, boot_observ = ragged_ref.inputs(RAGGED, BASE)
    flags = ragged_ref.boot_flags("last", len(RAGGED))
    np.testing.assert_array_equal(flags, [0, 0, 1])
    with trpo_amd.Baseline(list(BASE), BASE_AC) as b:
        adv, ret, info = b.advantage_ragged(x, observ, reward, RAGGED, horizon, gamma, lam, boot_observ=boot_observ,
                                            boot=flags)
    GRAG.check_against_reference(adv, ret, info, ref)


def test_gnvp_and_fit():
    assert fit_rows(BASE) > LDS_ROWS
    c, J = GV.case(BASE, BASE_AC, NUM_EP, EP_LEN), GV.jacobian(BASE, BASE_AC, NUM_EP, EP_LEN)
    P = J.shape[1]
    rng = np.random.default_rng(3)
    u, v = rng.normal(0.0, 1.0, P), rng.normal(0.0, 1.0, P)
    with GV.baseline(c) as b:
        Hv, Hu = b.gnvp(c["phi"], v, GV.LAM), b.gnvp(c["phi"], u, GV.LAM)
        err = max(GV.rel_l2(Hv, J.T @ (J @ v) / N + GV.LAM * v), GV.rel_l2(Hu, J.T @ (J @ u) / N + GV.LAM * u))
        print("scratch gnvp %s N=%d: relL2 %.3e" % (BASE, N, err))
        assert err <= GV.TOL
        assert abs(u @ Hv - v @ Hu) <= 2 * GV.TOL * max(np.linalg.norm(u) * np.linalg.norm(Hv),
                                                        np.linalg.norm(v) * np.linalg.norm(Hu))
        GV.compare(b, c)


def test_one_object_through_every_layout_of_its_pinned_buffer():
    """set_data(130), evaluate, advantage, evaluate, fit_tr, set_data(66), evaluate, set_data(130), evaluate on
    one object: the evaluate, the advantage stage and the fit share (or sit beside) one pinned buffer that grows,
    is zero-filled when it does, and whose flag words move with the batch.  Every evaluate has the bits of a
    fresh object's on the same data."""
    big, small = GV.case(BASE, BASE_AC, NUM_EP, EP_LEN), GV.case(BASE, BASE_AC, 2, 33)
    x = padded(big["phi"])
    xa, observ, reward = GADV.inputs(NUM_EP, EP_LEN, BASE)
    got, data = [], []
    with trpo_amd.Baseline(list(BASE), BASE_AC) as b:
        def evaluate(observ_, target_, num_ep, ep_len):
            got.append(b.evaluate(x, want_predict=True))
            data.append((observ_, target_, num_ep, ep_len))

        b.set_data(big["observ"], big["y"], NUM_EP, EP_LEN)
        evaluate(big["observ"], big["y"], NUM_EP, EP_LEN)
        _, ret, _ = b.advantage(xa, observ, reward, NUM_EP, EP_LEN)
        evaluate(observ, ret, NUM_EP, EP_LEN)                    # the object now holds (observ, ret)
        assert b.fit_tr(xa, GV.EPS, GV.K, GV.TH, GV.LAM, 10, 0.015)[2].evaluated >= 1
        b.set_data(small["observ"], small["y"], 2, 33)
        evaluate(small["observ"], small["y"], 2, 33)
        b.set_data(big["observ"], big["y"], NUM_EP, EP_LEN)
        evaluate(big["observ"], big["y"], NUM_EP, EP_LEN)
    assert len(got) == 4
    for k, (r, d) in enumerate(zip(got, data)):
        with trpo_amd.Baseline(list(BASE), BASE_AC) as fresh:
            fresh.set_data(*d)
            e = fresh.evaluate(x, want_predict=True)
        assert r[0] == e[0], k
        np.testing.assert_array_equal(r[1], e[1], err_msg="evaluate %d" % k)
        np.testing.assert_array_equal(r[2], e[2], err_msg="evaluate %d" % k)
    check_evaluate("after the advantage stage", got[1], x, *data[1])
    check_evaluate("66", got[2], x, *data[2])


# --- the policy side --------------------------------------------------------------------------------------------
def generic(monkeypatch):
    for k, v in GENERIC.items():
        monkeypatch.setenv(k, v)


def check_surrogates(tag, L, ctx, problem):
    th, obs, std, mean, action, adv, fs, kl_ref = problem
    s, kl = ctx.surrogate_kl(fs, 0, 3)
    plain = ctx.surrogate(fs, 0, 3)
    ref = np.array([oracle.surrogate_sum(list(L), POLICY_AC, th + 0.5 ** k * fs, obs, mean, action, adv, std)
                    for k in range(3)])
    print("scratch surrogate %s: worst |dev - ref| / max|ref| = %.3e" % (
        tag, np.abs(plain - ref).max() / np.abs(ref).max()))
    np.testing.assert_allclose(plain, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
    np.testing.assert_array_equal(s, plain)                     # the surrogate's own bits
    GT._check("scratch %s" % tag, kl, kl_ref[:3])
    np.testing.assert_array_equal(ctx.surrogate_kl(fs, 0, 3)[1], kl)


def test_policy_gradient_and_surrogates(monkeypatch):
    assert pg_rows(POLICY) > LDS_ROWS >= surr_rows(POLICY)
    generic(monkeypatch)
    problem = GT._problem(POLICY, POLICY_AC, N)
    th, obs, std, mean, action, adv, fs, _ = problem
    b_ref, _ = oracle.policy_grad(list(POLICY), POLICY_AC, th, obs, mean, action, adv)
    with GT._ctx(list(POLICY), POLICY_AC, th, obs, std, mean, action, adv) as ctx:
        r = ctx.update()
        print("scratch policy gradient %s n=%d: relL2 %.3e" % (POLICY, N, cases.rel_l2(r["b"], b_ref)))
        assert cases.rel_l2(r["b"], b_ref) <= 1e-12
        np.testing.assert_array_equal(ctx.update()["b"], r["b"])
        check_surrogates("%s n=%d" % (POLICY, N), POLICY, ctx, problem)


def test_surrogates_of_the_wide_policy(monkeypatch):
    assert surr_rows(POLICY_WIDE) > LDS_ROWS
    generic(monkeypatch)
    problem = GT._problem(POLICY_WIDE, POLICY_AC, N)
    th, obs, std, mean, action, adv, _, _ = problem
    with GT._ctx(list(POLICY_WIDE), POLICY_AC, th, obs, std, mean, action, adv) as ctx:
        check_surrogates("%s n=%d" % (POLICY_WIDE, N), POLICY_WIDE, ctx, problem)


def test_act_in_the_lane_form():
    L = list(POLICY)
    rng = np.random.default_rng(100)
    th = synth.make_theta(L) + 0.05 * rng.normal(size=synth.num_params(L))
    th[-L[-1]:] = rng.uniform(-1.0, 0.5, L[-1])
    p = dict(layers=L, ac=POLICY_AC, theta=th, obs=0.5 * rng.normal(size=(N, L[0])))
    ref = act_ref.act_ld(L, POLICY_AC, th, p["obs"], GA.SEED, GA.STEP)
    with GE.ctx_for(p, "lane") as ctx:
        out = ctx.act(p["obs"], GA.SEED, GA.STEP)
        GA.same_bits(ctx.act(p["obs"][:65], GA.SEED, GA.STEP), GE.take(out, slice(0, 65)))
    GE.check("scratch-shapes lane %s" % (POLICY,), p, out, ref)
