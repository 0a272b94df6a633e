"""MI355X: device policy inference (trpo_ctx_act) where its grids wrap, its layers widen and its nets saturate.

tests/test_gpu_act.py keeps to m <= 130 (one case at exactly 1024 lane passes), widths <= 64, A <= 17 and small
arguments.  Here (inputs: tests/act_edges.py, checked on the CPU by tests/test_act_inputs.py):

  1. tanh64 and the fp64 logistic themselves, through a [1,1,1] policy that hands obs to the activation unchanged,
     on 70 031 points in one pinned call: the lane form takes a second grid trip, the neuron form eighteen;
  2. biased policies under the settings A, B and S of tests/trained.py (S saturates the first hidden layer);
  3. batches beyond 4096 rows (the neuron form wraps) and beyond 65 536 (the lane form wraps), on the pinned and
     on the staged path, across the switch between them, strided, and handed to update();
  4. a layer of 128 and one of 130 outputs, 17 and 67 actions;
  5. the largest network the neuron form's LDS holds, and the refusal of the next one.

The reference is the long-double forward pass of tests/act_ref.py (act_ld); Philox, the uniforms and logp are
those of tests/test_gpu_act.py, and so are the bounds: mean 1e-12 (1 + |mean|), action against
mean_dev + exp(LogStd) z_ref 1e-13 (1 + |action|), logp 1e-12 (1 + |logp|).  tanh64 is held to 1.1e-15 relative,
twice the 5.4e-16 its header (csrc/trpo_common.h) states for the fit, the factor covering the device exp and the
division of the upper branch; the logistic to four times the error the same expression has in numpy float64
on the same points (measured here before it is used, 2.2e-16), the margin being a device exp of one ulp against
libm's half.  Everything called "the same bits" is assert_array_equal.  Every case prints what it measured
before it asserts.
"""
import functools

import numpy as np
import pytest

import act_edges as E
import act_ref as R
import test_gpu_act as G
import trpo_amd
from trpo_amd import synth

pytestmark = pytest.mark.gpu

SEED, STEP = G.SEED, G.STEP
FORMS = ("lane", "neuron", None)
TANH_TOL = 1.1e-15
MEAN_TOL, ACTION_TOL, LOGP_TOL = 1e-12, 1e-13, 1e-12


def ctx_for(p, form=None, obs=None, precision=None):
    return G.context((p["layers"], p["ac"]), p["obs"][:1] if obs is None else obs, form, precision, theta=p["theta"])


_REFERENCE = {}


def reference(name, p, rows, row0=0, stride=1):
    """act_ld on the samples rows of p at (SEED, STEP), computed once per name and left unchanged."""
    if name not in _REFERENCE:
        ref = R.act_ld(p["layers"], p["ac"], p["theta"], p["obs"][rows], SEED, STEP, row0, stride, samples=rows)
        for a in ref:
            a.setflags(write=False)
        _REFERENCE[name] = ref
    return _REFERENCE[name]


def check(tag, p, out, ref):
    """out = (mean, action, logp) of the samples the reference was taken on."""
    mean, action, logp = out
    rmean, _, rlogp, rz = ref
    A = p["layers"][-1]
    want = mean + np.exp(p["theta"][-A:]) * rz
    e_mean = float((np.abs(mean - rmean) / (1.0 + np.abs(rmean))).max())
    e_act = float((np.abs(action - want) / (1.0 + np.abs(want))).max())
    e_lp = float((np.abs(logp - rlogp) / (1.0 + np.abs(rlogp))).max())
    print("act-edges %s rows=%d: mean %.2e action %.2e logp %.2e" % (tag, mean.shape[0], e_mean, e_act, e_lp))
    assert all(np.all(np.isfinite(a)) for a in out)
    assert e_mean <= MEAN_TOL
    assert e_act <= ACTION_TOL
    assert e_lp <= LOGP_TOL


def take(out, rows):
    return [a[rows] for a in out]


# --- 1. the activations themselves ---------------------------------------------------------------------------
def _activation(ac):
    x = E.sweep_points()
    p = dict(layers=E.ACT_LAYERS, ac=ac, theta=E.activation_theta(), obs=x.reshape(-1, 1))
    got = {}
    for form in ("lane", "neuron"):
        with ctx_for(p, form) as ctx:
            mean, action, logp = ctx.act(p["obs"], SEED, STEP, sample=False)
            assert action is None and logp is None
            got[form] = mean.reshape(-1)
            np.testing.assert_array_equal(ctx.act(p["obs"][:9], SEED, STEP, sample=False)[0].reshape(-1),
                                          got[form][:9])
    np.testing.assert_array_equal(got["lane"], got["neuron"])
    return x, got["lane"]


def _rel(y, ref, sel):
    return np.abs(y[sel].astype(R.LD) - ref[sel]) / np.abs(ref[sel])


def test_tanh64_on_the_sweep():
    x, y = _activation("llt")
    ref = R.tanh_ld(x)
    sel = np.isfinite(x) & (x != 0.0)
    err = _rel(y, ref, sel)
    worst = x[sel][int(np.argmax(err))]
    lo = sel & (np.abs(x) < 0.55)
    print("act-edges tanh64: worst relative error %.2e at x = %r (polynomial branch %.2e, exponential branch "
          "%.2e); bound %.1e" % (float(err.max()), float(worst), float(_rel(y, ref, lo).max()),
                                 float(_rel(y, ref, sel & ~lo).max()), TANH_TOL))
    assert float(err.max()) <= TANH_TOL
    h = (x.size - 1) // 2
    np.testing.assert_array_equal(y[h:2 * h], -y[:h])                     # odd, bit for bit
    np.testing.assert_array_equal(np.signbit(y[:-1]), np.signbit(x[:-1]))  # the zeros keep their signs
    assert np.all(y[x == 0.0] == 0.0)
    assert np.all(np.abs(y[:-1]) <= 1.0)
    assert y[x == np.inf] == 1.0 and y[x == -np.inf] == -1.0
    assert np.isnan(y[-1]) and not np.isnan(y[:-1]).any()
    # a denormal and the smallest arguments come back as they are: tanh x = x (1 - x^2 / 3 ...)
    tiny = np.abs(x) < 1e-9
    np.testing.assert_array_equal(y[tiny], x[tiny])


def test_logistic_on_the_sweep():
    x, y = _activation("lls")
    ref = R.logistic_ld(x)
    mid = np.abs(x) <= 700.0
    e_np = float(_rel(R.logistic_np(x), ref, mid).max())
    err = _rel(y, ref, mid)
    print("act-edges logistic: worst relative error %.2e at x = %r over |x| <= 700; numpy float64 %.2e, bound "
          "4 x = %.2e" % (float(err.max()), float(x[mid][int(np.argmax(err))]), e_np, 4 * e_np))
    assert float(err.max()) <= 4 * e_np
    out = ~mid[:-1]
    assert np.all(np.isfinite(y[:-1][out])) and np.all((y[:-1][out] >= 0.0) & (y[:-1][out] <= 1.0))
    assert np.all((y[:-1] >= 0.0) & (y[:-1] <= 1.0))
    assert y[x == np.inf] == 1.0 and y[x == -np.inf] == 0.0
    assert y[x == 1e300] == 1.0 and y[x == -1e300] == 0.0
    assert np.all(y[x == 0.0] == 0.5)
    assert np.isnan(y[-1])


# --- 2. saturating, biased policies ---------------------------------------------------------------------------
@pytest.mark.parametrize("setting", "ABS")
@pytest.mark.parametrize("k", range(len(E.SAT_SHAPES)), ids=[E.shape_id(s) for s in E.SAT_SHAPES])
def test_saturating_policies(k, setting):
    p = E.saturating(k, setting)
    tag = "sat-%s-%s" % (E.shape_id(E.SAT_SHAPES[k]), setting)
    ref = reference(tag, p, np.arange(E.SAT_M))
    got = {}
    for form in FORMS:
        with ctx_for(p, form) as ctx:
            got[form] = ctx.act(p["obs"], SEED, STEP)
        check("%s %s" % (tag, form or "default"), p, got[form], ref)     # finite too, under S like the others
    G.same_bits(got["lane"], got["neuron"])
    G.same_bits(got["lane"], got[None])


# --- 3. grids that wrap, on both transfer paths -----------------------------------------------------------------
WRAP_N, WRAP_L = E.GRID * E.NEURON_ROWS, E.GRID * E.LANE_ROWS


@functools.lru_cache(maxsize=None)
def wrapped(m, form):
    """One call of m rows of the shared batch, kept for the tests that compare results with each other."""
    p = E.wrap_problem(m)
    with ctx_for(p, form) as ctx:
        out = ctx.act(p["obs"], SEED, STEP)
    for a in out:
        a.setflags(write=False)
    return out


def check_wrapped(tag, m, out, period):
    p = E.wrap_problem(m)
    rows = E.near_rows(m, period)
    check(tag, p, take(out, rows), reference("wrap-%d-%d" % (m, period), p, rows))


def test_neuron_form_second_trip_pinned():
    """m = 4101: on the second trip block 0 holds four rows, block 1 one live wave and three dead ones."""
    out = wrapped(4101, "neuron")
    check_wrapped("wrap m=4101 neuron pinned", 4101, out, WRAP_N)
    G.same_bits(out, take(wrapped(E.WRAP_SWITCH, None), slice(0, 4101)))
    # the same batch one row shorter and three rows shorter: other tails of the second trip
    for m in (4100, 4098):
        G.same_bits(wrapped(m, "neuron"), take(out, slice(0, m)))


def test_across_the_switch_between_the_paths():
    """m = 11 915 is pinned (neuron form, third trip), m = 11 916 staged (lane form): the rows they share have
    the same bits; forced neuron on the staged batch (no flag words) equals the default rule's result."""
    m = E.WRAP_SWITCH
    last, first = wrapped(m, None), wrapped(m + 1, None)
    check_wrapped("wrap m=%d default pinned" % m, m, last, WRAP_N)
    check_wrapped("wrap m=%d default staged" % (m + 1), m + 1, first, WRAP_N)
    G.same_bits(last, take(first, slice(0, m)))
    staged_neuron = wrapped(m + 1, "neuron")
    check_wrapped("wrap m=%d neuron staged" % (m + 1), m + 1, staged_neuron, WRAP_N)
    G.same_bits(staged_neuron, first)
    # the lane form on the pinned batch, and every row of it, not only those near a wrap
    G.same_bits(wrapped(m, "lane"), last)


def test_lane_form_second_trip():
    """m = 65 606, default rule: staged lane form, a second trip of 70 rows, six of them in block 1."""
    m = 65606
    out = wrapped(m, None)
    check_wrapped("wrap m=65606 default staged", m, out, WRAP_L)
    G.same_bits(take(out, slice(0, E.WRAP_SWITCH + 1)), wrapped(E.WRAP_SWITCH + 1, None))
    # the neuron form reaches its 17th trip on the same batch; a batch is a prefix of a longer one
    G.same_bits(wrapped(m, "neuron"), out)


def test_strided_call_after_a_wrap():
    """row0 = 3, row_stride = 7, m = 4101 under forced neuron (pinned, wrapped): the bits of rows 3, 10, ... of a
    contiguous call over rows 0 .. 28 703 (staged, seven trips), and the reference's on the rows near the wrap."""
    s = E.STRIDED
    rows = s["row0"] + s["row_stride"] * np.arange(s["m"])
    big = E.wrap_problem(int(rows[-1]) + 1)
    p = dict(big, obs=big["obs"][rows])
    with ctx_for(big, "neuron") as ctx:
        strided = ctx.act(p["obs"], SEED, STEP, row0=s["row0"], row_stride=s["row_stride"])
        whole = ctx.act(big["obs"], SEED, STEP)
    near = E.near_rows(s["m"], WRAP_N)
    check("wrap strided m=4101 neuron", p, take(strided, near),
          reference("wrap-strided", p, near, s["row0"], s["row_stride"]))
    G.same_bits(strided, take(whole, rows))
    G.same_bits(whole, take(wrapped(65606, None), slice(0, rows[-1] + 1)))


@pytest.mark.parametrize("n", E.HANDOFF_NS)
def test_hand_off_after_a_wrap(n):
    """act(keep) in keep_all's two strided calls under forced neuron, set_rollout_acted, update == set_rollout
    with what the host received, update on a fresh context, bit for bit.  n = 4101: calls of 2050 and 2051 rows
    whose kept rows reach beyond 4096; n = 8197: 4098 and 4099 rows, each call wraps."""
    p = E.wrap_problem(n)
    adv = synth.normal(synth.SEED, synth.STREAM_ADV, n)
    with ctx_for(p, "neuron", obs=p["obs"]) as ctx:
        mean, action = G.keep_all(ctx, p["obs"])
        ctx.set_rollout_acted(adv)
        r = ctx.update()
    G.same_bits((mean, action), take(wrapped(65606, None), slice(0, n))[:2])
    with ctx_for(p, obs=p["obs"]) as fresh:
        fresh.set_rollout(mean, action, adv)
        s = fresh.update()
    G.assert_same_update(r, s)


# --- 4. wide layers and many actions ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(E.WIDE_SHAPES)), ids=[E.shape_id(s) for s in E.WIDE_SHAPES])
def test_wide_layers_and_many_actions(k):
    """m = 1, 5 and 130 in the three forms.  376x128x64x17, the reference project's Humanoid policy, has 57 634
    parameters, more than the device CG's 32 768: its context serves inference only (the test below);
    180x128x64x17 (32 546) is the widest input of the same hidden layers that the solver takes as well."""
    p = E.wide(k)
    tag = "wide-%s" % E.shape_id(E.WIDE_SHAPES[k])
    ref = reference(tag, p, np.arange(max(E.WIDE_MS)))
    got = {}
    for form in FORMS:
        with ctx_for(p, form) as ctx:
            for m in E.WIDE_MS:
                got[form, m] = ctx.act(p["obs"][:m], SEED, STEP)
                check("%s %s" % (tag, form or "default"), p, got[form, m], take(ref, slice(0, m)))
    for m in E.WIDE_MS:
        G.same_bits(got["lane", m], got["neuron", m])
        G.same_bits(got["lane", m], got[None, m])
        G.same_bits(got["lane", m], take(got["neuron", max(E.WIDE_MS)], slice(0, m)))


def test_policy_beyond_the_solver_serves_inference_only():
    """376x128x64x17: the context exists, every call that would run the FVP, the CG, the update path, a timer
    or attach a collective is refused with TRPO_E_INVALID and says why, and inference goes on as before."""
    p = E.wide(0)
    P, A, n = p["theta"].size, p["layers"][-1], 16
    assert P == 57634
    obs = p["obs"][:n]
    v, adv = np.ones(P), np.ones(n)
    L = trpo_amd.lib()
    with ctx_for(p, obs=obs) as ctx, trpo_amd.Baseline([16, 16, 16, 1], "lttl") as bl, trpo_amd.Group(1) as grp:
        before = ctx.act(obs, SEED, STEP, keep=True)
        for call in (lambda: ctx.fvp(v), lambda: ctx.cg(v), lambda: ctx.set_rollout(before[0], before[1], adv),
                     lambda: ctx.set_rollout_from(bl, before[0], before[1]), lambda: ctx.set_rollout_acted(adv),
                     lambda: ctx.update(), lambda: ctx.update(kl_cap=1.0), lambda: ctx.surrogate(v),
                     lambda: ctx.surrogate_kl(v), lambda: ctx.attach_comm(0, 1, b"\0" * 128),
                     lambda: ctx.attach_group(grp, 0), lambda: ctx.peer_handle()):
            with pytest.raises(trpo_amd.TRPOError) as e:
                call()
            assert "inference only" in str(e.value) and "57634" in str(e.value), str(e.value)
        ctx.upload_v(v)
        assert L.trpo_ctx_enqueue_fvp(ctx._h) == -1 and L.trpo_ctx_enqueue_cg(ctx._h, 10, 0.0) == -1
        assert L.trpo_ctx_enqueue_fvp_kernel_only(ctx._h) == -1 and L.trpo_ctx_time(ctx._h, 0, 1, 10, 0.0) == -1.0
        ctx.set_theta(p["theta"])
        ctx.set_obs(obs)
        G.same_bits(ctx.act(obs, SEED, STEP), before)


# --- 5. the neuron form's LDS limit ----------------------------------------------------------------------------
def test_largest_network_of_the_neuron_form():
    """[2030,8,2]: 4 x 2042 doubles are 65 344 B; the input loop takes 32 trips per lane."""
    p = E.lds_problem("fits")
    ref = reference("lds-fits", p, np.arange(E.LDS_M))
    got = {}
    for form in FORMS:
        with ctx_for(p, form) as ctx:
            got[form] = ctx.act(p["obs"], SEED, STEP)
            G.same_bits(ctx.act(p["obs"][:5], SEED, STEP), take(got[form], slice(0, 5)))
        check("lds-fits %s" % (form or "default"), p, got[form], ref)
    G.same_bits(got["neuron"], got["lane"])
    G.same_bits(got[None], got["lane"])


def test_network_beyond_the_neuron_forms_lds():
    """[2040,8,2] needs 65 664 B: forced neuron is refused and names the LDS, nothing else is disturbed, and
    the default rule runs the pinned batch in the lane form (scratch rows)."""
    p = E.lds_problem("over")
    ref = reference("lds-over", p, np.arange(E.LDS_M))
    with ctx_for(p, "neuron") as ctx:
        for kw in (dict(), dict(sample=False)):
            with pytest.raises(trpo_amd.TRPOError) as e:
                ctx.act(p["obs"], SEED, STEP, **kw)
            assert e.value.code == G.TRPO_E_INVALID
            assert "LDS" in str(e.value) and "LDS" in trpo_amd.last_error()
    with ctx_for(p) as ctx:
        default = ctx.act(p["obs"], SEED, STEP)
        G.same_bits(ctx.act(p["obs"][:5], SEED, STEP), take(default, slice(0, 5)))
    check("lds-over default", p, default, ref)
    with ctx_for(p, "lane") as ctx:
        G.same_bits(ctx.act(p["obs"], SEED, STEP), default)
