"""CPU check of the inputs and the reference of tests/test_gpu_act_edges.py (tests/act_edges.py,
tests/act_ref.py): every figure is printed before it is asserted.

  * each case that is held to the long-double forward pass is well conditioned: the oracle's float64 forward
    pass (libm tanh / exp, its own summation order) agrees with it to 1e-13 (1 + |mean|), a tenth of the bound the
    device is held to;
  * the sweep holds the points the activation tests rely on, and tanh64's formula evaluated in numpy float64
    without fma stays inside the bound of the device test, as does four times the logistic's own error;
  * the batch sizes do to the launch geometry what the GPU tests say they do.
"""
import numpy as np
import pytest

import act_edges as E
import act_ref as R
import oracle
import trained as T

ORACLE_TOL = 1e-13
TANH_TOL = 1.1e-15                       # twice the 5.4e-16 of tanh64's header (csrc/trpo_common.h)
CASES = E.reference_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_oracle_agrees_with_long_double(case):
    name, p, rows = case
    obs = p["obs"][rows]
    ref = R.forward_ld(p["layers"], p["ac"], p["theta"], obs)
    got = oracle.forward(p["layers"], p["ac"], p["theta"], obs)
    err = float((np.abs(got - ref) / (1 + np.abs(ref))).max())
    pre = T.preact(p["layers"], p["ac"], p["theta"], obs)
    print("act-edges %s: oracle against long double %.2e; max |x| per layer %s; max |mean| %.3g" % (
        name, err, " ".join("%.1f" % np.abs(x).max() for x in pre), float(np.abs(ref).max())))
    assert np.all(np.isfinite(got))
    assert err <= ORACLE_TOL


def test_saturating_settings_saturate():
    """A and B put pre-activations on both sides of tanh64's switch at 0.55, S drives the first hidden layer
    beyond its cutoff at 22; every bias and LogStd entry is live."""
    for k, (layers, ac) in enumerate(E.SAT_SHAPES):
        for s in "ABS":
            p = E.saturating(k, s)
            parts, logstd = T._split(layers, p["theta"])
            assert all(np.all(B != 0.0) for _, B in parts) and np.all(logstd != 0.0)
            assert np.all((logstd >= -1.0) & (logstd <= 0.3))
            x = np.abs(T.preact(layers, ac, p["theta"], p["obs"])[0])
            if s == "S":
                assert x.max() >= 40.0, (layers, x.max())
            else:
                assert (x < 0.55).any() and (x >= 0.55).any(), layers


def test_sweep_points():
    x = E.sweep_points()
    assert 69000 <= x.size <= 71000
    assert E.pinned(E.ACT_LAYERS, x.size, sample=False)
    assert x.size > E.GRID * E.LANE_ROWS                        # the lane form takes a second trip
    assert x.size > 17 * E.GRID * E.NEURON_ROWS                 # the neuron form an 18th
    h = (x.size - 1) // 2
    np.testing.assert_array_equal(x[h:2 * h], -x[:h])
    assert np.isnan(x[-1]) and not np.isnan(x[:-1]).any()
    for v in (np.nextafter(0.55, 0.0), 0.55, np.nextafter(0.55, 1.0), np.nextafter(22.0, 0.0), 22.0,
              np.nextafter(22.0, 23.0), 5e-324, 60.0, 700.0, 1e300, np.inf):
        assert (x == v).any() and (x == -v).any(), v
    zeros = x[x == 0.0]
    assert zeros.size == 2 and np.signbit(zeros).sum() == 1
    a = np.abs(x[:-1])
    assert ((a > 0) & (a < 0.55)).sum() >= 30000 and ((a >= 0.55) & (a <= 25)).sum() >= 30000
    assert (a < 1e-200).sum() >= 1000 and ((a > 1e-100) & (a < 1e-1)).sum() >= 1000
    th = E.activation_theta()
    assert th.size == 5 and np.signbit(th[[1, 3]]).all() and th[0] == th[2] == 1.0 and th[4] == 0.0
    with np.errstate(invalid="ignore"):
        y = x * 1.0 + -0.0                                      # what each of the two layers computes
    np.testing.assert_array_equal(y, x)
    np.testing.assert_array_equal(np.signbit(y), np.signbit(x))


def rel_err(y, ref, sel):
    ref = ref[sel]
    return float((np.abs(y[sel].astype(R.LD) - ref) / np.abs(ref)).max())


def test_formula_errors_against_long_double():
    """The figures the device bounds are made of, measured on the sweep's own points."""
    x = E.sweep_points()
    fin = np.isfinite(x) & (x != 0.0)
    e_tanh = rel_err(R.tanh64_np(x), R.tanh_ld(x), fin)
    small, big = fin & (np.abs(x) < 0.55), fin & (np.abs(x) >= 0.55)
    print("act-edges tanh64 formula in numpy float64, no fma, against long double: %.2e relative "
          "(polynomial branch %.2e, exponential branch %.2e)" % (
              e_tanh, rel_err(R.tanh64_np(x), R.tanh_ld(x), small), rel_err(R.tanh64_np(x), R.tanh_ld(x), big)))
    assert e_tanh <= TANH_TOL
    mid = np.abs(x) <= 700.0
    e_sig = rel_err(R.logistic_np(x), R.logistic_ld(x), mid)
    print("act-edges logistic in numpy float64 against long double over |x| <= 700: %.2e relative; "
          "device bound 4 x = %.2e" % (e_sig, 4 * e_sig))
    assert 0.0 < e_sig <= 4e-16                                 # libm's exp is within an ulp
    # the references themselves at the ends
    t, s = R.tanh_ld(x), R.logistic_ld(x)
    assert t[x == np.inf] == 1 and t[x == -np.inf] == -1 and np.isnan(t[-1])
    assert s[x == np.inf] == 1 and s[x == -np.inf] == 0
    assert np.all(np.abs(t[:-1]) <= 1) and np.all((s[:-1] >= 0) & (s[:-1] <= 1))


def test_long_double_is_extended():
    """The reference is only a reference where long double carries more than float64's 53 bits."""
    assert np.finfo(np.longdouble).nmant >= 63


def test_act_ld_is_act_with_another_mean():
    """act_ld shares Philox, the uniforms and logp with act(); on a small-argument policy, where the
    continued-fraction tanh is good, the two means agree, and a subset of samples gives the rows of the whole."""
    layers, ac = [15, 16, 16, 3], "lttl"
    rng = np.random.default_rng(3)
    from trpo_amd import synth
    th = synth.make_theta(layers) + 0.05 * rng.normal(size=synth.num_params(layers))
    obs = 0.5 * rng.normal(size=(40, 15))
    a = R.act(layers, ac, th, obs, 77, 5, row0=3, row_stride=7)
    b = R.act_ld(layers, ac, th, obs, 77, 5, row0=3, row_stride=7)
    assert np.abs(a[0] - b[0]).max() <= 1e-13
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[3], b[3])
    sub = np.array([0, 7, 39])
    c = R.act_ld(layers, ac, th, obs[sub], 77, 5, row0=3, row_stride=7, samples=sub)
    for whole, part in zip(b, c):
        np.testing.assert_array_equal(whole[sub], part)


def test_batch_sizes_meet_the_geometry():
    L = E.WRAP_SHAPE[0]
    wrap_n, wrap_l = E.GRID * E.NEURON_ROWS, E.GRID * E.LANE_ROWS
    assert E.pinned(L, 4101) and 4101 == wrap_n + 5             # trip 2: block 0 full, block 1 one live wave
    assert E.pinned(L, E.WRAP_SWITCH) and not E.pinned(L, E.WRAP_SWITCH + 1)
    assert E.WRAP_SWITCH > 2 * wrap_n
    assert not E.pinned(L, 65606) and 65606 == wrap_l + 70      # trip 2: 70 rows, six of them in block 1
    s = E.STRIDED
    last = s["row0"] + s["row_stride"] * (s["m"] - 1)
    assert s["m"] > wrap_n and E.pinned(L, s["m"]) and not E.pinned(L, last + 1) and last + 1 <= 65606
    assert E.HANDOFF_NS[0] == 4101 and E.HANDOFF_NS[1] // 2 > wrap_n
    for rows, period, m in ((E.near_rows(4101, wrap_n), wrap_n, 4101), (E.near_rows(65606, wrap_l), wrap_l, 65606)):
        assert rows[0] == 0 and rows[-1] == m - 1 and {period - 1, period, period + 1} <= set(rows.tolist())
        assert rows.size <= 4 * E.NEAR
    assert E.WIDE_SHAPES[1][0][2] == 130 and E.WIDE_SHAPES[1][0][-1] == 67
    for layers, _ in E.SAT_SHAPES + E.WIDE_SHAPES:
        assert E.neuron_lds_bytes(layers) <= E.NEURON_LDS and E.pinned(layers, 130)
    assert E.neuron_lds_bytes(E.LDS_SHAPES["fits"][0]) == 65344
    assert E.neuron_lds_bytes(E.LDS_SHAPES["over"][0]) == 65664 > E.NEURON_LDS
    # pinned, so the default rule would take the neuron form if the network fitted its LDS
    assert all(E.pinned(layers, E.LDS_M) for layers, _ in E.LDS_SHAPES.values())
