"""CPU check of tests/trained.py: the biased, saturating inputs do what tests/test_gpu_trained_policy.py
assumes, the numpy emulation is the oracle's FVP, and the gates admit the comparisons that file relies on.

Per case of the table (each row under settings A and B, one row per family under S), printed before it is
asserted:
  * every bias and LogStd entry is non-zero;
  * A, B: every tanh / sigmoid layer has >= 25 % of its pre-activations at |x| >= 0.625 (tanh_fast's
    exponential branch) and >= 5 % below it.  One exception, by arithmetic and not by measurement: a layer
    behind a 0.1 x layer.  Under A its inputs are |0.1 x| <= 0.4, its weights 1.5 N(0, 1 / fan_in) and its
    biases within 0.5, so its pre-activations have a standard deviation near 0.4 and 25 % of them cannot pass
    0.625 ([16,16,16,4] 'lots': 2 % and 20 %).  Such a layer must still have pre-activations on both sides
    under A and meets the full condition under B;
  * S: the first hidden layer reaches |x| >= 40;
  * fvp_np(float64) within 1e-12 of oracle.fvp (the helper is the oracle's product) and fvp_np(float32) within
    1e-6: plain float32 with tanh_fast's formula is ten times inside the fp32 FVP bound of 1e-5, so a device
    miss of that bound is not the number format's.
The fp64 CG gate leaves at most 2 rows of the table outside, and every family has a case on which the fp32 CG
and the update are compared.
"""
import numpy as np
import pytest

import trained as T


def _behind_tenth(ac, i):
    """Whether layer i + 1's input has passed a 0.1 x layer."""
    return "o" in ac[1:i + 1]


@pytest.mark.parametrize("c", T.cases(), ids=T.case_id)
def test_inputs_populate_both_branches_and_emulation_matches_oracle(c):
    row, setting = c
    p = T.problem(row, setting)
    L, ac, th = p["layers"], p["ac"], p["theta"]
    parts, logstd = T._split(L, th)
    assert all(np.all(B != 0.0) for _, B in parts) and np.all(logstd != 0.0)
    np.testing.assert_array_equal(p["std"], np.exp(logstd))
    pre = T.preact(L, ac, th, p["obs"])
    share = [float(np.mean(np.abs(x) >= T.BRANCH)) for x in pre]
    peak = [float(np.abs(x).max()) for x in pre]
    g = T.gates(row, setting)
    e64 = T.rel_l2(T.fvp_np(L, ac, th, p["obs"], p["std"], p["v"], np.float64), g["zr"])
    e32 = T.rel_l2(T.fvp_np(L, ac, th, p["obs"], p["std"], p["v"], np.float32), g["zr"])
    print("trained %s: max|x| / share >= 0.625 per layer %s; emulation FVP fp64 %.1e fp32 %.1e; CG sens64 %.1e "
          "cg32 %.1e upd32 %.1e margin %s" % (
              T.case_id(c), " ".join("%s %.1f / %.0f%%" % (ac[i + 1], peak[i], 100 * share[i])
                                     for i in range(len(pre))),
              e64, e32, g["sens64"], g["cg32"], g["upd32"], g["margin"]))
    for i, s in enumerate(share):
        if ac[i + 1] not in "ts":
            continue
        if setting == "S":
            continue
        if setting == "A" and _behind_tenth(ac, i):
            assert 0.0 < s < 1.0, (i, s)
        else:
            assert s >= 0.25 and 1.0 - s >= 0.05, (i, s)
    if setting == "S":
        assert peak[0] >= 40.0, peak
    assert e64 <= 1e-12, e64
    assert e32 <= 1e-6, e32


def test_tanh_fast_emulation_is_tanh_on_both_branches():
    """The numpy copy of tanh_fast against float64 tanh: the kernel comment's 1.5e-7 relative plus the copy's
    unfused products, exactly +-1 in saturation and no overflow to NaN where exp2 does."""
    x = np.concatenate([np.linspace(-0.62499, 0.62499, 4001), np.linspace(0.625, 20.0, 4001),
                        -np.linspace(0.625, 20.0, 4001)]).astype(np.float32)
    y = T.tanh_fast_np(x)
    ref = np.tanh(x.astype(np.float64))
    nz = ref != 0.0
    assert np.max(np.abs(y[nz] - ref[nz]) / np.abs(ref[nz])) <= 4e-7
    big = np.array([10.0, 44.0, 64.0, 89.0, 1e4, 3e38], np.float32)
    np.testing.assert_array_equal(T.tanh_fast_np(big), np.ones(6, np.float32))
    np.testing.assert_array_equal(T.tanh_fast_np(-big), -np.ones(6, np.float32))


def test_gates_admit_what_the_gpu_test_relies_on():
    assert set(T.RELY_CG32) == set(T.RELY_UPDATE) == set(T.FAMILIES)
    for fam in T.FAMILIES:
        assert T.RELY_CG32[fam] and T.RELY_UPDATE[fam], fam
        for c in T.RELY_CG32[fam]:
            assert T.ROWS[c[0]]["family"] == fam and c in T.cases()
            assert T.gates(*c)["cmp32"], (T.case_id(c), T.gates(*c)["cg32"])
        for c in T.RELY_UPDATE[fam]:
            assert T.ROWS[c[0]]["family"] == fam and c in T.cases()
            g = T.gates(*c)
            assert g["cmp_upd"], (T.case_id(c), g["cg32"], g["upd32"], g["margin"])
    # fp64 mode: at most 2 rows of the table have a case outside the gate
    outside = {c[0] for c in T.cases() if not T.gates(*c)["cmp64"]}
    print("trained: rows outside the fp64 CG gate: %s" % sorted(T.case_id((r, "*")) for r in outside))
    assert len(outside) <= 2, outside


def test_decision_margin_refuses_a_close_call():
    ok = dict(evaluated=2, accepted=1, actual=[-0.1, 0.5], expected=[1.0, 0.5], ratio=[-0.1, 1.0])
    assert T.decision_margin(ok)
    close = dict(ok, ratio=[0.09995, 1.0], actual=[0.09995, 0.5])
    assert not T.decision_margin(close)
    barely = dict(evaluated=1, accepted=0, actual=[0.10005], expected=[1.0], ratio=[0.10005])
    assert not T.decision_margin(barely)
