"""MI355X: every FVP kernel family on biased, saturating policies (tests/trained.py) against the oracle.

The synthetic inputs and the goldens have zero biases, a zero LogStd and hidden pre-activations below 0.6, so
they never enter the exponential branch of the tile kernels' tanh_fast (|x| >= 0.625) and never put a live
value into a bias slot of the packed layouts.  Here each row of trained.ROWS runs at N = 777 (49 tiles, the
last with 9 live rows) under settings A and B, and one row per family under the saturating setting S; the
kernel name is asserted, so a dispatch change cannot move a case to another kernel unnoticed.

Per case, with the bounds the suite already holds the same quantities to:
  * fvp(v) twice (the first call writes the forward cache, the second reads it): identical bits, relative
    L2 <= 1e-5 against oracle.fvp; under S also finite, the LogStd block exactly (2 + lambda) v;
  * the policy gradient of update(): <= 2e-6 against oracle.policy_grad;
  * surrogate sums and mean KL of the candidates theta + 0.5^k fs, k = 0 .. 3: tests/test_gpu_surrogate.py's
    1e-12 and tests/test_gpu_trust.py's 1e-10 ref + 1e-14, on the form the shape takes by default and, where
    that is the fp64 MFMA kernel, also on the register / one-lane form (TRPO_SURR_GENERIC=1);
  * precision="fp64": FVP <= 1e-12 -- the check that does not depend on the number format (bias placement in
    the fp64 pack, the cooperative fp64 kernel, the generic fp64 instantiation).
CG and the update are compared only where that is well posed (trained.gates, asserted on the CPU by
tests/test_trained_inputs.py): the fp64 solve at max(1e-9, 100 x the oracle's own sensitivity to its row
order) where that sensitivity is <= 1e-6; the fp32 solve at 1e-4 where plain float64 CG on the float32
emulation lands within 1e-5 of the oracle; the update (accepted, x and theta - theta0 at 1e-4, also when
the stall guard re-solved it in fp64, as in tests/test_gpu_random_shapes.py) where that holds for its own
right-hand side too and the oracle's line search decided with a relative margin of 1e-3.
Every case prints the figures it measured before it asserts them.
"""
import numpy as np
import pytest

import oracle
import trained as T
import trpo_amd

pytestmark = pytest.mark.gpu

LAM = 0.1
FVP_TOL, FVP64_TOL, GRAD_TOL, CG_TOL = 1e-5, 1e-12, 2e-6, 1e-4
SURR_TOL = 1e-12                       # tests/test_gpu_surrogate.py
KL_RTOL, KL_ATOL = 1e-10, 1e-14        # tests/test_gpu_trust.py
NK = 4


def _check_name(r, name):
    assert all(s in name for s in r["has"]), name
    assert not any(s in name for s in r["lacks"]), name
    assert r["ends"] is None or name.endswith(r["ends"]), name


def _line_search_refs(p):
    L, ac = p["layers"], p["ac"]
    surr, kl = [], []
    for k in range(NK):
        th_k = p["theta"] + 0.5 ** k * p["fs"]
        surr.append(oracle.surrogate_sum(L, ac, th_k, p["obs"], p["mean"], p["action"], p["adv"], p["std"]))
        kl.append(T.kl_closed_form(L, ac, th_k, p["obs"], p["mean"], p["std"]))
    return np.array(surr), np.array(kl)


def _check_line_search(tag, ctx, p, sref, klref):
    s = ctx.surrogate(p["fs"], 0, NK)
    s2, kl = ctx.surrogate_kl(p["fs"], 0, NK)
    sig, smp = klref[:, 0], klref[:, 1]
    err_s = np.abs((kl - sig) - smp)
    err = np.abs(kl - (sig + smp))
    print("trained %s: surrogate worst rel %.2e; KL sample term worst %.2e of ref, KL worst %.2e of ref" % (
        tag, float(np.max(np.abs(s - sref)) / np.abs(sref).max()), float(np.max(err_s / smp)),
        float(np.max(err / (sig + smp)))))
    np.testing.assert_array_equal(s, s2)
    np.testing.assert_allclose(s, sref, rtol=SURR_TOL, atol=SURR_TOL * np.abs(sref).max())
    assert np.all(err_s <= KL_RTOL * smp + KL_ATOL), (tag, kl - sig, smp)
    assert np.all(err <= KL_RTOL * (sig + smp) + KL_ATOL), (tag, kl, sig + smp)


@pytest.mark.parametrize("c", T.cases(), ids=T.case_id)
def test_trained_policy(c, monkeypatch):
    row, setting = c
    r = T.ROWS[row]
    p, g = T.problem(row, setting), T.gates(row, setting)
    L, ac, th, obs, std, v, b = p["layers"], p["ac"], p["theta"], p["obs"], p["std"], p["v"], p["b"]
    A = L[-1]
    tag = T.case_id(c)
    for k, val in r["env"].items():
        monkeypatch.setenv(k, val)
    sref, klref = _line_search_refs(p)
    ref = g["upd"]
    with trpo_amd.Context(L, ac, th, obs, std, LAM) as ctx:
        kname = ctx.kernel_name
        _check_name(r, kname)
        z, z_again = ctx.fvp(v), ctx.fvp(v)
        x = ctx.cg(b, T.CG_ITERS, 0.0) if g["cmp32"] else None
        ctx.set_rollout(p["mean"], p["action"], p["adv"])
        _check_line_search(tag + " default form", ctx, p, sref, klref)
        if T.mfma_surrogate(L):
            monkeypatch.setenv("TRPO_SURR_GENERIC", "1")
            _check_line_search(tag + " generic form", ctx, p, sref, klref)
            monkeypatch.delenv("TRPO_SURR_GENERIC")
        u = ctx.update()
    with trpo_amd.Context(L, ac, th, obs, std, LAM, precision="fp64") as c64:
        kname64 = c64.kernel_name
        z64 = c64.fvp(v)
        x64 = c64.cg(b, T.CG_ITERS, 0.0) if g["cmp64"] else None
    e_z, e_z64, e_b = T.rel_l2(z, g["zr"]), T.rel_l2(z64, g["zr"]), T.rel_l2(u["b"], g["bref"])
    e_x = T.rel_l2(x, g["xr"]) if g["cmp32"] else float("nan")
    e_x64 = T.rel_l2(x64, g["xr"]) if g["cmp64"] else float("nan")
    e_ux = T.rel_l2(u["x"], ref["x"])
    print("trained %s: kernel '%s' / '%s'; FVP %.2e fp64 %.2e; gradient %.2e; CG fp32 %.2e (gate %s, emulation "
          "%.1e) fp64 %.2e (gate %s, sensitivity %.1e); update x %.2e accepted %d / %d fp64_rerun %d (gate %s, "
          "emulation %.1e)" % (tag, kname, kname64, e_z, e_z64, e_b, e_x, g["cmp32"], g["cg32"], e_x64, g["cmp64"],
                               g["sens64"], e_ux, u["accepted"], ref["accepted"], u["fp64_rerun"], g["cmp_upd"],
                               g["upd32"]))
    np.testing.assert_array_equal(z, z_again)
    assert e_z <= FVP_TOL, (tag, kname)
    if setting == "S":
        assert np.all(np.isfinite(z)) and np.all(np.isfinite(z64)), tag
        np.testing.assert_array_equal(z[-A:], 2.0 * v[-A:] + LAM * v[-A:])
    assert e_b <= GRAD_TOL, (tag, kname)
    assert kname64.endswith("fp64"), kname64
    assert e_z64 <= FVP64_TOL, (tag, kname64)
    if g["cmp64"]:
        assert e_x64 <= max(1e-9, 100.0 * g["sens64"]), (tag, kname64, g["sens64"])
    if g["cmp32"]:
        assert e_x <= CG_TOL, (tag, kname)
    if g["cmp_upd"]:
        assert u["accepted"] == ref["accepted"], tag
        assert e_ux <= CG_TOL, (tag, u["ritz_residual"], u["fp64_rerun"])
        if ref["accepted"] >= 0:
            assert T.rel_l2(u["theta"] - th, ref["theta"] - th) <= CG_TOL, tag


def test_every_family_is_compared():
    """The gates, evaluated on this machine, admit a CG and an update comparison in every family."""
    for fam in T.FAMILIES:
        mine = [c for c in T.cases() if T.ROWS[c[0]]["family"] == fam]
        assert any(T.gates(*c)["cmp32"] for c in mine), fam
        assert any(T.gates(*c)["cmp_upd"] for c in mine), fam
