"""ABI of the device trust-region value fit (include/trpo_mi355x.h Part 2), checked without a GPU: the layout
of trpo_vfit_info, the two entry points in the header and in the library, the refusals that need no device, and
the numpy reference (tests/vfit_ref.py) against finite differences of its own forward pass."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np

import trpo_amd
import vfit_ref as R

TRPO_E_INVALID = -1


def test_vfit_info_layout_matches_c(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "off.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "trpo_mi355x.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(trpo_vfit_info),
                 offsetof(trpo_vfit_info, loss_before), offsetof(trpo_vfit_info, gnorm),
                 offsetof(trpo_vfit_info, shs), offsetof(trpo_vfit_info, alpha_tr),
                 offsetof(trpo_vfit_info, alpha0), offsetof(trpo_vfit_info, loss), offsetof(trpo_vfit_info, shift),
                 offsetof(trpo_vfit_info, rdotr), offsetof(trpo_vfit_info, cg_iters),
                 offsetof(trpo_vfit_info, evaluated), offsetof(trpo_vfit_info, accepted), TRPO_VFIT_MAX_CG,
                 TRPO_MAX_BACKTRACKS);
          return 0; }
    """))
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    T = trpo_amd.VFitInfo
    assert [name for name, _ in T._fields_] == ["loss_before", "gnorm", "shs", "alpha_tr", "alpha0", "loss", "shift",
                                                "rdotr", "cg_iters", "evaluated", "accepted"]
    assert got == [C.sizeof(T), T.loss_before.offset, T.gnorm.offset, T.shs.offset, T.alpha_tr.offset,
                   T.alpha0.offset, T.loss.offset, T.shift.offset, T.rdotr.offset, T.cg_iters.offset,
                   T.evaluated.offset, T.accepted.offset, trpo_amd.VFIT_MAX_CG, trpo_amd.MAX_BACKTRACKS]
    assert got == [40 + 2 * 256 + 65 * 8 + 16, 0, 8, 16, 24, 32, 40, 296, 552, 1072, 1080, 1084, 64, 32]


def test_entry_points_are_declared_and_exported():
    syms = trpo_amd.header_symbols()
    L = trpo_amd.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", trpo_amd.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in ("trpo_baseline_gnvp", "trpo_baseline_fit_tr", "trpo_baseline_kernel_name"):
        assert name in syms
        assert hasattr(L, name)
        assert " T %s\n" % name in out
    assert L.trpo_baseline_kernel_name(None) == b""


def test_null_object_is_refused_before_anything_else():
    """A NULL baseline (and then a NULL x or x_out) is refused whatever eps, damping and shift_cap are: no
    device is needed to say so."""
    L = trpo_amd.lib()
    x, out = np.zeros(8), np.zeros(8)
    info = trpo_amd.VFitInfo()
    for eps in (0.01, 0.0, -1.0, float("nan")):
        for damping in (1e-3, -1.0, float("nan")):
            for cap in (0.015, float("inf"), 0.0, -1.0, float("nan")):
                rc = L.trpo_baseline_fit_tr(None, x.ctypes.data, 8, eps, 10, 1e-10, damping, 10, cap, out.ctypes.data,
                                            None, C.byref(info))
                assert rc == TRPO_E_INVALID
    assert L.trpo_baseline_fit_tr(None, None, 8, 0.01, 10, 1e-10, 1e-3, 10, 0.015, None, None, None) == TRPO_E_INVALID
    assert trpo_amd.last_error()
    for damping in (0.0, -1.0, float("nan")):
        assert L.trpo_baseline_gnvp(None, x.ctypes.data, x.ctypes.data, 8, damping, out.ctypes.data) == TRPO_E_INVALID


def test_reference_jacobian_against_finite_differences():
    """vfit_ref's explicit Jacobian is the derivative of its own forward pass (central differences, h = 1e-6:
    truncation h^2 |V'''| / 6 ~ 1e-13 and rounding u |V| / h ~ 1e-10, so 1e-8 relative to the largest entry)."""
    for layers, ac in (((6, 7, 3, 1), "lttl"), ((4, 8, 8, 8, 1), "ltttl"), ((5, 1), "ll"), ((12, 32, 1), "ltl"),
                       ((6, 7, 3, 1), "ltll")):
        phi, observ, _ = R.problem(layers, 1, 5)
        X = R.rows(observ, 1, 5)
        _, J = R.forward_jac(layers, ac, phi, X)
        assert J.shape == (5, R.num_params(layers))
        h, fd = 1e-6, np.zeros_like(J)
        for q in range(phi.size):
            e = np.zeros(phi.size)
            e[q] = h
            fd[:, q] = (R.forward_jac(layers, ac, phi + e, X, False)[0] -
                        R.forward_jac(layers, ac, phi - e, X, False)[0]) / (2 * h)
        assert np.abs(J - fd).max() <= 1e-8 * np.abs(J).max()


def test_reference_cg_solves_the_linear_model():
    """With a model linear in phi, no damping and P iterations the reference's step is the least-squares one."""
    layers, ac = (5, 1), "ll"
    phi, observ, y = R.problem(layers, 1, 40)
    X = R.rows(observ, 1, 40)
    f = R.fit(layers, ac, phi, X, y, 1e9, phi.size + 2, 0.0, 0.0, 1, np.inf)
    best = np.linalg.lstsq(np.column_stack([X, np.ones(40)]), y, rcond=None)[0]
    assert f["alpha0"] == 1.0 and f["accepted"] == 0
    assert R.vec_err(f["x_out"], best) <= 1e-12
