"""CPU check of tests/baseline_forms.py, so that tests/test_gpu_baseline_forms.py can rely on its cases
instead of skipping them.  Printed before it is asserted:

  * the case table's forms follow from the row counts (8 rows 65 bytes + 8 theta against 160 KiB), every form
    the host can select for a one-sample-per-lane kernel is in the table, and baseline_predict_kernel's
    "Y in LDS, theta in global" cannot be planned for any net;
  * per case, the CPU oracle's f, g and predictions lie within 1e-14 of a numpy.longdouble evaluate written
    from the definition: the device's bounds (f 1e-13, g and predictions 1e-12) leave the oracle 10x room or more;
  * scale 1.0 saturates: the wide shapes' first-layer pre-activations pass |z| = 15;
  * the fit's gate (vfit_ref.sensitivity <= 1e-9, tests/test_gpu_vfit.py's rule) admits every RELY_FIT case, the
    reference under random orders of the samples stays within the bound the case will be compared at
    (baseline_forms.fit_reorder_distance says why reversal alone is not enough at N = 17), and the cases cover
    every product form, every candidates form (lane included) and both settings;
  * the advantage reference's conditioning std A / max|A| >= 0.05 holds for every row used there.
"""
import numpy as np
import pytest

import baseline_forms as F
import ragged_ref

RS_BYTES, LDS_CAP = 8 * 65, 160 * 1024
ORACLE_TOL = 1e-14


def plan(rows, theta):
    """rows_plan (csrc/upd_host.h) in words."""
    if rows * RS_BYTES > LDS_CAP:
        return F.G
    return F.T if rows * RS_BYTES + 8 * theta <= LDS_CAP else F.Y


def planned(layers):
    S, P = sum(layers), sum(a * b + b for a, b in zip(layers[:-1], layers[1:]))
    lane = len(layers) == 4 and max(layers[:3]) <= 16
    ev = plan(2 * S + 2, P)
    cand = plan(S, 0)
    return dict(eval=F.LANE if lane else ev, predict=plan(S, P) if ev != F.G else F.G,
                gnvp=F.LANE if lane else plan(3 * S + 2, 2 * P),
                cand=F.LANE if lane else (F.G if cand == F.G else F.Y))


@pytest.mark.parametrize("row", range(len(F.ROWS)))
def test_table_forms_follow_from_the_row_counts(row):
    r = F.ROWS[row]
    assert r["forms"] == planned(r["layers"]), (r["layers"], planned(r["layers"]))
    assert F.parse_name(r["name"]) == r["forms"]
    assert len(r["layers"]) <= 8 and r["layers"][-1] == 1 and len(r["ac"]) == len(r["layers"])


def test_every_selectable_form_is_in_the_table():
    """The lane rows run the one-sample-per-lane kernels too (TRPO_BASELINE_LANE=0), but only in the form
    the narrow nets of the table already take; the coverage is asked of the rows as they run by default."""
    for user, forms in F.SELECTABLE.items():
        seen = {r["forms"][user] for r in F.ROWS} - {F.LANE}
        assert seen == forms, (user, seen)


def test_predict_kernel_has_no_lds_form_without_theta():
    """With S = the sum of the widths, evaluate's 2 S + 2 rows fit only for S <= 156, and a net with widths
    summing to S has at most S^2 / 4 + S weights and biases (adjacent products: even-indexed widths times
    odd-indexed ones), so theta always fits behind the prediction pass's S rows."""
    S_max = max(S for S in range(2, 400) if (2 * S + 2) * RS_BYTES <= LDS_CAP)
    assert S_max == 156
    worst = max(S * RS_BYTES + 8 * (S * S // 4 + S) for S in range(2, S_max + 1))
    print("predict: at most %d bytes of %d" % (worst, LDS_CAP))
    assert worst <= LDS_CAP
    # and the bound on the parameter count, by enumeration of the two- and three-layer splits of a small S
    for S in (9, 20):
        most = max([a * (S - a) + (S - a) for a in range(1, S)] +
                   [a * b + b + b * (S - a - b) + (S - a - b) for a in range(1, S) for b in range(1, S - a)])
        assert most <= S * S // 4 + S


@pytest.mark.parametrize("c", F.cases(), ids=F.case_id)
def test_oracle_is_the_long_double_evaluate(c):
    cs = F.case(*c)
    P = cs["phi"].size
    f, g, pred = F.evaluate_ref(*c)
    fl, gl, pl = F.evaluate_longdouble(cs["layers"], cs["ac"], cs["phi"], cs["X"], cs["y"])
    e_f, e_g, e_p = float(abs(f - fl) / abs(fl)), F.rel_l2(g[:P], gl), F.rel_l2(pred, pl)
    z = F.preact_max(*c)
    print("baseline forms %s: oracle vs long double f %.1e g %.1e predict %.1e; first-layer max|z| %.1f" % (
        F.case_id(c), e_f, e_g, e_p, z))
    assert e_f <= ORACLE_TOL and e_g <= ORACLE_TOL and e_p <= ORACLE_TOL
    assert np.all(g[P:] == 0.0)
    if c[0] in F.WIDE and c[2] == "sat":
        assert z >= 15.0, z


def test_fit_gate_admits_what_the_gpu_test_relies_on():
    seen_gnvp, seen_cand, seen_setting = set(), set(), set()
    for row, batch, setting in F.RELY_FIT:
        assert batch in F.ROWS[row]["batches"] and batch != F.BIG
        s, d = F.fit_sensitivity(row, batch, setting), F.fit_reorder_distance(row, batch, setting)
        print("baseline forms %s: fit sensitivity %.1e, random orders %.1e" % (F.case_id((row, batch, setting)), s, d))
        assert s <= F.FIT_GATE, (F.case_id((row, batch, setting)), s)
        assert d <= max(1e-12, 100.0 * s), (F.case_id((row, batch, setting)), s, d)
        seen_gnvp.add(F.ROWS[row]["forms"]["gnvp"])
        seen_cand.add(F.ROWS[row]["forms"]["cand"])
        seen_setting.add(setting)
    assert seen_gnvp == F.SELECTABLE["gnvp"] | {F.LANE}
    assert seen_cand == F.SELECTABLE["cand"] | {F.LANE}
    assert seen_setting == set(F.SCALES)


def test_advantage_cases_are_well_conditioned():
    for row in F.ADV_ROWS:
        assert F.ADV_BATCH in F.ROWS[row]["batches"]
        for setting in F.SCALES:
            for gamma, lam in F.ADV_COEFFS:
                k = F.advantage_ref(row, setting, gamma, lam)["conditioning"]
                print("baseline forms %s (%g, %g): std A / max|A| %.3f" % (
                    F.case_id((row, F.ADV_BATCH, setting)), gamma, lam, k))
                assert k >= F.ADV_GATE
    layers, ac = F.ROWS[F.RAGGED_ROW]["layers"], F.ROWS[F.RAGGED_ROW]["ac"]
    for gamma, lam in F.ADV_COEFFS:
        k = ragged_ref.reference(F.RAGGED_LENS, F.RAGGED_HORIZON, "all", gamma, lam, layers, ac)["conditioning"]
        print("baseline forms ragged (%g, %g): std A / max|A| %.3f" % (gamma, lam, k))
        assert k >= F.ADV_GATE
