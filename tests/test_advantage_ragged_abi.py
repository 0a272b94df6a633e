"""ABI of the ragged advantage stage (include/trpo_mi355x.h), checked without a GPU: the two entry points
are declared (tests/test_abi.py then forces them into exports.map), refuse a NULL baseline, and the numpy
reference the GPU tests compare with (tests/ragged_ref.py) is pinned to the CPU oracle first: its baseline
forward against oracle.baseline_evaluate's predictions, and its cases' conditioning."""
import numpy as np
import pytest

import oracle
import ragged_ref as R
import trpo_amd

TRPO_E_INVALID = -1


def test_entry_points_are_declared_in_the_header():
    syms = trpo_amd.header_symbols()
    assert "trpo_baseline_set_data_ragged" in syms
    assert "trpo_baseline_advantage_ragged" in syms


def test_advantage_ragged_rejects_null_baseline():
    L = trpo_amd.lib()
    x, observ, reward = np.zeros(8), np.zeros(8), np.zeros(2)
    lens = np.array([2], np.uintp)
    rc = L.trpo_baseline_advantage_ragged(None, x, observ, reward, 1, lens.ctypes.data, 2, None, None, 0.995, 0.98,
                                          None, None, None)
    assert rc == TRPO_E_INVALID
    assert trpo_amd.last_error()


def test_set_data_ragged_rejects_null_baseline():
    L = trpo_amd.lib()
    observ, target = np.zeros(8), np.zeros(2)
    lens = np.array([2], np.uintp)
    assert L.trpo_baseline_set_data_ragged(None, observ, target, 1, lens.ctypes.data, 2) == TRPO_E_INVALID
    assert trpo_amd.last_error()


def test_numpy_forward_matches_the_oracle():
    """20 x 150, [16,16,16,1] "lttl": equal lengths with horizon = ep_len are the oracle's own rows."""
    lens = R.LENGTHS["20x150"]
    x, observ, _, _ = R.inputs(lens)
    V, _ = R.values(lens, 150)
    want = oracle.baseline_evaluate(list(R.BASE), R.AC, x, observ, np.zeros(V.size), 20, 150)[2]
    err = np.abs(V - want).max() / np.abs(want).max()
    print("numpy forward vs oracle predictions: %.3e" % err)
    assert err <= 1e-13


@pytest.mark.parametrize("gamma,lam", R.COEFFS)
@pytest.mark.parametrize("name,horizon,mode", R.PARITY_CASES)
def test_reference_cases_are_well_conditioned(name, horizon, mode, gamma, lam):
    ref = R.reference(R.LENGTHS[name], R.horizon_of(name, horizon), mode, gamma, lam)
    assert ref["conditioning"] >= 0.05, "ill-conditioned case: change its seed"
