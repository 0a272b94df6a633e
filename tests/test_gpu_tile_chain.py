"""MI355X: the small-net tile kernel (fvp_mlp3_kernel) with its weight-gradient contractions deferred
(DESIGN §5.1).

Each wave transposes the operands of RGW2 / RGW1 / RGW0 through a scratch region of its own and runs the
three contractions as one batch behind G1.  What that can get wrong shows where a wave runs more than one
tile: a region reused before the previous trip's reads have returned, a batch left incomplete across the
ring loop's unroll by two, a ragged last tile.  The grid is shrunk to one and two blocks of 8 waves
(TRPO_FVP_BLOCKS), so multi-trip waves occur at tiny N:

  N = 1, 17          a single, ragged tile
  N = 128            one block: every wave exactly one full tile
  N = 129            one block: one wave a second tile with one live column
  N = 257            one block: a wave with three trips (ring slot 0 reused)
  N = 16 * 8 * 4 + 5 one block: four trips, ragged last

Both narrow-output twins (TRPO_NO_VALU_MIN_TILES), a tanh output layer (y3 cached; the run-time
activation kernels, ACT = -1).  Checked: FVP and CG against the fp64 oracle to test_gpu_parity.py's
tolerances, the cached forward (MODE 2 / 3) bit for bit against recomputing (TRPO_YCACHE=0), and
consecutive FVPs / solves bit for bit against each other.
"""
import numpy as np
import pytest

import cases
import oracle
import trpo_amd
from trpo_amd import synth

pytestmark = pytest.mark.gpu

FVP_TOL, CG_TOL = 1e-5, 1e-4                          # test_gpu_parity.py's
TWINS = {"no-mfma": "1000000", "no-valu": "0"}       # TRPO_NO_VALU_MIN_TILES forcing each twin
L = [15, 16, 16, 3]                                   # armDOF_0
NS = [1, 17, 128, 129, 257, 16 * 8 * 4 + 5]
STD = np.array([0.7, 1.0, 1.4])


def _problem(n):
    P = synth.num_params(L)
    return synth.make_theta(L), synth.make_obs(n, L[0]), synth.make_v(P), synth.make_b(P)


def _run(acts, twin, n):
    """Three FVPs (the first writes the forward cache, the others read it), two solves, one more FVP."""
    th, obs, v, b = _problem(n)
    with trpo_amd.Context(L, acts, th, obs, STD, 0.1) as ctx:
        assert ctx.kernel_name.endswith(twin) and "coop" not in ctx.kernel_name, ctx.kernel_name
        z = [ctx.fvp(v) for _ in range(3)]
        x = [ctx.cg(b, 10, 0.0) for _ in range(2)]
        z.append(ctx.fvp(v))
    return z, x


def _check(acts, twin, blocks, n, monkeypatch):
    monkeypatch.setenv("TRPO_FVP_BLOCKS", str(blocks))
    monkeypatch.setenv("TRPO_NO_VALU_MIN_TILES", TWINS[twin])
    monkeypatch.setenv("TRPO_RITZ_RERUN", "0")        # the fp32 solve itself, not an fp64 re-solve
    monkeypatch.setenv("TRPO_YCACHE", "0")
    z0, x0 = _run(acts, twin, n)
    monkeypatch.delenv("TRPO_YCACHE")
    z, x = _run(acts, twin, n)
    th, obs, v, _ = _problem(n)
    zr, _ = oracle.fvp(L, acts, th, obs, STD, v)
    err = cases.rel_l2(z[1], zr)
    print("%s %s blocks %d N %d: FVP relL2 %.3e" % (acts, twin, blocks, n, err))
    assert err <= FVP_TOL                                              # a
    for a in z + z0:
        np.testing.assert_array_equal(a, z0[0])                        # c, d: FVPs
    for a in x + x0:
        np.testing.assert_array_equal(a, x0[0])                        # c, d: solves
    assert np.all(np.isfinite(x[0]))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("twin", list(TWINS))
def test_fvp_and_solves_bitwise_and_oracle(twin, blocks, n, monkeypatch):
    _check("lttl", twin, blocks, n, monkeypatch)


@pytest.mark.parametrize("n", [129, 257])
@pytest.mark.parametrize("twin", list(TWINS))
def test_tanh_output_runtime_activations(twin, n, monkeypatch):
    """act3 = tanh: y3 is cached too, and the shape runs the run-time activation kernels (ACT = -1)."""
    _check("lttt", twin, 1, n, monkeypatch)


@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("twin", list(TWINS))
def test_cg_against_oracle_three_trips(twin, blocks, monkeypatch):
    """b: the 10-iteration solve at N = 257 (three trips on one wave) against the fp64 oracle."""
    monkeypatch.setenv("TRPO_FVP_BLOCKS", str(blocks))
    monkeypatch.setenv("TRPO_NO_VALU_MIN_TILES", TWINS[twin])
    n = 257
    th, obs, _, b = _problem(n)
    with trpo_amd.Context(L, "lttl", th, obs, STD, 0.1) as ctx:
        assert ctx.kernel_name.endswith(twin), ctx.kernel_name
        x = ctx.cg(b, 10, 0.0)
    xr = oracle.cg(L, "lttl", th, obs, STD, b, 10, 0.0)["x"]
    err = cases.rel_l2(x, xr)
    print("%s blocks %d N %d: CG relL2 %.3e" % (twin, blocks, n, err))
    assert err <= CG_TOL
