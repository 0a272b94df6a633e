"""MI355X: the CG step's block reduction carries 3 + QB sums; x.p and p.p are the publishing block's own
(DESIGN §5.3).

Every block of the CG-iteration kernel repeats the fp64 step in its prologue.  Its single reduction sums
p.z, r.z, z.z and the QB basis dots; x.p and p.p, which feed only |x'|^2 and with it the ||x|| column of the
history, are summed by a second, two-value reduction that the publishing block alone runs, and the blocks
that do not publish load no x.  None of this may change a bit.  What it can get wrong: a sum read from the
wrong column of the narrower reduction (the basis dots moved from column 5 + i to 3 + i), the padded width on
the wrong side of the 3 + QB = 8 boundary, the second reduction on LDS the first still reads, x', ||x|| or
the next step's |x|^2 taken from a block that holds no x, a one-block launch (publisher = the only block)
treated as a non-publisher.  The 3 + QB step is a compile-time form of the MODE 3 kernels (S3), bound where
some wave runs more than one tile (more than 16 x blocks x 8 samples); below, the five-wide step stays.  So the
default grid at these sizes runs the five-wide kernels, one block at 257 and 517 the 3 + QB ones with the
publisher as only block, and two blocks at 517 (33 tiles on 16 waves) the 3 + QB ones with a block that does
not publish: a context bound to the wrong table, or one form's LDS sized for the other, shows here too.

Steps: maxiter = 1, 2, 5, 6, 7, 8, 10 end on steps holding nq = 0, 1, 4, 5, 6, 7, 9 vectors (and run every
size below on the way), maxiter = 17 ends on 16: both sides of the 3 + QB = 8 boundary (QB 5 | 6) and the
16-slot kernel.  The 17-step solve uses damping 0.01: at 0.1 these inputs reach round-off after 13 .. 16
steps and stop (tests/test_gpu_basis_slots.py).  The reference for the bits is the same solve with
TRPO_YCACHE=0 -- MODE 0 with the streaming basis dots, which shares the step's source with MODE 3 and must
keep its bits -- compared on x, the iteration count and BOTH columns of the history (||x|| is what x.p and p.p
feed).  Of a solve that stopped before maxiter on a non-positive |r|^2 that final |r|^2 is left out: it is
what cancellation leaves of the correction sum, which the two paths round differently (one case of 24, by
4e-31, tests/test_gpu_basis_slots.py); its ||x|| does not depend on that sum and stays in.  Sizes 17 (one
tile over the tile edge, one block), 257 and 517 (several blocks, the last partly empty), on the default grid
and on TRPO_FVP_BLOCKS=1; both narrow-output twins; armDOF_0 and a tanh-output net.  Tolerances against the
fp64 oracle: test_gpu_parity.py's (CG 1e-4) and test_gpu_coop_step.py's (history 1e-2), up to 10 iterations.
All solves are the fp32 solve itself (TRPO_RITZ_RERUN=0).  Every case passes on the commit before the change.
"""
import os

import numpy as np
import pytest

import cases
import oracle
import trpo_amd
from trpo_amd import synth

pytestmark = pytest.mark.gpu

CG_TOL = 1e-4                                         # test_gpu_parity.py's
HIST_RTOL = 1e-2                                      # test_gpu_coop_step.py's
TWINS = {"no-mfma": "1000000", "no-valu": "0"}       # TRPO_NO_VALU_MIN_TILES forcing each twin
L = [15, 16, 16, 3]                                   # armDOF_0
NS = [17, 257, 517]
MAXITERS = [1, 2, 5, 6, 7, 8, 10]                     # damping 0.1
LONG, LONG_DAMPING = 17, 0.01                         # all 17 steps run, the last holds 16 vectors
STD = np.array([0.7, 1.0, 1.4])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_sums_n517.txt")
GOLDEN_N = 517
GOLDEN_SOLVES = ((10, 0.1), (LONG, LONG_DAMPING))     # (maxiter, damping)

_REF = {}


def _problem(n):
    P = synth.num_params(L)
    return synth.make_theta(L), synth.make_obs(n, L[0]), synth.make_b(P)


def _oracle(acts, n, maxiter):
    """The fp64 oracle's solve (damping 0.1), computed once per (net, size, maxiter)."""
    if (acts, n, maxiter) not in _REF:
        th, obs, b = _problem(n)
        _REF[acts, n, maxiter] = oracle.cg(L, acts, th, obs, STD, b, maxiter, 0.0)
    return _REF[acts, n, maxiter]


def _env(monkeypatch, twin, blocks):
    if blocks:
        monkeypatch.setenv("TRPO_FVP_BLOCKS", str(blocks))
    if twin:
        monkeypatch.setenv("TRPO_NO_VALU_MIN_TILES", TWINS[twin])
    monkeypatch.setenv("TRPO_RITZ_RERUN", "0")


def _solves(acts, n, maxiters, twin=None, damping=0.1):
    """The solves of maxiters in a row on one context: [(x, |r|^2 history, ||x|| history, iterations,
    Ritz residual)]."""
    th, obs, b = _problem(n)
    out = []
    with trpo_amd.Context(L, acts, th, obs, STD, damping) as ctx:
        assert "coop" not in ctx.kernel_name and (not twin or ctx.kernel_name.endswith(twin)), ctx.kernel_name
        for m in maxiters:
            x = ctx.cg(b, m, 0.0)
            rr, xn, it = ctx.cg_history()
            out.append((x, np.array(rr), np.array(xn), it, ctx.cg_status()["ritz_residual"]))
    return out


def _same_solve(got, want, m):
    """Bit for bit: x, the iteration count, both columns of the history (without the non-positive |r|^2 a
    solve stopped on before maxiter)."""
    (x, rr, xn, it, _), (x0, rr0, xn0, it0, _) = got, want
    assert it == it0 <= m
    keep = it + 1 if it == m or rr0[-1] > 0.0 else it
    np.testing.assert_array_equal(x, x0, err_msg="x, maxiter %d" % m)
    np.testing.assert_array_equal(rr[:keep], rr0[:keep], err_msg="|r|^2 history, maxiter %d" % m)
    np.testing.assert_array_equal(xn, xn0, err_msg="||x|| history, maxiter %d" % m)
    assert len(xn) == it + 1 and xn[0] == 0.0 and np.all(xn[1:] > 0.0)


def _check(acts, twin, blocks, n, monkeypatch):
    _env(monkeypatch, twin, blocks)
    monkeypatch.setenv("TRPO_YCACHE", "0")
    stream = _solves(acts, n, MAXITERS, twin)
    stream17 = _solves(acts, n, [LONG], twin, damping=LONG_DAMPING)[0]
    monkeypatch.delenv("TRPO_YCACHE")
    cached = _solves(acts, n, MAXITERS, twin)
    cached17 = _solves(acts, n, [LONG], twin, damping=LONG_DAMPING)[0]
    for m, want, got in zip(MAXITERS, stream, cached):
        _same_solve(got, want, m)
        x, rr, xn, it, _ = got
        assert it == m
        ref = _oracle(acts, n, m)
        ex = cases.rel_l2(x, ref["x"])
        print("%s %s blocks %d N %d maxiter %d: CG relL2 %.3e |r|^2 max rel %.3e ||x|| max rel %.3e" % (
            acts, twin, blocks, n, m, ex, float(np.max(np.abs(rr / ref["rdotr"] - 1.0))),
            float(np.max(np.abs(xn[1:] / ref["xnorm"][1:] - 1.0)))))
        assert ex <= CG_TOL
        assert it == ref["iters"]
        np.testing.assert_allclose(rr, ref["rdotr"], rtol=HIST_RTOL)
        np.testing.assert_allclose(xn, ref["xnorm"], rtol=HIST_RTOL)
    _same_solve(cached17, stream17, LONG)
    assert cached17[3] == LONG


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("twin", list(TWINS))
def test_step_bits(twin, blocks, n, monkeypatch):
    _check("lttl", twin, blocks, n, monkeypatch)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("twin", list(TWINS))
def test_step_bits_tanh_output(twin, blocks, n, monkeypatch):
    _check("lttt", twin, blocks, n, monkeypatch)


@pytest.mark.parametrize("acts", ["lttl", "lttt"])
@pytest.mark.parametrize("twin", list(TWINS))
def test_step_bits_two_blocks(twin, acts, monkeypatch):
    """N = 517 on two blocks: every wave runs two or three tiles, so the 3 + QB kernels run, block 0 without
    x and block 1 as publisher."""
    _check(acts, twin, 2, 517, monkeypatch)


@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("twin", list(TWINS))
def test_ritz_residual(twin, blocks, monkeypatch):
    """cg_status' Ritz residual after 2 and after 10 iterations -- it is built from the steps' alpha and the
    |r|^2 history -- on a context that ran the other solve first equals the same call on a fresh context."""
    _env(monkeypatch, twin, blocks)
    for seq in ([2, 10], [10, 2]):
        row = _solves("lttl", 257, seq, twin)
        fresh = _solves("lttl", 257, seq[1:], twin)[0]
        assert np.isfinite(fresh[4]) and fresh[4] > 0.0
        assert row[1][4] == fresh[4], (seq, row[1][4], fresh[4])
        _same_solve(row[1], fresh, seq[1])


@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("twin", list(TWINS))
def test_sequence_on_one_context(twin, blocks, monkeypatch):
    """Solves of 3, 10, 1 and 7 iterations in a row on one context: |x|^2 and x start from zero in every solve
    and the publisher's sums belong to the launch that formed them, so each has a fresh context's bits."""
    _env(monkeypatch, twin, blocks)
    seq = [3, 10, 1, 7]
    row = _solves("lttl", 257, seq, twin)
    for m, got in zip(seq, row):
        _same_solve(got, _solves("lttl", 257, [m], twin)[0], m)
        assert got[3] == m


def golden_solves():
    """The solves tests/golden/step_sums_n517.txt records (default grid and twin, fp32 solve; the caller sets
    TRPO_RITZ_RERUN=0), each on a fresh context: {maxiter: (x, |r|^2 history, ||x|| history)}."""
    return {m: _solves("lttl", GOLDEN_N, [m], damping=d)[0][:3] for m, d in GOLDEN_SOLVES}


def test_parent_bits(monkeypatch):
    """x and both columns of the history for N = 517 after 10 and after 17 iterations equal the bits recorded
    from the commit before the change (the file's header names it; lines `maxiter column hex-double`)."""
    _env(monkeypatch, None, 0)
    want = {m: {"x": [], "rr": [], "xn": []} for m, _ in GOLDEN_SOLVES}
    with open(GOLDEN) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                m, col, h = line.split()
                want[int(m)][col].append(float.fromhex(h))
    got = golden_solves()
    for m, _ in GOLDEN_SOLVES:
        assert len(want[m]["x"]) == synth.num_params(L) and len(want[m]["rr"]) == len(want[m]["xn"]) == m + 1
        for col, arr in zip(("x", "rr", "xn"), got[m]):
            np.testing.assert_array_equal(arr, np.array(want[m][col]), err_msg="maxiter %d %s" % (m, col))
