"""MI355X: the epilogue of the small-net tile kernel (fvp_mlp3_kernel) and who publishes.

The wave dumps of the atomic-replica epilogue have an LDS region of their own (one block barrier, in front
of the gather), and the LAST block -- not block 0 -- loads x, publishes the CG step (p', r', x, the basis
row, the scalar state, the history, ctl, alpha[]) and zeroes the next-but-one replica set.  None of this
may change a bit.  What it can get wrong: a dump that lands on memory a slower wave still reads, a gather
that starts early, a state field left on block 0, a replica set left non-zero for the next solve.

Sizes: 1, 15, 16, 17 (the tile edge), 127, 128, 129 (one 8-wave block: short, full, one tile over),
255, 257 (two blocks / a third block owning a single tile), 517 (test_gpu_tile_chain.py's upper size);
each on its own grid and on one and two blocks (TRPO_FVP_BLOCKS), so that the last block is block 0, a
full block, and a partly empty one; both narrow-output twins (TRPO_NO_VALU_MIN_TILES); armDOF_0 and a
tanh-output net (the run-time activation kernels).  Tolerances against the fp64 oracle are
test_gpu_parity.py's (FVP 1e-5, CG 1e-4; the solve as a caller gets it, stall guard included); the bit
comparisons run the fp32 solve itself (TRPO_RITZ_RERUN=0).
"""
import os

import numpy as np
import pytest

import cases
import oracle
import trpo_amd
from trpo_amd import synth

pytestmark = pytest.mark.gpu

FVP_TOL, CG_TOL = 1e-5, 1e-4                          # test_gpu_parity.py's
HIST_RTOL = 1e-2                                      # test_gpu_coop_step.py's, for the rdotr history
TWINS = {"no-mfma": "1000000", "no-valu": "0"}       # TRPO_NO_VALU_MIN_TILES forcing each twin
L = [15, 16, 16, 3]                                   # armDOF_0
NS = [1, 15, 16, 17, 127, 128, 129, 255, 257, 517]
STD = np.array([0.7, 1.0, 1.4])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_REF = {}


def _problem(n):
    P = synth.num_params(L)
    return synth.make_theta(L), synth.make_obs(n, L[0]), synth.make_v(P), synth.make_b(P)


def _oracle(acts, n):
    """FVP and the 10-iteration solve of the fp64 oracle, computed once per (net, size)."""
    if (acts, n) not in _REF:
        th, obs, v, b = _problem(n)
        zr, _ = oracle.fvp(L, acts, th, obs, STD, v)
        _REF[acts, n] = (zr, oracle.cg(L, acts, th, obs, STD, b, 10, 0.0))
    return _REF[acts, n]


def _env(monkeypatch, twin, blocks):
    if blocks:
        monkeypatch.setenv("TRPO_FVP_BLOCKS", str(blocks))
    monkeypatch.setenv("TRPO_NO_VALU_MIN_TILES", TWINS[twin])


def _run(acts, twin, n, monkeypatch):
    """A standalone FVP, the solve as a caller gets it, then the fp32 solve and another FVP."""
    th, obs, v, b = _problem(n)
    monkeypatch.delenv("TRPO_RITZ_RERUN", raising=False)
    with trpo_amd.Context(L, acts, th, obs, STD, 0.1) as ctx:
        assert ctx.kernel_name.endswith(twin) and "coop" not in ctx.kernel_name, ctx.kernel_name
        z = ctx.fvp(v)
        x = ctx.cg(b, 10, 0.0)
        monkeypatch.setenv("TRPO_RITZ_RERUN", "0")
        x32 = ctx.cg(b, 10, 0.0)
        z2 = ctx.fvp(v)
    return z, x, x32, z2


def _check(acts, twin, blocks, n, monkeypatch):
    _env(monkeypatch, twin, blocks)
    monkeypatch.setenv("TRPO_YCACHE", "0")
    z0, _, x0, z02 = _run(acts, twin, n, monkeypatch)
    monkeypatch.delenv("TRPO_YCACHE")
    z, x, x32, z2 = _run(acts, twin, n, monkeypatch)
    zr, cgr = _oracle(acts, n)
    ez, ex = cases.rel_l2(z, zr), cases.rel_l2(x, cgr["x"])
    print("%s %s blocks %d N %d: FVP relL2 %.3e CG relL2 %.3e" % (acts, twin, blocks, n, ez, ex))
    assert ez <= FVP_TOL
    assert ex <= CG_TOL
    for a in (z, z2, z02):
        np.testing.assert_array_equal(a, z0)           # cached forward == recomputed, FVP after a solve
    np.testing.assert_array_equal(x32, x0)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("blocks", [0, 1, 2])
@pytest.mark.parametrize("twin", list(TWINS))
def test_parity_and_bits(twin, blocks, n, monkeypatch):
    _check("lttl", twin, blocks, n, monkeypatch)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("twin", list(TWINS))
def test_parity_and_bits_tanh_output(twin, n, monkeypatch):
    _check("lttt", twin, 0, n, monkeypatch)


@pytest.mark.parametrize("blocks", [0, 1, 2])
@pytest.mark.parametrize("twin", list(TWINS))
def test_zeroing(twin, blocks, monkeypatch):
    """Every solve's launches zero the replica sets two launches ahead (the last block's duty) and the last
    step the next solve's first: three solves in a row repeat bit for bit, and a solve after an early stop
    (the residual threshold met at iteration 3; at iteration 0 with b = 0) has a fresh context's bits."""
    _env(monkeypatch, twin, blocks)
    monkeypatch.setenv("TRPO_RITZ_RERUN", "0")
    n = 257
    th, obs, _, b = _problem(n)
    rr = _oracle("lttl", n)[1]["rdotr"]
    resth = float(np.sqrt(rr[3] * rr[2]))              # between |r_2|^2 and |r_3|^2: met at iteration 3
    assert rr[3] < resth < rr[2] and min(rr[:3]) > resth
    with trpo_amd.Context(L, "lttl", th, obs, STD, 0.1) as ctx:
        fresh = ctx.cg(b, 10, 0.0)
        again = [ctx.cg(b, 10, 0.0) for _ in range(2)]
    with trpo_amd.Context(L, "lttl", th, obs, STD, 0.1) as ctx:
        ctx.cg(b, 10, resth)
        _, _, it3 = ctx.cg_history()
        after3 = ctx.cg(b, 10, 0.0)
        x_zero = ctx.cg(np.zeros_like(b), 10, 1e-10)
        _, _, it0 = ctx.cg_history()
        after0 = ctx.cg(b, 10, 0.0)
    assert it3 == 3 and it0 == 0
    assert np.all(x_zero == 0.0)
    for a in again + [after3, after0]:
        np.testing.assert_array_equal(a, fresh)


def _ritz_oracle(acts, th, obs, b, m):
    """The statistic trpo_ctx_cg_status derives from the published alpha[] and history (the smallest
    relative Ritz residual of the solve's Lanczos matrix), from an fp64 CG on the oracle's FVP."""
    x, r, p = np.zeros_like(b), b.copy(), b.copy()
    rr, al = [float(r @ r)], []
    for _ in range(m):
        z, _ = oracle.fvp(L, acts, th, obs, STD, p)
        a = rr[-1] / float(p @ z)
        x, r = x + a * p, r - a * z
        rr.append(float(r @ r))
        al.append(a)
        p = r + (rr[-1] / rr[-2]) * p
    T = np.zeros((m, m))
    for j in range(m):
        T[j, j] = 1.0 / al[j] + (rr[j] / rr[j - 1] / al[j - 1] if j else 0.0)
        if j + 1 < m:
            T[j, j + 1] = T[j + 1, j] = np.sqrt(rr[j + 1] / rr[j]) / al[j]
    _, V = np.linalg.eigh(T)
    bk = np.sqrt(rr[m] / rr[m - 1]) / al[m - 1]
    return min(1.0, float(np.min(bk * np.abs(V[-1, :])) / np.max(np.abs(np.diag(T))))), np.array(rr)


@pytest.mark.parametrize("maxiter", [1, 2, 10])
@pytest.mark.parametrize("blocks", [0, 1])
def test_published_state(blocks, maxiter, monkeypatch):
    """History, iteration count and the alpha's (through cg_status's Ritz residual, the only place a caller
    sees them) after 1, 2 and 10 iterations.  The Ritz residual's inputs are the alpha's and ratios of
    the history, each held to HIST_RTOL: for one and two steps it is a closed form of them (one step:
    sqrt(rr_1 / rr_0)) and gets 4 HIST_RTOL; after ten steps the smallest residual belongs to an
    eigenvector of a 10 x 10 matrix whose last component amplifies the entries' error, so it is held
    to a factor of two -- an alpha left unpublished cuts the matrix to a prefix (or gives 1)."""
    _env(monkeypatch, "no-mfma", blocks)
    monkeypatch.setenv("TRPO_RITZ_RERUN", "0")
    n = 257
    th, obs, _, b = _problem(n)
    ref = oracle.cg(L, "lttl", th, obs, STD, b, maxiter, 0.0)
    ritz_ref, rr_ref = _ritz_oracle("lttl", th, obs, b, maxiter)
    # the fp64 CG above is the oracle's (an operator or recurrence slip would show at O(1); the two differ
    # by fp64 rounding amplified along the recurrence, 1.4e-4 on the last of ten residuals)
    np.testing.assert_allclose(rr_ref, ref["rdotr"], rtol=HIST_RTOL)
    with trpo_amd.Context(L, "lttl", th, obs, STD, 0.1) as ctx:
        x = ctx.cg(b, maxiter, 0.0)
        rr, xn, it = ctx.cg_history()
        st = ctx.cg_status()
    print("maxiter %d blocks %d: iters %d ritz %.6e (oracle %.6e) x relL2 %.3e" % (
        maxiter, blocks, it, st["ritz_residual"], ritz_ref, cases.rel_l2(x, ref["x"])))
    assert it == ref["iters"] == maxiter
    assert cases.rel_l2(x, ref["x"]) <= CG_TOL
    np.testing.assert_allclose(rr, ref["rdotr"], rtol=HIST_RTOL)
    np.testing.assert_allclose(xn, ref["xnorm"], rtol=HIST_RTOL)
    if maxiter <= 2:
        np.testing.assert_allclose(st["ritz_residual"], ritz_ref, rtol=4 * HIST_RTOL)
    else:
        assert 0.5 * ritz_ref <= st["ritz_residual"] <= 2.0 * ritz_ref
    assert not st["fp64_rerun"]


def test_two_ranks_one_gpu():
    """Two ranks in one process (the peer-window exchange reads the replica sets the kernels wrote, not one
    block's stores): both end with the same bits, which are the bits recorded from the commit before the
    epilogue changed (tests/golden/epilogue_path_peer2_x.txt, one hex double per line)."""
    from test_gpu_peer import run_peer_ranks
    n = 517
    th, obs, _, b = _problem(n)
    bounds = [(0, 257), (257, n)]
    ctxs = [trpo_amd.Context(L, "lttl", th, obs[lo:hi], STD, 0.1) for lo, hi in bounds]
    try:
        res = run_peer_ranks(ctxs, lambda ctx, r: ctx.cg(b, 10, 0.0), warm=lambda ctx: ctx.cg(b, 10, 0.0))
    finally:
        for ctx in ctxs:
            ctx.close()
    with open(os.path.join(GOLDEN, "epilogue_path_peer2_x.txt")) as f:
        want = np.array([float.fromhex(s) for s in f.read().split()])
    np.testing.assert_array_equal(res[1], res[0])
    np.testing.assert_array_equal(res[0], want)
    assert cases.rel_l2(res[0], _oracle("lttl", n)[1]["x"]) <= CG_TOL
