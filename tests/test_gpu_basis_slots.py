"""MI355X: the CG-iteration kernel's reorthogonalisation slots are sized to the step that runs.

Step j-1 -> j removes the nq = min(j - 1, 16) stored basis vectors from the new residual; the MODE 3 kernel
that runs it is looked up by nq: for the armDOF_0-class shape the instantiation with exactly nq slots up to
8, then the 16-slot one.  None of this may change a bit.  What it can get wrong: a step launched on a kernel
with fewer slots than vectors held, a dynamic-LDS attribute missing on an instantiation, a boundary off by
one, a selection left over from a solve with another maxiter on the same context.

Every basis size: maxiter = 1 .. 12 and 17 launch nq = 0 .. 11 and 0 .. 16 (every exact size, the first
sizes on the 16-slot kernel and the cap).  With the damping of the other cases (0.1) these inputs reach
round-off after 13 .. 16 steps -- |r|^2 comes out non-positive and the solve stops, on either path and
before the slot table alike -- so the 17-step solve is run a second time with damping 0.01 (the fp64
oracle's |r_17|^2 / |r_0|^2 is 4e-7 .. 1e-5 there), where all 17 steps run and the last holds 16 vectors.
The reference for the bits is the same solve with TRPO_YCACHE=0: MODE 0 with the streaming basis dots,
which reproduces MODE 3's bits and takes no slot table.  (x, the iteration count and the residual history
are compared; of a solve that stopped at round-off the final, non-positive |r|^2 is left out: it is what
cancellation leaves of the correction sum, which the two paths round differently in its last bit -- one
case of 24 differs there, by 4e-31, with and without the slot table.)  Sizes: 17
(one tile over the tile edge, a single block), 257 and 517 (several blocks, the last one partly empty), each
on its own grid and on one block (publisher = block 0 = the only block); both narrow-output twins; armDOF_0
and a tanh-output net (the run-time-activation kernels).  Tolerances against the fp64 oracle are
test_gpu_parity.py's (CG 1e-4) and test_gpu_coop_step.py's (history 1e-2), up to 10 iterations; past that the
fp32 / fp64 drift at these sizes is unmeasured and only the bits are compared.  All solves are the fp32
solve itself (TRPO_RITZ_RERUN=0).
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
HIST_RTOL = 1e-2                                      # test_gpu_coop_step.py's, for the rdotr history
TWINS = {"no-mfma": "1000000", "no-valu": "0"}       # TRPO_NO_VALU_MIN_TILES forcing each twin
L = [15, 16, 16, 3]                                   # armDOF_0
NS = [17, 257, 517]
MAXITERS = list(range(1, 13)) + [17]
STD = np.array([0.7, 1.0, 1.4])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "basis_slots_x.txt")
GOLDEN_N, GOLDEN_MAXITERS = 517, (3, 7, 10)

_REF = {}


def _problem(n):
    P = synth.num_params(L)
    return synth.make_theta(L), synth.make_obs(n, L[0]), synth.make_b(P)


def _oracle(acts, n, maxiter):
    """The fp64 oracle's solve, computed once per (net, size, maxiter)."""
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
    """The solves of maxiters in a row on one context: [(x, rdotr history, iterations)]."""
    th, obs, b = _problem(n)
    out = []
    with trpo_amd.Context(L, acts, th, obs, STD, damping) as ctx:
        assert "coop" not in ctx.kernel_name and (not twin or ctx.kernel_name.endswith(twin)), ctx.kernel_name
        for m in maxiters:
            x = ctx.cg(b, m, 0.0)
            rr, _, it = ctx.cg_history()
            out.append((x, np.array(rr), it))
    return out


def _same_solve(got, want, m):
    """Bit for bit: x, the iteration count, the |r|^2 history (without the non-positive value a solve
    stopped on before maxiter)."""
    (x, rr, it), (x0, rr0, it0) = got, want
    assert it == it0 <= m
    keep = it + 1 if it == m or rr0[-1] > 0.0 else it
    np.testing.assert_array_equal(x, x0, err_msg="maxiter %d" % m)
    np.testing.assert_array_equal(rr[:keep], rr0[:keep], err_msg="maxiter %d" % m)


def _check_sizes(acts, twin, blocks, n, monkeypatch):
    _env(monkeypatch, twin, blocks)
    monkeypatch.setenv("TRPO_YCACHE", "0")
    stream = _solves(acts, n, MAXITERS, twin)
    monkeypatch.delenv("TRPO_YCACHE")
    slots = _solves(acts, n, MAXITERS, twin)
    for m, (x0, rr0, it0), (x, rr, it) in zip(MAXITERS, stream, slots):
        _same_solve((x, rr, it), (x0, rr0, it0), m)
        assert it == m or m == 17                      # 17 at this damping: stops at round-off (see above)
        if m <= 10:
            ref = _oracle(acts, n, m)
            ex = cases.rel_l2(x, ref["x"])
            print("%s %s blocks %d N %d maxiter %d: CG relL2 %.3e rdotr max rel %.3e" % (
                acts, twin, blocks, n, m, ex, float(np.max(np.abs(rr / ref["rdotr"] - 1.0)))))
            assert ex <= CG_TOL
            assert it == ref["iters"]
            np.testing.assert_allclose(rr, ref["rdotr"], rtol=HIST_RTOL)
    # the cap: all 17 steps run, the last one with QCAP = 16 vectors held
    monkeypatch.setenv("TRPO_YCACHE", "0")
    stream17 = _solves(acts, n, [17], twin, damping=0.01)[0]
    monkeypatch.delenv("TRPO_YCACHE")
    slots17 = _solves(acts, n, [17], twin, damping=0.01)[0]
    _same_solve(slots17, stream17, 17)
    assert slots17[2] == 17


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("twin", list(TWINS))
def test_every_basis_size(twin, blocks, n, monkeypatch):
    _check_sizes("lttl", twin, blocks, n, monkeypatch)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("twin", list(TWINS))
def test_every_basis_size_tanh_output(twin, blocks, n, monkeypatch):
    _check_sizes("lttt", twin, blocks, n, monkeypatch)


def golden_solves():
    """x of the solves tests/golden/basis_slots_x.txt records (default grid and twin, fp32 solve; the caller
    sets TRPO_RITZ_RERUN=0), each on a fresh context: {maxiter: x}."""
    return {m: _solves("lttl", GOLDEN_N, [m])[0][0] for m in GOLDEN_MAXITERS}


def test_parent_bits(monkeypatch):
    """x for N = 517 after 3, 7 and 10 iterations equals the bits recorded from the commit before the slot
    table (the file's header names it; lines `maxiter hex-double`)."""
    _env(monkeypatch, None, 0)
    want = {m: [] for m in GOLDEN_MAXITERS}
    with open(GOLDEN) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                m, h = line.split()
                want[int(m)].append(float.fromhex(h))
    got = golden_solves()
    for m in GOLDEN_MAXITERS:
        np.testing.assert_array_equal(got[m], np.array(want[m]), err_msg="maxiter %d" % m)


@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("twin", list(TWINS))
def test_selection_across_solves(twin, blocks, monkeypatch):
    """Solves of 3, 10, 3 and 17 iterations in a row on one context: the kernel is chosen per launch and the
    replica sets are zeroed for whatever comes next, so each has a fresh context's bits."""
    _env(monkeypatch, twin, blocks)
    seq = [3, 10, 3, 17]
    row = _solves("lttl", 257, seq, twin)
    for m, (x, rr, it) in zip(seq, row):
        _same_solve((x, rr, it), _solves("lttl", 257, [m], twin)[0], m)
        assert it == m or m == 17


@pytest.mark.parametrize("twin", list(TWINS))
def test_reorth_off(twin, monkeypatch):
    """TRPO_CG_REORTH=0: every step holds no basis vector (the slotless kernel throughout) and keeps the
    bits of the TRPO_YCACHE=0 solve."""
    _env(monkeypatch, twin, 0)
    monkeypatch.setenv("TRPO_CG_REORTH", "0")
    monkeypatch.setenv("TRPO_YCACHE", "0")
    x0, rr0, it0 = _solves("lttl", 257, [10], twin)[0]
    monkeypatch.delenv("TRPO_YCACHE")
    x, rr, it = _solves("lttl", 257, [10], twin)[0]
    _same_solve((x, rr, it), (x0, rr0, it0), 10)
    assert it == 10


def test_large_batch_rungs(monkeypatch):
    """Above 131 072 samples the steps run the rungs {0, 4, 8, 16} (the per-size kernels stop paying once a
    launch's samples push the code out of L2): the first size past the cut keeps the
    TRPO_YCACHE=0 bits like the sizes below it."""
    _env(monkeypatch, None, 0)
    monkeypatch.setenv("TRPO_YCACHE", "0")
    want = _solves("lttl", 131073, [10])[0]
    monkeypatch.delenv("TRPO_YCACHE")
    _same_solve(_solves("lttl", 131073, [10])[0], want, 10)
