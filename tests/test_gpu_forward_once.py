"""MI355X: each theta's forward pass runs once -- K_0 of a solve and the policy gradient share the
forward-activation cache.

On the one-wave path a solve whose context already holds the cache for the current theta and observations
runs K_0 on it (the cached-forward kernel with the CG start), and the policy gradient stores the cache on
the way, so an update runs the forward pass once.  None of this may change a bit.  What it can get wrong:
a cache read after set_theta / set_obs / a re-bound twin made it stale, a captured graph replaying the
cached K_0 on an invalid cache, a policy-gradient forward pass that rounds differently from the FVP
kernel's, a CG start that differs between the two K_0 kernels, a silent fall-back to recomputing (hence
the counter, Context.forward_passes).

Every comparison is bit for bit: x, the iteration count and the |r|^2 / |x| histories against a fresh
context that ran only the solve in question, or against a context created under TRPO_YCACHE=0.  Sizes: 17
(one tile with a ragged tail), 257 (several tiles) and 517 (more tiles than one block's waves); armDOF_0
and the tanh-output net (its y3 is cached too); both narrow-output twins.  The bound against the fp64
oracle is test_gpu_parity.py's (CG 1e-4).  All solves are the fp32 solve itself (TRPO_RITZ_RERUN=0).

Run against a library from before the change (TRPO_LIB) the comparisons still apply and the counter
assertions, which need the new entry point, are left out.
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
TWINS = {"no-mfma": "1000000", "no-valu": "0"}       # TRPO_NO_VALU_MIN_TILES forcing each twin
L = [15, 16, 16, 3]                                   # armDOF_0
P = synth.num_params(L)
NS = [17, 257, 517]
NETS = ["lttl", "lttt"]
STD = np.array([0.7, 1.0, 1.4])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "basis_slots_x.txt")
GOLDEN_N, GOLDEN_MAXITERS = 517, (3, 7, 10)

TH = {0: synth.make_theta(L), 1: synth.make_theta(L, seed=synth.SEED + 1)}
B = {0: synth.make_b(P), 1: synth.make_b(P, seed=synth.SEED + 1)}
V = synth.make_v(P)

_FRESH, _REF = {}, {}


def _obs(n):
    return synth.make_obs(n, L[0])


def _env(monkeypatch, twin):
    if twin:
        monkeypatch.setenv("TRPO_NO_VALU_MIN_TILES", TWINS[twin])
    monkeypatch.setenv("TRPO_RITZ_RERUN", "0")


def _ctx(acts, n, twin=None, th=0):
    ctx = trpo_amd.Context(L, acts, TH[th], _obs(n), STD, 0.1)
    assert "coop" not in ctx.kernel_name and (not twin or ctx.kernel_name.endswith(twin)), ctx.kernel_name
    return ctx


def _counted():
    """Whether the library has the counter (always, unless an older library is loaded through TRPO_LIB)."""
    return hasattr(trpo_amd.lib(), "trpo_ctx_forward_passes") or not os.environ.get("TRPO_LIB")


def _passes(ctx):
    return ctx.forward_passes if _counted() else 0


def _rose(ctx, before, by):
    if _counted():
        assert ctx.forward_passes - before == by, (ctx.forward_passes, before, by)


def _solve(ctx, b, m):
    x = ctx.cg(B[b], m, 0.0)
    rr, xn, it = ctx.cg_history()
    return x, np.array(rr), np.array(xn), it


def _fresh(acts, n, twin, th, b, m):
    """The solve of b on a context that ran nothing else, computed once per case."""
    key = (acts, n, twin, th, b, m)
    if key not in _FRESH:
        with _ctx(acts, n, twin, th) as ctx:
            _FRESH[key] = _solve(ctx, b, m)
    return _FRESH[key]


def _same(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def _oracle(acts, n, b, m):
    if (acts, n, b, m) not in _REF:
        _REF[acts, n, b, m] = oracle.cg(L, acts, TH[0], _obs(n), STD, B[b], m, 0.0)["x"]
    return _REF[acts, n, b, m]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("twin", list(TWINS))
@pytest.mark.parametrize("acts", NETS)
def test_solve_then_solve(acts, twin, n, monkeypatch):
    """A second solve with another b runs K_0 on the cache the first one wrote: a fresh context's bits, one
    forward pass over the two solves, and the fp64 oracle's x within the parity bound."""
    _env(monkeypatch, twin)
    for m in (1, 3, 10):
        with _ctx(acts, n, twin) as ctx:
            c0 = _passes(ctx)
            _same(_solve(ctx, 0, m), _fresh(acts, n, twin, 0, 0, m))
            second = _solve(ctx, 1, m)
            _rose(ctx, c0, 1)
        _same(second, _fresh(acts, n, twin, 0, 1, m))
        assert second[3] == m
    ex = cases.rel_l2(second[0], _oracle(acts, n, 1, 10))
    print("%s %s N %d second solve: CG relL2 %.3e" % (acts, twin, n, ex))
    assert ex <= CG_TOL


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("acts", NETS)
def test_fvp_then_solve_then_fvp(acts, n, monkeypatch):
    """FVP -> solve and solve -> FVP(x) each share one forward pass."""
    _env(monkeypatch, None)
    with _ctx(acts, n) as ctx:
        z_first = ctx.fvp(V)
    with _ctx(acts, n) as ctx:
        c0 = _passes(ctx)
        np.testing.assert_array_equal(ctx.fvp(V), z_first)
        got = _solve(ctx, 0, 10)
        _rose(ctx, c0, 1)
        _same(got, _fresh(acts, n, None, 0, 0, 10))
    x = got[0]
    with _ctx(acts, n) as ctx:
        z_fresh = ctx.fvp(x)
    with _ctx(acts, n) as ctx:
        c0 = _passes(ctx)
        np.testing.assert_array_equal(ctx.cg(B[0], 10, 0.0), x)
        np.testing.assert_array_equal(ctx.fvp(x), z_fresh)
        _rose(ctx, c0, 1)


@pytest.mark.parametrize("acts", NETS)
def test_set_theta_and_set_obs_between_solves(acts, monkeypatch):
    """New parameters or new observations (257 -> 517 samples) make the cache stale: the next solve
    recomputes, and has the bits of a fresh context on the new inputs."""
    _env(monkeypatch, None)
    with _ctx(acts, 257) as ctx:
        c0 = _passes(ctx)
        _solve(ctx, 0, 10)
        ctx.set_theta(TH[1])
        got = _solve(ctx, 1, 10)
        _rose(ctx, c0, 2)
    _same(got, _fresh(acts, 257, None, 1, 1, 10))
    with _ctx(acts, 257) as ctx:
        c0 = _passes(ctx)
        _solve(ctx, 0, 10)
        ctx.set_obs(_obs(517))
        got = _solve(ctx, 1, 10)
        _rose(ctx, c0, 2)
    _same(got, _fresh(acts, 517, None, 0, 1, 10))


def _updates(acts, n):
    """Two consecutive updates (theta installed between them when the first is accepted):
    [(theta, x, b, accepted, rdotr history, |x| history, iterations)], forward passes per update."""
    out, passes = [], []
    th = TH[0].copy()
    std = np.ones(L[-1])                               # sigma of theta's LogStd = 0: the full step is accepted
    with trpo_amd.Context(L, acts, th, _obs(n), std, 0.1) as ctx:
        for _ in range(2):
            mean, action, adv = synth.make_rollout(L, acts, th, _obs(n), std)
            ctx.set_rollout(mean, action, adv)
            c0 = _passes(ctx)
            r = ctx.update()
            passes.append(_passes(ctx) - c0)
            rr, xn, it = ctx.cg_history()
            out.append((r["theta"], r["x"], r["b"], r["accepted"], np.array(rr), np.array(xn), it))
            if r["accepted"] >= 0:
                th = r["theta"]
                ctx.set_theta(th)
    return out, passes


@pytest.mark.parametrize("twin", list(TWINS))
@pytest.mark.parametrize("acts", NETS)
def test_update_runs_the_forward_pass_once(acts, twin, monkeypatch):
    """update(): the policy gradient writes the cache, the solve's K_0 and FVP(x) read it -- one forward
    pass per update, and the bits of a context that never uses the cache (TRPO_YCACHE=0 at creation)."""
    _env(monkeypatch, twin)
    monkeypatch.setenv("TRPO_YCACHE", "0")
    want, _ = _updates(acts, 257)
    monkeypatch.delenv("TRPO_YCACHE")
    got, passes = _updates(acts, 257)
    for g, w in zip(got, want):
        _same(g, w)
    print("%s %s accepted %s" % (acts, twin, [g[3] for g in got]))
    assert got[0][3] >= 0                              # the first update is accepted: the second runs on a new theta
    if _counted():
        assert passes == [1, 1], passes


@pytest.mark.parametrize("acts", NETS)
def test_forced_graph_form(acts, monkeypatch):
    """TRPO_CG_GRAPH=1: one captured graph per form of K_0, picked per call from the cache's validity -- a
    replay never runs the cached K_0 on a stale cache.  solve, solve, set_theta, solve, solve."""
    _env(monkeypatch, None)
    monkeypatch.setenv("TRPO_CG_GRAPH", "1")
    rose = []
    with _ctx(acts, 257) as ctx:
        for th, b in ((0, 0), (0, 1), (1, 0), (1, 1)):
            if (th, b) == (1, 0):
                ctx.set_theta(TH[1])
            c0 = _passes(ctx)
            got = _solve(ctx, b, 10)
            rose.append(_passes(ctx) - c0)
            monkeypatch.delenv("TRPO_CG_GRAPH")
            _same(got, _fresh(acts, 257, None, th, b, 10))       # its eager counterpart
            monkeypatch.setenv("TRPO_CG_GRAPH", "1")
    if _counted():
        assert rose == [1, 0, 1, 0], rose


def test_parent_bits_second_solve(monkeypatch):
    """x for N = 517 after 3, 7 and 10 iterations of a SECOND solve (K_0 on the cache) equals the bits
    tests/golden/basis_slots_x.txt records (lines `maxiter hex-double`)."""
    _env(monkeypatch, None)
    want = {m: [] for m in GOLDEN_MAXITERS}
    with open(GOLDEN) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                m, h = line.split()
                want[int(m)].append(float.fromhex(h))
    with _ctx("lttl", GOLDEN_N) as ctx:
        _solve(ctx, 1, 10)
        for m in GOLDEN_MAXITERS:
            c0 = _passes(ctx)
            np.testing.assert_array_equal(ctx.cg(B[0], m, 0.0), np.array(want[m]), err_msg="maxiter %d" % m)
            _rose(ctx, c0, 0)
