"""MI355X: the CG step's load round on padded, zero-kept rows.

On the pair layout (P <= 1 024) every P-vector the step's load round reads -- the replica sets, p, r, x, the
fp32 basis, the slot map -- has a row stride of whole 128-element wave rows, and the padding holds zeros (the
slot map: -1) from allocation on.  The loads of the waves that hold elements therefore carry no clamped index
and the loaded values no select against zero: the replica sum runs over all RMAX rows (unused rows exist and
stay zero), a stored basis vector's padding is zero (a slot beyond nq still selects a stored vector away), and
the reduction of 9 .. 12 sums is 12 wide.  None of this may change a bit.  What it can get wrong: a stride
that is not the one the buffers were allocated with; padding dirtied by set_theta, set_damping, upload_b, a
standalone FVP, a solve that stopped early or an update; an unused replica row that is not zero; a
half-valid last pair (odd P); padding of nearly a whole wave row (P = 258) or of one element (P = 383); a sum
read from the wrong column of the 12-wide reduction.

Every solve is compared three ways: bit for bit with the same solve under TRPO_YCACHE=0 (MODE 0 with the
streaming basis dots, which shares the step's source), bit for bit with what the commit before the change
gave (tests/golden/step_trim_solves.txt: the iteration count, both history columns as hex doubles and the
SHA-256 of x's little-endian bytes; tools/record_step_trim.py wrote it from that commit's library), and
x <= 1e-4 against the fp64 oracle up to 10 iterations (test_gpu_parity.py's bound).  Of a solve that stopped
before maxiter on a non-positive |r|^2 that final |r|^2 is left out of the TRPO_YCACHE=0 comparison, as in
tests/test_gpu_step_sums.py.  maxiter 1, 2, 6, 7, 8, 10 (damping 0.1) end on steps holding nq = 0, 1, 5, 6, 7, 9
vectors and run every smaller one on the way; 17 (damping 0.01) ends on 16: every reduction width (4, 8, 12,
16, 32) and the move from the exact-QB kernels to QB 16.  Grids as tests/test_gpu_step_sums.py forces them:
default (the five-wide kernels at these sizes), one block (3 + QB sums, publisher = only block), two blocks at
517 (3 + QB sums with a block that does not publish).  All solves are the fp32 solve (TRPO_RITZ_RERUN=0).
The register-resident shape besides (1, 1, 1, 1) is (2, 1, 1, 1), here [20, 16, 16, 3]: strided step, rungs
with empty slots at maxiter 6 and 7, the padded stride in its last step ([15, 32, 16, 3] runs the cooperative
kernel, which has no cached-forward CG kernels).  The solve that stops early does so at iteration 3 at damping
0.1; at 0.01 |r|^2 of these inputs rises above its start first and no threshold stops it there.
"""
import contextlib
import hashlib
import os

import numpy as np
import pytest

import cases
import oracle
import trpo_amd
from trpo_amd import synth

pytestmark = pytest.mark.gpu

CG_TOL = 1e-4                                         # test_gpu_parity.py's
ACTS = "lttl"
STD = np.array([0.7, 1.0, 1.4])
NETS = {
    "arm": ([15, 16, 16, 3], 582),                    # armDOF_0: 70 elements short of five wave rows
    "odd": ([15, 13, 15, 3], 469),                    # odd P: the last pair is half valid
    "above": ([11, 8, 13, 3], 258),                   # two above a multiple of 128: 126 elements of padding
    "below": ([11, 13, 13, 3], 383),                  # one below a multiple of 128: one element of padding
    "in20": ([20, 16, 16, 3], 662),                   # the other register-resident shape, (2, 1, 1, 1): strided
}
MAXITERS = (1, 2, 6, 7, 8, 10)                        # damping 0.1
LONG, LONG_DAMPING = 17, 0.01                         # all 17 steps run, the last holds 16 vectors
GRIDS = ((17, 0), (257, 0), (517, 0), (517, 1), (517, 2))      # (samples, TRPO_FVP_BLOCKS; 0: default)
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "step_trim_solves.txt")
GOLDEN_UPDATE = os.path.join(HERE, "golden", "step_trim_update.txt")


def _case(net, n, blocks, env=(), solves=tuple((m, 0.1) for m in MAXITERS) + ((LONG, LONG_DAMPING),)):
    return dict(net=net, n=n, blocks=blocks, env=dict(env), solves=tuple(solves))


CASES = {}
for _net in ("arm", "odd", "above", "below"):
    for _n, _b in GRIDS:
        CASES["%s-n%d-b%d" % (_net, _n, _b)] = _case(_net, _n, _b)
for _b in (0, 1):                                     # the rungs {0, 4, 8, 16}: slots beyond nq at nq 5 and 6
    CASES["in20-n257-b%d" % _b] = _case("in20", 257, _b, solves=((6, 0.1), (7, 0.1), (10, 0.1)))
for _r in (1, 4):                                     # unused replica rows
    for _b in (0, 2):
        CASES["arm-n517-b%d-replicas%d" % (_b, _r)] = _case("arm", 517, _b, env={"TRPO_REPLICAS": str(_r)})
for _b in (0, 2):
    CASES["arm-n517-b%d-noreorth" % _b] = _case("arm", 517, _b, env={"TRPO_CG_REORTH": "0"},
                                                solves=tuple((m, 0.1) for m in MAXITERS))

_REF = {}
_GOLD = {}


@contextlib.contextmanager
def environment(env):
    """os.environ with env set (None: unset) for the block; TRPO_RITZ_RERUN=0 always."""
    env = dict(env, TRPO_RITZ_RERUN="0")
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def problem(net, n, seed=synth.SEED):
    layers, P = NETS[net]
    assert synth.num_params(layers) == P
    return layers, synth.make_theta(layers, seed), synth.make_obs(n, layers[0]), synth.make_b(P)


def _take(ctx, x):
    rr, xn, it = ctx.cg_history()
    return x, np.array(rr), np.array(xn), it


def run_case(case, ycache=True):
    """The case's solves: those of one damping in a row on one context, [(x, |r|^2 history, ||x|| history,
    iterations)] in the order of case["solves"]."""
    layers, th, obs, b = problem(case["net"], case["n"])
    env = dict(case["env"], TRPO_FVP_BLOCKS=str(case["blocks"]) if case["blocks"] else None,
               TRPO_YCACHE=None if ycache else "0")
    out = {}
    with environment(env):
        for damping in sorted({d for _, d in case["solves"]}):
            with trpo_amd.Context(layers, ACTS, th, obs, STD, damping) as ctx:
                assert "coop" not in ctx.kernel_name, ctx.kernel_name
                for m, d in case["solves"]:
                    if d == damping:
                        out[m, d] = _take(ctx, ctx.cg(b, m, 0.0))
    return [out[s] for s in case["solves"]]


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype="<f8").tobytes()).hexdigest()


def golden_lines(key, solves, results):
    """The lines of one case in the golden file: `key maxiter column value`."""
    lines = []
    for (m, _), (x, rr, xn, it) in zip(solves, results):
        lines.append("%s %d it %d" % (key, m, it))
        lines.append("%s %d xsha %s" % (key, m, digest(x)))
        lines += ["%s %d rr %s" % (key, m, float(v).hex()) for v in rr]
        lines += ["%s %d xn %s" % (key, m, float(v).hex()) for v in xn]
    return lines


def _golden(path):
    if path not in _GOLD:
        g = {}
        with open(path) as f:
            for line in f:
                if line.strip() and not line.startswith("#"):
                    key, m, col, v = line.split()
                    g.setdefault((key, int(m)), {}).setdefault(col, []).append(v)
        _GOLD[path] = g
    return _GOLD[path]


def _oracle(net, n, m):
    if (net, n, m) not in _REF:
        layers, th, obs, b = problem(net, n)
        _REF[net, n, m] = oracle.cg(layers, ACTS, th, obs, STD, b, m, 0.0)
    return _REF[net, n, m]


def _same_solve(got, want, m):
    (x, rr, xn, it), (x0, rr0, xn0, it0) = got, want
    assert it == it0 <= m
    keep = it + 1 if it == m or rr0[-1] > 0.0 else it
    np.testing.assert_array_equal(x, x0, err_msg="x, maxiter %d" % m)
    np.testing.assert_array_equal(rr[:keep], rr0[:keep], err_msg="|r|^2 history, maxiter %d" % m)
    np.testing.assert_array_equal(xn, xn0, err_msg="||x|| history, maxiter %d" % m)


def _same_as_golden(path, key, m, got):
    x, rr, xn, it = got
    want = _golden(path)[key, m]
    assert [str(it)] == want["it"], (key, m, it, want["it"])
    assert [float(v).hex() for v in rr] == want["rr"], (key, m, "|r|^2 history")
    assert [float(v).hex() for v in xn] == want["xn"], (key, m, "||x|| history")
    assert [digest(x)] == want["xsha"], (key, m, "x")


@pytest.mark.parametrize("key", list(CASES))
def test_trim_bits(key):
    case = CASES[key]
    stream = run_case(case, ycache=False)
    cached = run_case(case)
    for (m, damping), want, got in zip(case["solves"], stream, cached):
        _same_solve(got, want, m)
        _same_as_golden(GOLDEN, key, m, got)
        if m <= 10:
            assert damping == 0.1
            ref = _oracle(case["net"], case["n"], m)
            ex = cases.rel_l2(got[0], ref["x"])
            print("%s maxiter %d: %d iterations, CG relL2 %.3e" % (key, m, got[3], ex))
            assert ex <= CG_TOL
            assert got[3] == ref["iters"] == m
        else:
            assert got[3] == m


def _early_resth(layers, th, obs, b):
    """A residual threshold that stops the 10-iteration solve at damping 0.1 at iteration 3: below |r|^2 of
    iterations 0 .. 2, above that of iteration 3 (taken from the solve itself, on a context of its own)."""
    with trpo_amd.Context(layers, ACTS, th, obs, STD, 0.1) as ctx:
        ctx.cg(b, 10, 0.0)
        rr = np.array(ctx.cg_history()[0])
    lo, hi = rr[3], min(rr[:3])
    assert 0.0 < lo < hi, rr[:4]
    return float(np.sqrt(lo * hi))


def sequence(net, n, blocks, fresh):
    """Solves of 3, 10, 1, 7 and 17 iterations (damping 0.01) with set_theta, upload_b, a standalone FVP and a
    solve stopped at iteration 3 (at damping 0.1, where |r|^2 falls below its start by then: set_damping)
    between them -- on one context, or (fresh) each on a context of its own."""
    layers, th0, obs, b0 = problem(net, n)
    th1, b1 = synth.make_theta(layers, synth.SEED + 1), synth.make_b(NETS[net][1], synth.SEED + 1)
    v = synth.make_v(NETS[net][1])
    out = []
    with environment({"TRPO_FVP_BLOCKS": str(blocks) if blocks else None}):
        resth = _early_resth(layers, th0, obs, b0)
        ctx = None

        def context(th, damping=LONG_DAMPING):
            nonlocal ctx
            if ctx is None or fresh:
                if ctx is not None:
                    ctx.close()
                ctx = trpo_amd.Context(layers, ACTS, th, obs, STD, damping)
            else:
                ctx.set_theta(th)
                ctx.set_damping(damping)
            return ctx

        try:
            out.append(_take(context(th0), ctx.cg(b0, 3, 0.0)))
            out.append(_take(context(th1), ctx.cg(b0, 10, 0.0)))          # after set_theta
            if not fresh:
                ctx.upload_b(b1)                                            # b rewritten
            out.append(_take(context(th1), ctx.cg(b1, 1, 0.0)))
            if not fresh:
                ctx.fvp(v)                                                  # the standalone FVP's replica sets
            out.append(_take(context(th1), ctx.cg(b0, 7, 0.0)))
            out.append(_take(context(th0, 0.1), ctx.cg(b0, 10, resth)))    # stops at iteration 3
            assert out[-1][3] == 3, out[-1][3]
            out.append(_take(context(th0), ctx.cg(b1, LONG, 0.0)))         # 16 basis vectors after 3
        finally:
            if ctx is not None:
                ctx.close()
    return out


@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("net", ["arm", "odd"])
def test_padding_stays_clean(net, blocks):
    """Whatever ran before on the context, a solve has a fresh context's bits."""
    row, alone = sequence(net, 257, blocks, False), sequence(net, 257, blocks, True)
    for m, got, want in zip((3, 10, 1, 7, 10, LONG), row, alone):
        _same_solve(got, want, m)
        np.testing.assert_array_equal(got[1], want[1])


def updates(net, n):
    """Three updates in a row on one context (sigma = 1: the full step is accepted), theta set to each result:
    [(theta, x, b, accepted)]."""
    layers, th, obs, _ = problem(net, n)
    std = np.ones(layers[-1])
    out = []
    with environment({}):
        with trpo_amd.Context(layers, ACTS, th, obs, std, 0.1) as ctx:
            for k in range(3):
                mean, action, adv = synth.make_rollout(layers, ACTS, th, obs, std, synth.SEED + k)
                ctx.set_rollout(mean, action, adv)
                r = ctx.update()
                out.append((r["theta"], r["x"], r["b"], r["accepted"]))
                if r["accepted"] >= 0:
                    th = r["theta"]
                    ctx.set_theta(th)
    return out


def update_lines(key, results):
    lines = []
    for k, (th, x, b, acc) in enumerate(results):
        lines.append("%s %d accepted %d" % (key, k, acc))
        for col, v in (("theta", th), ("x", x), ("b", b)):
            lines.append("%s %d %ssha %s" % (key, k, col, digest(v)))
    lines += ["%s 2 theta %s" % (key, float(v).hex()) for v in results[2][0]]
    return lines


UPDATE_CASES = {"arm-n517": ("arm", 517), "odd-n257": ("odd", 257)}


@pytest.mark.parametrize("key", list(UPDATE_CASES))
def test_update_sequence_parent_bits(key):
    """theta, x and b of three updates in a row equal what the commit before the change gave."""
    got = updates(*UPDATE_CASES[key])
    gold = _golden(GOLDEN_UPDATE)
    for k, (th, x, b, acc) in enumerate(got):
        want = gold[key, k]
        assert [str(acc)] == want["accepted"] and acc >= 0
        for col, v in (("theta", th), ("x", x), ("b", b)):
            assert [digest(v)] == want[col + "sha"], (key, k, col)
    assert [float(v).hex() for v in got[2][0]] == gold[key, 2]["theta"]
