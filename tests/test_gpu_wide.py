"""The wide-policy solver path (trpo_ctx_create_wide, Context(form="wide")) against the clean-room
oracle: FVP, 10-iteration CG and the full update on small shapes forced onto the path -- widths at and one
past the 16-wide tile edges, depths 3 to 5, one output, sample counts that are no multiple of 16, sigma != 1,
non-zero biases and LogStd -- and on 376-128-64-17 (57 634 parameters, past the default solver's 32 768), there
also through the file entry points FVPFast and CG.  Then the sample-split edges (one row short of, at and one
past the layer kernels' 64-row tile and the contraction's 512-sample split; one sample), bitwise
repeatability, the forward cache's discipline and the refusals.

Tolerances are the project's own (tests/test_gpu_random_shapes.py): FVP relative L2 <= 1e-5, CG and
update step <= 1e-4; the policy gradient <= 1e-12, the fp64 mode's bound, since b comes from the generic fp64
kernel; equal `accepted` and, with a positive threshold, equal iteration counts.

A condition, not a tolerance.  The wide path never re-solves in fp64 (there is no fp64 twin of it), so every
CG / update case is one whose reference is not a stalled solve: the reference's recurrence on the oracle
(tools/diag/ritz_probe.py's computation, run over this table by tools/diag/wide_ritz.py) keeps its smallest
relative Ritz residual >= 1e-13, ten times the guard's threshold.  With synth.make_obs's narrow observations a
policy with few outputs fails that at every seed (F is 0.1 I plus about 2 A large eigenvalues and ten
iterations converge to rounding: 40 seeds per shape probed, best 2e-13), so the observations are scaled by
wide_cases.OBS_SCALE and the seeds chosen from the probe.  Probed values, CG (b, threshold 0) / update (policy
gradient, 1e-10):
    one-tile  [15,16,16,3] lttl n=333       2.4e-08 / 6.8e-08
    past-tile [17,33,65,5] ltsl n=1001      1.7e-10 / 3.0e-11
    thin      [3,130,20,1] ltll n=47        8.9e-11 / 5.0e-12
    depth3    [8,24,6] ltl n=200            3.6e-03 / 7.1e-03
    depth5    [6,20,12,9,2] ltstl n=150     3.3e-13 / 1.8e-12   (seed 29: the one of 79 probed above 1e-13)
    humanoid  [376,128,64,17] lttl n=257    2.0e-03 / 1.0e-02
The sample-split edges are compared on the FVP alone (a one-sample Fisher matrix has rank A: its solve
converges to rounding whatever the seed, 8.8e-19).

Every test fails on the parent commit: the entry point does not exist."""
import os

import numpy as np
import pytest

import cases
import oracle
import trpo_amd
import wide_cases as W
from trpo_amd import synth

pytestmark = pytest.mark.gpu

SMALL = [k for k in W.CASES if k != "humanoid"]


def wide_ctx(p, **kw):
    ctx = trpo_amd.Context(p["layers"], p["acts"], p["theta"], p["obs"], p["std"], 0.1, form="wide", **kw)
    name = ctx.kernel_name
    assert name.startswith("wide") and "-".join(str(x) for x in p["layers"]) in name, name
    return ctx


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_solver(name):
    p, ref = W.case(name), W.reference(name)
    what = "%s %s %s n=%d" % (name, p["layers"], p["acts"], p["n"])
    with wide_ctx(p) as ctx:
        z = ctx.fvp(p["v"])
        x = ctx.cg(p["b"], 10, 0.0)
        st = ctx.cg_status()
        ctx.set_rollout(p["mean"], p["action"], p["adv"])
        r = ctx.update()
    u = ref["update"]
    figures = dict(fvp=cases.rel_l2(z, ref["z"]), cg=cases.rel_l2(x, ref["x"]), pg=cases.rel_l2(r["b"], ref["pg"]),
                   step=cases.rel_l2(r["x"], u["x"]), ritz_cg=st["ritz_residual"], ritz_update=r["ritz_residual"])
    print("wide-figures", what, " ".join("%s=%.3e" % kv for kv in figures.items()), flush=True)
    assert figures["fvp"] <= 1e-5, (what, figures)
    assert figures["cg"] <= 1e-4, (what, figures)
    assert not st["fp64_rerun"] and not r["fp64_rerun"], what
    assert figures["pg"] <= 1e-12, (what, figures)
    assert r["accepted"] == u["accepted"], (what, r["accepted"], u["accepted"])
    assert r["cg_iters"] == ref["update_iters"], (what, r["cg_iters"], ref["update_iters"])   # resth = 1e-10 > 0
    assert figures["step"] <= 1e-4, (what, figures)
    if u["accepted"] >= 0:
        assert cases.rel_l2(r["theta"] - p["theta"], u["theta"] - p["theta"]) <= 1e-4, what


@pytest.mark.parametrize("name", SMALL)
def test_small_shapes_forced_onto_the_path(name):
    check_solver(name)


def test_past_the_old_bound():
    assert W.case("humanoid")["P"] == 57634
    check_solver("humanoid")


def test_past_the_old_bound_through_the_file_entry_points(tmp_path, capfd):
    p, ref = W.case("humanoid"), W.reference("humanoid")
    m, d = str(tmp_path / "model.txt"), str(tmp_path / "data.txt")
    synth.write_model_file(m, p["theta"])
    synth.write_data_file(d, p["obs"], p["std"])
    prm = trpo_amd.make_param(m, d, p["layers"], p["acts"], p["n"])
    z, x = np.zeros(p["P"]), np.zeros(p["P"])
    try:
        assert trpo_amd.FVPFast(prm, z, p["v"], 1) >= 0
        assert trpo_amd.CG(prm, x, p["b"], 10, 0.0, 1) >= 0
    finally:
        trpo_amd.cache_clear()
    assert cases.rel_l2(z, ref["z"]) <= 1e-5
    assert cases.rel_l2(x, ref["x"]) <= 1e-4
    assert "CG Iter[10]" in capfd.readouterr().out


@pytest.mark.parametrize("n", W.EDGE_N)
def test_sample_split_edges(n):
    """n around WIDE_TS = 64 (the layer kernels' rows per block) and WIDE_SPLIT = 512 (the contraction's
    samples per block), and n = 1: the padded rows must add nothing, the last block's short range must be
    summed whole"""
    layers, acts, seed = W.EDGE_SHAPE
    p = W.make(layers, acts, n, seed)
    zr, _ = oracle.fvp(layers, acts, p["theta"], p["obs"], p["std"], p["v"])
    with wide_ctx(p) as ctx:
        z = ctx.fvp(p["v"])
        assert ctx.geometry["blocks"] == max(1, -(-(-(-n // W.WIDE_TS) * W.WIDE_TS) // W.WIDE_SPLIT))
    err = cases.rel_l2(z, zr)
    print("wide-figures edge n=%d fvp=%.3e" % (n, err), flush=True)
    assert err <= 1e-5, (n, err)


def test_bitwise_repeatability():
    p = W.case("past-tile")
    runs = []
    for _ in range(2):
        with wide_ctx(p) as ctx:
            z1, z2 = ctx.fvp(p["v"]), ctx.fvp(p["v"])
            x1, x2 = ctx.cg(p["b"], 10, 0.0), ctx.cg(p["b"], 10, 0.0)
            h = ctx.cg_history()
        same_bits(z1, z2)
        same_bits(x1, x2)
        runs.append((z1, x1, h[0]))
    for a, b in zip(*runs):
        same_bits(a, b)


def test_cache_discipline():
    p, q = W.case("past-tile"), W.case("one-tile")
    layers, acts, seed = W.CASES["past-tile"][0], W.CASES["past-tile"][1], 11
    other = W.make(layers, acts, 130, seed)                      # another theta, another n
    with wide_ctx(p) as ctx:
        f0 = ctx.forward_passes
        z = ctx.fvp(p["v"])
        assert ctx.forward_passes == f0 + 1
        same_bits(ctx.fvp(p["v"]), z)
        assert ctx.forward_passes == f0 + 1                     # the second FVP runs on the cache
        ctx.cg(p["b"], 10, 0.0)
        assert ctx.forward_passes == f0 + 1                     # and so does a solve
        ctx.set_theta(other["theta"])
        z_theta = ctx.fvp(p["v"])
        assert ctx.forward_passes == f0 + 2
        ctx.set_obs(other["obs"])
        z_obs = ctx.fvp(p["v"])
        assert ctx.forward_passes == f0 + 3
    fresh = dict(p, theta=other["theta"])
    with wide_ctx(fresh) as ctx:
        same_bits(ctx.fvp(p["v"]), z_theta)
    fresh = dict(fresh, obs=other["obs"])
    with wide_ctx(fresh) as ctx:
        same_bits(ctx.fvp(p["v"]), z_obs)
    # an accepted update moves theta on the host side only: the context keeps its own until set_theta, and the
    # caller's set_theta(theta_out) -- the accepted step -- invalidates the cache
    with wide_ctx(q) as ctx:
        ctx.set_rollout(q["mean"], q["action"], q["adv"])
        r = ctx.update()
        assert r["accepted"] >= 0
        f1 = ctx.forward_passes
        ctx.set_theta(r["theta"])
        z_new = ctx.fvp(q["v"])
        assert ctx.forward_passes == f1 + 1
    with wide_ctx(dict(q, theta=r["theta"])) as ctx:
        same_bits(ctx.fvp(q["v"]), z_new)


def test_refusals():
    p = W.case("one-tile")
    L = trpo_amd.lib()
    with wide_ctx(p) as ctx, trpo_amd.Group(1) as grp:
        for call in (lambda: ctx.attach_comm(0, 1, b"\0" * 128), lambda: ctx.attach_group(grp, 0),
                     lambda: ctx.peer_handle(), lambda: ctx.attach_peers(0, 1, [b"\0" * trpo_amd.PEER_HANDLE_BYTES]),
                     lambda: ctx.enqueue_fvp_kernel()):
            with pytest.raises(trpo_amd.TRPOError) as e:
                call()
            assert "wide-policy path" in str(e.value), str(e.value)
        ctx.upload_v(p["v"])
        assert L.trpo_ctx_enqueue_fvp_kernel_only(ctx._h) == -1
        assert L.trpo_ctx_time(ctx._h, 0, 1, 10, 0.0) == -1.0
        assert ctx.time_ms(1, 2) > 0 and ctx.time_ms(2, 2, 10, 0.0) > 0          # the timers it serves
        z = ctx.fvp(p["v"])                                                      # and it goes on working
    assert cases.rel_l2(z, W.reference("one-tile")["z"]) <= 1e-5
    with pytest.raises(trpo_amd.TRPOError) as e:
        trpo_amd.Context(p["layers"], p["acts"], p["theta"], p["obs"], p["std"], 0.1, form="wide", precision="fp64")
    assert "wide-policy path" in str(e.value) and "fp64" in str(e.value), str(e.value)
    assert os.environ.get("TRPO_PRECISION") is None or os.environ["TRPO_PRECISION"] != "fp64"
    h = W.case("humanoid")
    with trpo_amd.Context(h["layers"], h["acts"], h["theta"], h["obs"][:16], h["std"], 0.1) as ctx:
        assert not ctx.kernel_name.startswith("wide")
        with pytest.raises(trpo_amd.TRPOError) as e:
            ctx.fvp(h["v"])
        assert "inference only" in str(e.value) and "57634" in str(e.value), str(e.value)
