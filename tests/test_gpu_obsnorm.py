"""MI355X tests of the observation filter (trpo_ctx_obsnorm_*; include/trpo_mi355x.h "The observation filter",
DESIGN §5.14).

The normalised path is held bit for bit: a context WITHOUT the filter, fed rows normalised in numpy with the pair
the device derived (tests/obsnorm_ref.py: the contract's operations in the contract's order), must give the same
mean, action, logp and the same update.  The statistics are held to 1e-12, per element and relative to the
long-double reference's own value, on rows whose column k has offset 10^(k mod 4) and spread 10^(-2 + k mod 5)
(tests/test_obsnorm_abi.py shows a one-pass sum of squares losing six digits on them); counts are exact.

Shapes: 3-8-2 and 70-16-3 (L0 = 70 crosses the 64-lane stride of the neuron form's observation load and of the
statistics kernel's column blocks), 376-128-64-17 whose lane form keeps its rows in the global scratch;
m in {1, 5, 65, 130}: a tail of the neuron form's 4-row blocks, a tail of the lane form's 64-row pass and of the
statistics' 64-row chunk, a second pass / a third chunk.
"""
import functools

import numpy as np
import pytest

import obsnorm_ref as N
import test_gpu_devloop as D
import test_gpu_record as R
import trpo_amd
from trpo_amd import devmem

pytestmark = pytest.mark.gpu

SEED = R.SEED
S3 = ((3, 8, 2), "ltl")
S70 = ((70, 16, 3), "ltl")
SCRATCH = ((376, 128, 64, 17), "lttl")
SHAPES = {"3-8-2": S3, "70-16-3": S70, "376-128-64-17": SCRATCH}
MS = (1, 5, 65, 130)
FORMS = ("lane", "neuron")
CLIP, EPS = 1.5, 1e-3
TOL = 1e-12


def test_the_scratch_shape_is_one():
    """the lane form keeps 8 * rows * 65 bytes of activations per block in LDS while they fit 160 KiB"""
    assert 8 * sum(SCRATCH[0]) * 65 > 160 * 1024 >= 8 * sum(S70[0]) * 65


@functools.lru_cache(maxsize=None)
def problem(L0):
    """live statistics to restore and 130 rows around them of 1.5 x their spread: by the normal law 32 % of the
    elements then lie beyond clip = 1.5 after the filter"""
    rng = np.random.default_rng(40 + L0)
    count = 50.0
    mean, std = rng.normal(size=L0), rng.uniform(0.5, 2.0, L0)
    m2 = (count - 1.0) * std * std
    obs = mean + 1.5 * std * rng.normal(size=(max(MS), L0))
    for a in (mean, m2, obs):
        a.setflags(write=False)
    return count, mean, m2, obs


def rows_of(m):
    """(row0, row_stride) of the calls with m rows: strided for m = 65"""
    return (3, 2) if m == 65 else (0, 1)


def same3(got, want, what):
    for g, w, name in zip(got, want, ("mean", "action", "logp")):
        R.same_bits(g, w, "%s: %s" % (what, name))


# ---- 1. identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ("3-8-2", "70-16-3"))
def test_enabled_and_nothing_folded_is_the_plain_path(name, form):
    shape = SHAPES[name]
    obs = problem(shape[0][0])[3]
    with R.context(shape, R.old_batch(shape), act_form=form) as a, R.context(shape, R.old_batch(shape),
                                                                            act_form=form) as b:
        a.obsnorm_enable(float("inf"), EPS)                         # the identity pair; nothing to clip
        st = a.obsnorm_state()
        assert st["count"] == 0 and not st["shift"].any() and np.array_equal(st["scale"], np.ones(shape[0][0]))
        for m in MS:
            row0, stride = rows_of(m)
            want = b.act(obs[:m], SEED, 3, row0=row0, row_stride=stride)
            same3(a.act(obs[:m], SEED, 3, row0=row0, row_stride=stride), want, "act m=%d" % m)
            a.record_begin(row0 + stride * m)
            same3(a.act_record(obs[:m], SEED, 3, row0=row0, row_stride=stride), want, "act_record m=%d" % m)
            same3(D.act_dev_call(a, obs[:m], np.float64, row0, stride), want, "act_dev m=%d" % m)


# ---- 2. the fused normalise ---------------------------------------------------------------------------------
def restored(ctx, L0):
    """enable, restore problem(L0)'s statistics, return the device's pair after checking it against numpy"""
    count, mean, m2, _ = problem(L0)
    ctx.obsnorm_enable(CLIP, EPS)
    ctx.obsnorm_set_state(count, mean, m2)
    st = ctx.obsnorm_state()
    assert st["count"] == count
    R.same_bits(st["mean"], mean, "mean")
    R.same_bits(st["m2"], m2, "m2")
    R.same_bits(st["shift"], mean, "shift")
    want = N.derived(count, mean, m2, EPS)[1]
    assert np.all(np.abs(st["scale"] - want) <= 4 * np.spacing(want)), "scale beyond 4 ulp"
    return st["shift"], st["scale"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_filtered_calls_are_the_plain_calls_on_normalised_rows(name, form):
    shape = SHAPES[name]
    L0 = shape[0][0]
    obs = problem(L0)[3]
    batch = R.draws(3 + 2 * max(MS), L0, 5)                         # every row a keep = 1 call touches is below n
    with R.context(shape, batch, act_form=form) as a, R.context(shape, batch, act_form=form) as b:
        shift, scale = restored(a, L0)
        clipped = np.mean(np.abs((obs - shift) * scale) > CLIP)
        assert 0.1 <= clipped <= 0.9, clipped
        for dtype in (np.float64, np.float32):
            raw = obs.astype(dtype)
            norm = N.normalise(raw, shift, scale, CLIP)             # of the widened values
            assert np.any(np.abs(norm) == CLIP) and np.any(np.abs(norm) < CLIP)
            for m in MS:
                row0, stride = rows_of(m)
                want = b.act(norm[:m], SEED, 3, row0=row0, row_stride=stride)
                for rec in (False, True):
                    if rec:
                        a.record_begin(row0 + stride * m)
                    got = D.act_dev_call(a, raw[:m], dtype, row0, stride, record=rec)
                    for g, w, what in zip(got, want, ("mean", "action", "logp")):
                        D.same_out(g, w, dtype, "%s m=%d rec=%d" % (what, m, rec))
                if dtype == np.float32:
                    continue
                same3(a.act(raw[:m], SEED, 3, row0=row0, row_stride=stride), want, "act m=%d" % m)
                same3(a.act(raw[:m], SEED, 3, row0=row0, row_stride=stride, keep=True), want, "keep m=%d" % m)
                a.record_begin(row0 + stride * m)
                same3(a.act_record(raw[:m], SEED, 3, row0=row0, row_stride=stride), want, "act_record m=%d" % m)
                R.same_bits(a.act(raw[:m], SEED, 3, sample=False)[0], b.act(norm[:m], SEED, 3, sample=False)[0],
                            "means only")


@pytest.mark.parametrize("form", FORMS)
def test_split_launch_gives_the_fused_bits(form):
    """the normalise as a launch of its own (obsnorm_apply_dev into a device array) in front of the plain kernels
    of a context without the filter: the bits of the fused normalise on the raw rows"""
    L0 = S70[0][0]
    obs = problem(L0)[3]
    with R.context(S70, R.old_batch(S70), act_form=form) as a, R.context(S70, R.old_batch(S70), act_form=form) as b, \
            R.context(S70, R.old_batch(S70), act_form=form) as c:
        restored(a, L0)
        restored(b, L0)
        A, d_raw, d_applied = S70[0][-1], D.dev(obs), devmem.DeviceArray(obs.shape, np.float64, 0)
        b.obsnorm_apply_dev(d_raw, d_applied)
        b.synchronize()
        for ctx in (a, c):
            ctx.record_begin(max(MS))
        for m in MS:
            out = []
            for ctx, rows in ((a, d_raw), (c, d_applied)):
                d_out = [devmem.DeviceArray(shape, np.float64, 0) for shape in ((m, A), (m, A), (m,))]
                ctx.act_record_dev(rows.view(0, (m, L0)), *d_out, seed=SEED, step=3)
                ctx.synchronize()
                out.append([d.to_host() for d in d_out])
            same3(out[0], out[1], "m=%d" % m)
        applied = d_applied.to_host()
        for ctx in (a, c):
            ctx.record_commit()
        same3(a.act(obs[:9], SEED, 1), c.act(applied[:9], SEED, 1), "act after the commit")


# ---- 3. the record holds what the policy saw -----------------------------------------------------------------
@pytest.mark.parametrize("kind,path", [("default", "host"), ("default", "dev"), ("wide", "host"), ("wide", "dev32"),
                                       ("inference", "host")])
def test_commit_after_filtered_record_is_set_obs_of_normalised_rows(kind, path):
    k = D.RECORD_KINDS[kind]
    shape = k["shape"]
    L0, num_ep, ep_len = shape[0][0], 5, 27                         # 5-row calls; 135 rows: a third 64-row pass
    n = num_ep * ep_len
    count, mean, m2, _ = problem(L0)
    rng = np.random.default_rng(77)
    dtype = np.float32 if path == "dev32" else np.float64
    raw = (mean + 1.5 * np.sqrt(m2 / (count - 1.0)) * rng.normal(size=(n, L0))).astype(dtype)
    with R.context(shape, R.old_batch(shape), **k["kw"]) as a, R.context(shape, R.old_batch(shape), **k["kw"]) as b:
        shift, scale = restored(a, L0)
        norm = N.normalise(raw, shift, scale, CLIP)
        a.record_begin(n)
        if path == "host":
            got = R.record_steps(a, raw, num_ep, ep_len, step_of=lambda t: 7)
        else:
            ep = raw.reshape(num_ep, ep_len, -1)
            for t in range(ep_len):
                D.act_dev_call(a, ep[:, t], dtype, t, ep_len, step=7, record=True)
        a.record_commit()
        b.set_obs(norm)
        if kind == "inference":
            same3(got, b.act(norm, SEED, 7), "recorded outputs")
            same3(a.act(raw[:9], SEED, 1), b.act(norm[:9], SEED, 1), "act after the commit")
            return
        want = b.act(norm, SEED, 7, keep=True)
        if path == "host":
            same3(got, want, "recorded outputs")
        adv = R.draws(n, 1, 21).reshape(-1)
        for c in (a, b):
            c.set_rollout_acted(adv=adv)
        R.same_update(a.update(), b.update())


# ---- 4. statistics -------------------------------------------------------------------------------------------
SEQ_A, SEQ_B = (1, 5, 130), (65, 5)
SEQ_ROWS = sum(SEQ_A) + sum(SEQ_B)


def sequence_rows(dtype):
    return N.ill_conditioned(SEQ_ROWS, S70[0][0]).astype(dtype)


def record_call(ctx, rows, path, dtype, row0):
    if path == "host":
        ctx.act_record(rows.astype(np.float64), SEED, 1, row0=row0)
    else:
        D.act_dev_call(ctx, rows, dtype, row0, 1, step=1, record=True)


def snapshot(ctx):
    p, l = ctx.obsnorm_state(pending=True), ctx.obsnorm_state()
    return tuple(np.concatenate([[s["count"]], s["mean"], s["m2"]]) for s in (p, l)) + (l["shift"], l["scale"])


@functools.lru_cache(maxsize=None)
def run_sequence(form, path, rep=0):
    """three record calls, a fold, two more calls on 70-16-3: the states at the three points the test looks, plus
    what the side calls must not have changed"""
    dtype = np.float32 if path in ("dev32", "host32") else np.float64          # host32: fp32 values, host calls
    x = sequence_rows(dtype)
    path = "host" if path == "host32" else path
    out = {}
    with R.context(S70, R.old_batch(S70), act_form=form) as ctx:
        ctx.obsnorm_enable(CLIP, EPS)
        ctx.record_begin(SEQ_ROWS)
        ctx.act_record(x[:7].astype(np.float64), SEED, 0)           # a recording that is thrown away ...
        out["discarded"] = snapshot(ctx)
        ctx.record_begin(SEQ_ROWS)                                  # ... leaves no trace
        out["begun"] = snapshot(ctx)
        at = 0
        for m in SEQ_A:
            record_call(ctx, x[at:at + m], path, dtype, at)
            at += m
        out["A"] = snapshot(ctx)
        ctx.act(x[:9].astype(np.float64), SEED, 2)                   # evaluation calls count nothing
        D.act_dev_call(ctx, x[:9], dtype, 0, 1)
        out["A_after_act"] = snapshot(ctx)
        ctx.obsnorm_fold()
        out["fold"] = snapshot(ctx)
        for m in SEQ_B:
            record_call(ctx, x[at:at + m], path, dtype, at)
            at += m
        out["B"] = snapshot(ctx)
    return out


def reference_sequence(dtype):
    x = sequence_rows(dtype)
    f, at, out = N.Filter(S70[0][0]), 0, {}
    for m in SEQ_A:
        f.record(x[at:at + m])
        at += m
    out["A"] = (f.pending, f.live)
    f.fold()
    out["fold"] = (f.pending, f.live)
    for m in SEQ_B:
        f.record(x[at:at + m])
        at += m
    out["B"] = (f.pending, f.live)
    return out


def held(got, want, what):
    """got = [count, mean, M2] of the device, want = (n, mean, M2) of the reference"""
    L0 = S70[0][0]
    assert got[0] == want[0], what
    if want[0] == 0:
        assert not got.any(), what
        return
    em, e2 = N.rel_err(got[1:1 + L0], want[1]), N.rel_err(got[1 + L0:], want[2])
    print("%s: mean %.2e  M2 %.2e" % (what, em, e2))
    assert em <= TOL and e2 <= TOL, (what, em, e2)


@pytest.mark.parametrize("path", ("host", "dev", "dev32"))
@pytest.mark.parametrize("form", FORMS)
def test_statistics_against_the_long_double_reference(form, path):
    got, want = run_sequence(form, path), reference_sequence(np.float32 if path == "dev32" else np.float64)
    N.assert_one_pass_loses(sequence_rows(np.float64)[:sum(SEQ_A)])         # what the bound below is there to catch
    for point in ("A", "fold", "B"):
        held(got[point][0], want[point][0], "%s pending" % point)
        held(got[point][1], want[point][1], "%s live" % point)
    n, mean, m2 = want["B"][1]
    sh, sc = N.derived(n, mean.astype(np.float64), m2.astype(np.float64), EPS)
    assert N.rel_err(got["B"][2], sh) <= TOL and N.rel_err(got["B"][3], sc) <= TOL


def test_statistics_side_conditions():
    got = run_sequence("neuron", "host")
    assert got["discarded"][0][0] == 7 and got["discarded"][0][1:].any()
    assert not got["begun"][0].any(), "record_begin leaves pending"
    for a, b in zip(got["A"], got["A_after_act"]):
        R.same_bits(a, b, "act / act_dev touched the statistics")
    assert got["A"][0][0] == sum(SEQ_A) and got["A"][1][0] == 0
    assert got["fold"][0][0] == 0 and got["fold"][1][0] == sum(SEQ_A)
    R.same_bits(got["fold"][1], got["B"][1], "live changed without a fold")
    R.same_bits(got["fold"][2], got["B"][2], "shift changed without a fold")
    R.same_bits(got["fold"][3], got["B"][3], "scale changed without a fold")


@pytest.mark.parametrize("other", [("neuron", "host", 1), ("lane", "host", 0), ("neuron", "dev", 0), ("lane", "dev", 0)],
                         ids=("again", "lane", "dev-fp64", "lane-dev-fp64"))
def test_statistics_bits_do_not_depend_on_the_path(other):
    """the same sequence a second time, the other kernel form, device fp64 rows against host rows: the same bits"""
    a, b = run_sequence("neuron", "host"), run_sequence(*other)
    for point in a:
        for x, y in zip(a[point], b[point]):
            R.same_bits(x, y, point)


def test_fp32_rows_give_the_statistics_of_their_widened_values():
    """the fp32 device sequence against host calls on the same rows widened: the same bits at every point"""
    a, b = run_sequence("neuron", "dev32"), run_sequence("neuron", "host32")
    for point in a:
        for x, y in zip(a[point], b[point]):
            R.same_bits(x, y, point)


# ---- 5. chunk edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ("host", "dev"))
@pytest.mark.parametrize("m", (2 * trpo_amd.OBSNORM_CHUNK + 1, 17 * trpo_amd.OBSNORM_CHUNK + 3),
                         ids=("two-chunks-and-a-row", "more-chunks-than-waves"))
def test_one_call_across_chunk_edges(m, path):
    shape = ((5, 8, 2), "ltl")
    x = N.ill_conditioned(m, 5, seed=3)
    with R.context(shape, R.old_batch(shape)) as ctx:
        ctx.obsnorm_enable(CLIP, EPS)
        ctx.record_begin(m)
        record_call(ctx, x, path, np.float64, 0)
        p = ctx.obsnorm_state(pending=True)
    n, mean, m2 = N.direct(x)
    assert p["count"] == n == m
    em, e2 = N.rel_err(p["mean"], mean), N.rel_err(p["m2"], m2)
    print("m=%d %s: mean %.2e  M2 %.2e" % (m, path, em, e2))
    assert em <= TOL and e2 <= TOL, (em, e2)


# ---- 6. checkpoint and apply ---------------------------------------------------------------------------------
def test_checkpoint_restores_the_filter():
    x = N.ill_conditioned(SEQ_ROWS, S70[0][0])
    with R.context(S70, R.old_batch(S70)) as a, R.context(S70, R.old_batch(S70)) as b:
        a.obsnorm_enable(CLIP, EPS)
        a.record_begin(130)
        a.act_record(x[:130], SEED, 0)
        a.obsnorm_fold()
        st = a.obsnorm_state()
        b.obsnorm_enable(CLIP, EPS)
        b.obsnorm_set_state(st["count"], st["mean"], st["m2"])
        st_b = b.obsnorm_state()
        for key in ("mean", "m2", "shift", "scale"):
            R.same_bits(st[key], st_b[key], key)
        assert st["count"] == st_b["count"] == 130 and b.obsnorm_state(pending=True)["count"] == 0
        same3(a.act(x[130:160], SEED, 5), b.act(x[130:160], SEED, 5), "act after the restore")


def test_apply_is_the_formula():
    L0 = S70[0][0]
    obs = problem(L0)[3]
    with R.context(S70, R.old_batch(S70)) as ctx:
        shift, scale = restored(ctx, L0)
        want = N.normalise(obs, shift, scale, CLIP)
        R.same_bits(ctx.obsnorm_apply(obs), want, "apply")
        for dtype in (np.float64, np.float32):
            raw = obs.astype(dtype)
            w = N.normalise(raw, shift, scale, CLIP)
            d_in, d_out = D.dev(raw, dtype), devmem.DeviceArray(raw.shape, dtype, 0)
            ctx.obsnorm_apply_dev(d_in, d_out, dtype=dtype)
            ctx.synchronize()
            D.same_out(d_out.to_host(), w, dtype, "apply_dev")
            assert np.array_equal(d_in.to_host().view(np.uint8), raw.view(np.uint8)), "apply_dev wrote its input"
            st = devmem.Stream(0)
            ctx.obsnorm_apply_dev(d_in, dtype=dtype, stream=st)     # in place
            st.synchronize()
            D.same_out(d_in.to_host(), w, dtype, "apply_dev in place")


# ---- 7. refusals ---------------------------------------------------------------------------------------------
class HostArray:
    """host memory behind the device-array protocol"""

    def __init__(self, a):
        self.a = a
        self.__cuda_array_interface__ = dict(shape=a.shape, typestr="<f8", data=(a.ctypes.data, False), version=3,
                                             strides=None)


def test_refusals():
    L0 = S3[0][0]
    nan, inf = float("nan"), float("inf")
    ok = np.ones(L0)
    with R.context(S3, R.old_batch(S3)) as ctx:
        d = D.dev(np.zeros((2, L0)))
        for fn in (ctx.obsnorm_disable, ctx.obsnorm_fold, ctx.obsnorm_state, lambda: ctx.obsnorm_state(pending=True),
                   lambda: ctx.obsnorm_set_state(2, ok, ok), lambda: ctx.obsnorm_apply(np.zeros((2, L0))),
                   lambda: ctx.obsnorm_apply_dev(d)):
            R.expect_invalid(fn, "trpo_ctx_obsnorm_", "not enabled")
        for clip, eps in ((0.0, 0.0), (-1.0, 0.0), (nan, 0.0), (1.0, -1e-9), (1.0, nan)):
            R.expect_invalid(lambda: ctx.obsnorm_enable(clip, eps), "trpo_ctx_obsnorm_enable")
        R.expect_invalid(ctx.obsnorm_fold, "not enabled")           # a refused enable has enabled nothing
        ctx.obsnorm_enable(inf, 0.0)
        bad = lambda v: np.array([1.0, v, 1.0])
        for count, mean, m2 in ((-1, ok, ok), (2.5, ok, ok), (nan, ok, ok), (2, bad(inf), ok), (2, bad(nan), ok),
                                (2, ok, bad(-1.0)), (2, ok, bad(inf)), (2, ok, bad(nan))):
            R.expect_invalid(lambda: ctx.obsnorm_set_state(count, mean, m2), "trpo_ctx_obsnorm_set")
        assert ctx.obsnorm_state()["count"] == 0
        R.expect_invalid(lambda: ctx.obsnorm_apply_dev(HostArray(np.zeros((2, L0)))), "trpo_ctx_obsnorm_apply_dev",
                         "in_dev", "not device memory")
        R.expect_invalid(lambda: ctx.obsnorm_apply_dev(d, HostArray(np.zeros((2, L0)))), "trpo_ctx_obsnorm_apply_dev",
                         "out_dev")
        short = D.dev(np.zeros((1, L0)))
        R.expect_invalid(lambda: apply_dev_two_rows(ctx, d, short), "trpo_ctx_obsnorm_apply_dev", "out_dev",
                         "allocation")
        ctx.obsnorm_disable()
        R.expect_invalid(ctx.obsnorm_fold, "not enabled")


def apply_dev_two_rows(ctx, d_in, d_short):
    """apply_dev on two rows with an output array that holds one: the C call, past the Python shape check"""
    rc = trpo_amd.lib().trpo_ctx_obsnorm_apply_dev(ctx._h, d_in.ptr, 2, trpo_amd.DT_F64, d_short.ptr, None)
    if rc < 0:
        raise ctx._refused("obsnorm_apply_dev", rc)
