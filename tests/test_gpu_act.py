"""MI355X tests of device policy inference (trpo_ctx_act, trpo_ctx_act_clear, trpo_ctx_set_rollout_acted).

The reference is tests/act_ref.py: synth.policy_mean for the mean, Philox4x32-10 in integer arithmetic and
numpy's sqrt / log / cos / sin for the normals.  Bounds: mean 1e-12 (1 + |mean|), the project's fp64 bound
(device tanh64 and the continued-fraction tanh differ in the last places); action against
mean_dev + exp(LogStd) z_ref 1e-13 (1 + |action|) (the uniforms are exact, the four functions a few ulp on a
value of magnitude <= 8.6); logp 1e-12 (1 + |logp|).  Everything else is bit for bit.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import act_ref as R
import trpo_amd
from trpo_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [([15, 16, 16, 3], "lttl"), ([11, 64, 64, 3], "lttl"), ([4, 8, 8, 8, 2], "ltsot"), ([12, 32, 1], "ltl"),
          ([376, 64, 64, 17], "lttl")]
IDS = ["arm", "2x64", "deep-s-o", "one-action", "wide-in"]
MS = [1, 63, 64, 65, 130]
NROWS = 130
SEED, STEP = 0x5EED0123456789AB, 41
TRPO_E_INVALID = -1


@functools.lru_cache(maxsize=None)
def problem(k, n=NROWS):
    """theta with non-zero biases and LogStd, obs [n][L0], and the reference's rows 0..n-1 at (SEED, STEP)."""
    layers, ac = SHAPES[k]
    rng = np.random.default_rng(100 + k)
    th = synth.make_theta(layers) + 0.05 * rng.normal(size=synth.num_params(layers))
    th[-layers[-1]:] = rng.uniform(-1.0, 0.5, layers[-1])
    obs = 0.5 * rng.normal(size=(n, layers[0]))
    mean, _, logp, z = R.act(layers, ac, th, obs, SEED, STEP)
    for a in (th, obs, mean, logp, z):
        a.setflags(write=False)
    return th, obs, mean, logp, z


@contextlib.contextmanager
def context(k, obs, form=None, precision=None, theta=None):
    """A context of shape k (an index into SHAPES, or (layers, activations) with a theta) whose std is the
    policy's own exp(LogStd); form: TRPO_ACT_FORM at its creation."""
    layers, ac = SHAPES[k] if isinstance(k, int) else k
    th = problem(k)[0] if theta is None else theta
    saved = os.environ.pop("TRPO_ACT_FORM", None)
    if form:
        os.environ["TRPO_ACT_FORM"] = form
    try:
        ctx = trpo_amd.Context(layers, ac, th, obs, np.exp(th[-layers[-1]:]), 0.1, precision=precision)
    finally:
        os.environ.pop("TRPO_ACT_FORM", None)
        if saved is not None:
            os.environ["TRPO_ACT_FORM"] = saved
    with ctx:
        yield ctx


def check_against_reference(k, out, rows, ref=None):
    mean, action, logp = out
    th, _, rmean, rlogp, rz = ref or problem(k)
    A = SHAPES[k][0][-1]
    want = mean + np.exp(th[-A:]) * rz[rows]
    e_mean = (np.abs(mean - rmean[rows]) / (1.0 + np.abs(rmean[rows]))).max()
    e_act = (np.abs(action - want) / (1.0 + np.abs(want))).max()
    e_lp = (np.abs(logp - rlogp[rows]) / (1.0 + np.abs(rlogp[rows]))).max()
    print("%s m=%d: mean %.2e action %.2e logp %.2e" % (IDS[k], mean.shape[0], e_mean, e_act, e_lp))
    assert e_mean <= 1e-12
    assert e_act <= 1e-13
    assert e_lp <= 1e-12


def same_bits(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_parity_and_form_bits(k):
    """Mean, action and logp against the reference at every m, in both forced forms and under the default
    rule; the same call twice, the two forms, the default rule and any batch size give a row the same bits."""
    _, obs, _, _, _ = problem(k)
    got = {}
    for form in ("lane", "neuron", None):
        with context(k, obs, form) as ctx:
            for m in MS:
                out = ctx.act(obs[:m], SEED, STEP)
                check_against_reference(k, out, slice(0, m))
                same_bits(out, ctx.act(obs[:m], SEED, STEP))
                got[form, m] = out
    for m in MS:
        same_bits(got["lane", m], got["neuron", m])
        same_bits(got["lane", m], got[None, m])
        same_bits(got["lane", m], [a[:m] for a in got["neuron", NROWS]])


@pytest.mark.parametrize("form", ["lane", "neuron", None])
@pytest.mark.parametrize("k", [0, 3, 4], ids=[IDS[0], IDS[3], IDS[4]])
def test_call_geometry_does_not_show(k, form):
    """Rows 0..129 in one call equal two calls (0..64, 65..129); a strided call equals per-row m = 1 calls."""
    _, obs, _, _, _ = problem(k)
    with context(k, obs, form) as ctx:
        whole = ctx.act(obs, SEED, STEP)
        lo, hi = ctx.act(obs[:65], SEED, STEP), ctx.act(obs[65:], SEED, STEP, row0=65)
        same_bits(whole, [np.concatenate([a, b]) for a, b in zip(lo, hi)])
        rows = 3 + 7 * np.arange(10)
        strided = ctx.act(obs[rows], SEED, STEP, row0=3, row_stride=7)
        check_against_reference(k, strided, rows)
        same_bits(strided, [a[rows] for a in whole])
        for i, r in enumerate(rows):
            one = ctx.act(obs[r], SEED, STEP, row0=int(r))
            same_bits(one, [a[i:i + 1] for a in strided])


@pytest.mark.parametrize("form", ["lane", "neuron"])
def test_counter_words(form):
    """The high halves of seed, step and row reach the generator: rows beyond 2^32, a step beyond 2^32."""
    k = 1
    layers, ac = SHAPES[k]
    th, obs, _, _, _ = problem(k)
    seed, step, row0, stride = 0xDEADBEEF12345678, (0x1234 << 32) | 77, (1 << 40) + 3, (1 << 33) + 1
    mean, _, logp, z = R.act(layers, ac, th, obs[:70], seed, step, row0, stride)
    with context(k, obs, form) as ctx:
        out = ctx.act(obs[:70], seed, step, row0=row0, row_stride=stride)
        check_against_reference(k, out, slice(0, 70), ref=(th, None, mean, logp, z))
        top = ctx.act(obs[:2], seed, (1 << 48) - 1, row0=(1 << 48) - 2)
        _, _, lp, zt = R.act(layers, ac, th, obs[:2], seed, (1 << 48) - 1, (1 << 48) - 2)
        check_against_reference(k, top, slice(0, 2), ref=(th, None, top[0], lp, zt))


def test_step_and_seed():
    """Another step or seed changes every action; sample=False returns the same means and no samples."""
    k = 4
    _, obs, _, _, _ = problem(k)
    with context(k, obs) as ctx:
        base = ctx.act(obs, SEED, STEP)
        for seed, step in ((SEED, STEP + 1), (SEED, STEP + (1 << 32)), (SEED + 1, STEP), (SEED ^ (1 << 63), STEP)):
            other = ctx.act(obs, seed, step)
            np.testing.assert_array_equal(other[0], base[0])
            assert np.all(other[1] != base[1])
            assert np.all(other[2] != base[2])
        for m in (1, 16, NROWS):
            mean, action, logp = ctx.act(obs[:m], SEED, STEP, sample=False)
            assert action is None and logp is None
            np.testing.assert_array_equal(mean, base[0][:m])
        same_bits(ctx.act(obs, SEED, STEP), base)


def test_sample_statistics():
    """Seed 20261020, step 0, rows 0..65535, A = 3 (a batch beyond the pinned buffer: the staged path):
    z = (action - mean) / sigma has |mean| sqrt(n) <= 4 and |var - 1| sqrt(n / 2) <= 4; the reference gives
    0.71 and 0.24 for exactly these inputs (tests/test_act_abi.py asserts the conditions on it)."""
    k, n = 0, 65536
    th = problem(k)[0]
    obs = np.random.default_rng(5).uniform(-0.2, 0.2, (n, 15))
    with context(k, obs[:1]) as ctx:
        mean, action, logp = ctx.act(obs, 20261020, 0)
        head = ctx.act(obs[:100], 20261020, 0)
    same_bits(head, [mean[:100], action[:100], logp[:100]])
    z = ((action - mean) / np.exp(th[-3:])).reshape(-1)
    zr = R.normals(20261020, 0, np.arange(n), 3).reshape(-1)
    s_mean, s_var = abs(z.mean()) * np.sqrt(z.size), abs(z.var() - 1.0) * np.sqrt(z.size / 2.0)
    print("mean %.3f var %.3f max|z - z_ref| %.2e" % (s_mean, s_var, np.abs(z - zr).max()))
    assert s_mean <= 4.0
    assert s_var <= 4.0
    assert np.abs(z - zr).max() <= 1e-12           # the recovered z carries the rounding of (action - mean) / sigma


UPDATE_KEYS = ("theta", "b", "x", "shs", "lagrange", "gnorm", "fval", "rate", "accepted", "evaluated", "actual",
               "expected", "ratio", "cg_iters")


def assert_same_update(r, s):
    for key in UPDATE_KEYS:
        np.testing.assert_array_equal(r[key], s[key], err_msg=key)


def keep_all(ctx, obs, seed=SEED, step=STEP):
    """The context's own rows in two strided calls; (mean, action) [n][A] as the host received them."""
    n, A = obs.shape[0], ctx.layers[-1]
    mean, action = np.zeros((n, A)), np.zeros((n, A))
    for r0 in (1, 0):
        m, a, _ = ctx.act(obs[r0::2], seed, step, row0=r0, row_stride=2, keep=True)
        mean[r0::2], action[r0::2] = m, a
    return mean, action


@pytest.mark.parametrize("precision", [None, "fp64"])
@pytest.mark.parametrize("k", [0, 4], ids=[IDS[0], IDS[4]])
def test_hand_off_to_update(k, precision):
    """act(keep) over the context's rows, set_rollout_acted(adv), update == set_rollout(mean_out, action_out,
    adv), update on a fresh context, bit for bit."""
    n = 301
    obs = problem(k, 320)[1][:n]
    adv = synth.normal(synth.SEED, synth.STREAM_ADV, n)
    with context(k, obs, precision=precision) as ctx:
        mean, action = keep_all(ctx, obs)
        ctx.set_rollout_acted(adv)
        r = ctx.update()
    with context(k, obs, precision=precision) as fresh:
        fresh.set_rollout(mean, action, adv)
        s = fresh.update()
    assert_same_update(r, s)


@pytest.mark.parametrize("precision", [None, "fp64"])
def test_hand_off_with_baseline_advantages(precision):
    """The same with the advantages taken on the device from a Baseline, against set_rollout_from."""
    k, num_ep, ep_len, first = 0, 4, 80, 19
    n = num_ep * ep_len - first
    obs = problem(k, 320)[1][:n]
    rng = np.random.default_rng(9)
    base = [16, 16, 16, 1]
    x = 0.3 * rng.normal(size=synth.num_params(base) - 1)
    observ, reward = rng.normal(size=(num_ep * ep_len, 15)), -np.abs(rng.normal(1.0, 0.7, num_ep * ep_len))
    with trpo_amd.Baseline(base, "lttl") as bl:
        bl.advantage(x, observ, reward, num_ep, ep_len)
        with context(k, obs, precision=precision) as ctx:
            mean, action = keep_all(ctx, obs)
            ctx.set_rollout_acted(baseline=bl, first=first)
            r = ctx.update()
        with context(k, obs, precision=precision) as fresh:
            fresh.set_rollout_from(bl, mean, action, first=first)
            s = fresh.update()
    assert_same_update(r, s)


def expect_invalid(fn):
    with pytest.raises(trpo_amd.TRPOError) as e:
        fn()
    assert e.value.code == TRPO_E_INVALID
    assert trpo_amd.last_error()


def test_refusals():
    k, n = 0, 90
    layers = SHAPES[k][0]
    obs = problem(k)[1][:n]
    adv = synth.normal(synth.SEED, synth.STREAM_ADV, n)
    with context(k, obs) as ctx, trpo_amd.Baseline([16, 16, 16, 1], "lttl") as bl:
        keep_all(ctx, obs)
        ctx.set_rollout_acted(adv)
        r1 = ctx.update()
        # exactly one of adv and the baseline
        expect_invalid(lambda: ctx.set_rollout_acted())
        expect_invalid(lambda: ctx.set_rollout_acted(adv, baseline=bl))
        # a baseline without advantages
        expect_invalid(lambda: ctx.set_rollout_acted(baseline=bl))
        # after act_clear; then with one row missing
        ctx.act_clear()
        expect_invalid(lambda: ctx.set_rollout_acted(adv))
        ctx.act(obs[:n - 1], SEED, STEP + 1, keep=True)
        expect_invalid(lambda: ctx.set_rollout_acted(adv))
        # the rollout is as it was
        assert_same_update(ctx.update(), r1)
        # the missing row arrives (twice: a row counts once)
        ctx.act(obs[n - 2:], SEED, STEP + 1, row0=n - 2, keep=True)
        ctx.set_rollout_acted(adv)
        assert not np.array_equal(ctx.update()["b"], r1["b"])
        # set_obs forgets the kept rows
        ctx.set_obs(obs)
        expect_invalid(lambda: ctx.set_rollout_acted(adv))
        # every argument error of the header
        expect_invalid(lambda: ctx.act(np.zeros((0, layers[0])), SEED))
        expect_invalid(lambda: ctx.act(obs, SEED, row_stride=0))
        expect_invalid(lambda: ctx.act(obs, SEED, step=1 << 48))
        expect_invalid(lambda: ctx.act(obs[:2], SEED, row0=(1 << 48) - 1))
        expect_invalid(lambda: ctx.act(obs[:2], SEED, row0=0, row_stride=1 << 48))
        expect_invalid(lambda: ctx.act(obs, SEED, keep=True, sample=False))
        expect_invalid(lambda: ctx.act(obs, SEED, row0=1, keep=True))
        expect_invalid(lambda: ctx.act(obs[:1], SEED, row0=n, keep=True))
        L, mean = trpo_amd.lib(), np.zeros((n, 3))
        assert L.trpo_ctx_act(ctx._h, None, n, 1, 0, 0, 1, 0, mean.ctypes.data, None, None) == TRPO_E_INVALID
        assert L.trpo_ctx_act(ctx._h, obs.ctypes.data, n, 1, 0, 0, 1, 0, None, None, None) == TRPO_E_INVALID
        assert L.trpo_ctx_act(ctx._h, obs.ctypes.data, n, 1, 0, 0, 1, 0, mean.ctypes.data, None,
                              mean.ctypes.data) == TRPO_E_INVALID
        # none of them kept anything
        expect_invalid(lambda: ctx.set_rollout_acted(adv))
        ctx.act(obs, SEED, STEP)                       # and the context still serves


def test_theta_change():
    """After set_theta, act runs the new weights."""
    k = 1
    layers, ac = SHAPES[k]
    th, obs, mean0, _, _ = problem(k)
    th2 = th + 0.1 * np.random.default_rng(3).normal(size=th.size)
    mean2, _, logp2, z2 = R.act(layers, ac, th2, obs, SEED, STEP)
    with context(k, obs) as ctx:
        before = ctx.act(obs, SEED, STEP)
        ctx.set_theta(th2)
        for m in (16, NROWS):
            after = ctx.act(obs[:m], SEED, STEP)
            check_against_reference(k, after, slice(0, m), ref=(th2, None, mean2, logp2, z2))
    assert np.abs(before[0] - mean0).max() <= 1e-12 * (1.0 + np.abs(mean0).max())
    assert np.all(after[0] != before[0])
