"""MI355X tests of the device-resident advantage stage (trpo_baseline_advantage, trpo_ctx_set_rollout_adv).

The reference is written here with numpy from the definitions, as direct sums sum_k c^k x[t+k] (np.power),
not as the recurrence, with a two-pass mean and variance; V comes from the CPU oracle's baseline forward.
Bounds: the project's fp64 bound 1e-12 (returns relative to max|ret|, standardised advantages absolute,
the four statistics relative).  Every case is checked to be well conditioned on the reference:
std(A) / max|A| >= 0.05.
"""
import functools

import numpy as np
import pytest

import oracle
import trpo_amd
from trpo_amd import synth

pytestmark = pytest.mark.gpu

BASE = [16, 16, 16, 1]
AC = "lttl"
SHAPES = [(20, 150), (1, 150), (5, 64), (7, 63), (3, 65), (2, 129), (257, 2), (4, 200)]
COEFFS = [(0.995, 0.98), (1.0, 1.0), (0.0, 0.5), (0.9, 0.0)]
TOL = 1e-12
TRPO_E_INVALID = -1


@functools.lru_cache(maxsize=None)
def inputs(num_ep, ep_len, layers=tuple(BASE), seed=7):
    rng = np.random.default_rng(seed)
    n = num_ep * ep_len
    npar = synth.num_params(list(layers)) - layers[-1]
    reward = -np.abs(rng.normal(1.0, 0.7, n))
    observ = rng.normal(0.0, 1.0, (n, layers[0] - 1))
    x = 0.3 * rng.normal(0.0, 1.0, npar)
    for a in (reward, observ, x):
        a.setflags(write=False)
    return x, observ, reward


def discounted(x, c):
    """y[e, t] = sum_k c^k x[e, t + k], as direct sums."""
    T = x.shape[1]
    k = np.arange(T)[None, :] - np.arange(T)[:, None]            # [t, j] -> j - t
    M = np.where(k >= 0, np.power(float(c), np.maximum(k, 0)), 0.0)
    return (x[:, None, :] * M[None, :, :]).sum(axis=2)


@functools.lru_cache(maxsize=None)
def reference(num_ep, ep_len, gamma, lam, layers=tuple(BASE), ac=AC):
    x, observ, reward = inputs(num_ep, ep_len, layers)
    V = oracle.baseline_evaluate(list(layers), ac, x, observ, np.zeros(num_ep * ep_len), num_ep, ep_len)[2]
    r, V = reward.reshape(num_ep, ep_len), V.reshape(num_ep, ep_len)
    Vn = np.concatenate([V[:, 1:], np.zeros((num_ep, 1))], axis=1)
    delta = r + gamma * Vn - V
    ret = discounted(r, gamma).ravel()
    A = discounted(delta, gamma * lam).ravel()
    am = A.sum() / A.size
    asd = np.sqrt(((A - am) ** 2).sum() / A.size)
    R = r.sum(axis=1)
    rm = R.sum() / R.size
    rsd = np.sqrt(((R - rm) ** 2).sum() / R.size)
    assert asd / np.abs(A).max() >= 0.05, "ill-conditioned case: change its seed"
    out = dict(ret=ret, adv=(A - am) / asd, A=A, ep_rew_mean=rm, ep_rew_std=rsd, adv_mean=am, adv_std=asd)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def check_against_reference(adv, ret, info, ref):
    e_ret = np.abs(ret - ref["ret"]).max() / np.abs(ref["ret"]).max()
    e_adv = np.abs(adv - ref["adv"]).max()
    e_st = {k: abs(info[k] - ref[k]) / abs(ref[k]) for k in ("ep_rew_mean", "ep_rew_std", "adv_mean", "adv_std")
            if ref[k] != 0.0}
    print("ret %.3e adv %.3e stats %s" % (e_ret, e_adv, {k: "%.2e" % v for k, v in e_st.items()}))
    assert e_ret <= TOL
    assert e_adv <= TOL
    for k in ("ep_rew_mean", "ep_rew_std", "adv_mean", "adv_std"):
        assert abs(info[k] - ref[k]) <= TOL * abs(ref[k]), k


@pytest.mark.parametrize("gamma,lam", COEFFS)
@pytest.mark.parametrize("num_ep,ep_len", SHAPES)
def test_parity(num_ep, ep_len, gamma, lam):
    x, observ, reward = inputs(num_ep, ep_len)
    ref = reference(num_ep, ep_len, gamma, lam)
    with trpo_amd.Baseline(BASE, AC) as bl:
        adv, ret, info = bl.advantage(x, observ, reward, num_ep, ep_len, gamma, lam)
    check_against_reference(adv, ret, info, ref)


@pytest.mark.parametrize("num_ep,ep_len", [(20, 150), (3, 65)])
def test_prediction_bits(num_ep, ep_len):
    """gamma = 0 makes ret = reward (exactly) and A = reward - V: the raw advantage recovered from the
    outputs is reward minus the predictions trpo_baseline_evaluate returns for the same x."""
    x, observ, reward = inputs(num_ep, ep_len)
    reference(num_ep, ep_len, 0.0, 0.0)                          # conditioning
    with trpo_amd.Baseline(BASE, AC) as bl:
        adv, ret, info = bl.advantage(x, observ, reward, num_ep, ep_len, 0.0, 0.0)
        V = bl.evaluate(x, want_predict=True)[2]
    np.testing.assert_array_equal(ret, reward)
    raw = adv * info["adv_std"] + info["adv_mean"]
    want = reward - V
    err = np.abs(raw - want).max() / np.abs(want).max()
    print("raw advantage vs reward - evaluate's predictions: %.3e" % err)
    assert err <= 1e-13


@pytest.mark.parametrize("gamma,lam", COEFFS)
def test_second_baseline_shape(gamma, lam):
    """[8, 24, 1] does not take the lane kernel: the prediction kernel serves every shape."""
    layers, ac, num_ep, ep_len = (8, 24, 1), "ltl", 3, 65
    x, observ, reward = inputs(num_ep, ep_len, layers)
    ref = reference(num_ep, ep_len, gamma, lam, layers, ac)
    with trpo_amd.Baseline(list(layers), ac) as bl:
        adv, ret, info = bl.advantage(x, observ, reward, num_ep, ep_len, gamma, lam)
    check_against_reference(adv, ret, info, ref)


def test_fit_target():
    """After advantage() the object holds (observ, target = ret): the fit's evaluate needs no upload."""
    num_ep, ep_len = 20, 150
    x, observ, reward = inputs(num_ep, ep_len)
    reference(num_ep, ep_len, 0.995, 0.98)
    x2 = 0.3 * np.random.default_rng(11).normal(0.0, 1.0, x.size)
    with trpo_amd.Baseline(BASE, AC) as bl, trpo_amd.Baseline(BASE, AC) as other:
        _, ret, _ = bl.advantage(x, observ, reward, num_ep, ep_len)
        f, g = bl.evaluate(x2)
        other.set_data(observ, ret, num_ep, ep_len)
        f2, g2 = other.evaluate(x2)
    assert f == f2
    np.testing.assert_array_equal(g, g2)


def test_repeatable():
    num_ep, ep_len = 20, 150
    x, observ, reward = inputs(num_ep, ep_len)
    reference(num_ep, ep_len, 0.995, 0.98)
    with trpo_amd.Baseline(BASE, AC) as bl:
        a = bl.advantage(x, observ, reward, num_ep, ep_len)
        b = bl.advantage(x, observ, reward, num_ep, ep_len)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2]


def policy_problem(layers, n, start=0):
    th, obs = synth.make_theta(layers), synth.make_obs(n, layers[0], start=start)
    std = np.ones(layers[-1])
    mean, action, _ = synth.make_rollout(layers, "lttl", th, obs, std)
    return th, obs, std, mean, action


def assert_same_update(r, s):
    for k in ("theta", "b", "x"):
        np.testing.assert_array_equal(r[k], s[k])


@pytest.mark.parametrize("layers,num_ep,ep_len", [([15, 16, 16, 3], 334, 150), ([15, 64, 64, 3], 20, 150)])
def test_hand_off_to_update(layers, num_ep, ep_len):
    x, observ, reward = inputs(num_ep, ep_len)
    reference(num_ep, ep_len, 0.995, 0.98)
    th, obs, std, mean, action = policy_problem(layers, num_ep * ep_len)
    with trpo_amd.Baseline(BASE, AC) as bl:
        adv, _, _ = bl.advantage(x, observ, reward, num_ep, ep_len)
        with trpo_amd.Context(layers, "lttl", th, obs, std, 0.1) as ctx:
            ctx.set_rollout_from(bl, mean, action)
            r = ctx.update()
    with trpo_amd.Context(layers, "lttl", th, obs, std, 0.1) as host:
        host.set_rollout(mean, action, adv)
        s = host.update()
    assert_same_update(r, s)


def test_slice():
    """A sharded caller's rank: the global batch's advantages, its own contiguous slice of them."""
    layers, num_ep, ep_len, first = [15, 16, 16, 3], 20, 150, 1350
    x, observ, reward = inputs(num_ep, ep_len)
    reference(num_ep, ep_len, 0.995, 0.98)
    th, obs, std, mean, action = policy_problem(layers, num_ep * ep_len - first, start=first)
    with trpo_amd.Baseline(BASE, AC) as bl:
        adv, _, _ = bl.advantage(x, observ, reward, num_ep, ep_len)
        with trpo_amd.Context(layers, "lttl", th, obs, std, 0.1) as ctx:
            ctx.set_rollout_from(bl, mean, action, first=first)
            r = ctx.update()
    with trpo_amd.Context(layers, "lttl", th, obs, std, 0.1) as host:
        host.set_rollout(mean, action, adv[first:])
        s = host.update()
    assert_same_update(r, s)


def test_hand_off_invalidates_cached_rollout_rows():
    """The policy gradient's cached fp32 rows follow the rollout's generation: a device hand-off after a
    host upload must rebuild them."""
    layers, num_ep, ep_len = [15, 16, 16, 3], 20, 150
    x, observ, reward = inputs(num_ep, ep_len)
    reference(num_ep, ep_len, 0.995, 0.98)
    th, obs, std, mean, action = policy_problem(layers, num_ep * ep_len)
    a1 = synth.normal(synth.SEED, synth.STREAM_ADV, num_ep * ep_len)
    with trpo_amd.Baseline(BASE, AC) as bl, trpo_amd.Context(layers, "lttl", th, obs, std, 0.1) as ctx:
        ctx.set_rollout(mean, action, a1)
        r1 = ctx.update()
        adv, _, _ = bl.advantage(x, observ, reward, num_ep, ep_len)
        ctx.set_rollout_from(bl, mean, action)
        r2 = ctx.update()
    with trpo_amd.Context(layers, "lttl", th, obs, std, 0.1) as fresh:
        fresh.set_rollout(mean, action, adv)
        s = fresh.update()
    assert not np.array_equal(r1["b"], r2["b"])
    assert_same_update(r2, s)


def expect_invalid(fn):
    with pytest.raises(trpo_amd.TRPOError) as e:
        fn()
    assert e.value.code == TRPO_E_INVALID
    assert trpo_amd.last_error()


def test_errors():
    layers, num_ep, ep_len = [15, 16, 16, 3], 20, 150
    n = num_ep * ep_len
    x, observ, reward = inputs(num_ep, ep_len)
    th, obs, std, mean, action = policy_problem(layers, n)
    a1 = synth.normal(synth.SEED, synth.STREAM_ADV, n)
    with trpo_amd.Baseline(BASE, AC) as bl, trpo_amd.Context(layers, "lttl", th, obs, std, 0.1) as ctx:
        ctx.set_rollout(mean, action, a1)
        r1 = ctx.update()
        # no advantage computed: a fresh baseline, and one whose batch was replaced by set_data
        expect_invalid(lambda: ctx.set_rollout_from(bl, mean, action))
        bl.advantage(x, observ, reward, num_ep, ep_len)
        bl.set_data(observ, reward, num_ep, ep_len)
        expect_invalid(lambda: ctx.set_rollout_from(bl, mean, action))
        # the slice does not fit
        bl.advantage(x, observ, reward, num_ep, ep_len)
        expect_invalid(lambda: ctx.set_rollout_from(bl, mean, action, first=1))
        # zero standard deviation: one sample; constant advantages (x = 0 makes V = 0, one-step episodes
        # make A = reward, and sums of -1.0 are exact); each leaves no advantage behind
        x1, o1, w1 = inputs(1, 1)
        expect_invalid(lambda: bl.advantage(x1, o1, w1, 1, 1))
        expect_invalid(lambda: ctx.set_rollout_from(bl, mean, action))
        bl.advantage(x, observ, reward, num_ep, ep_len)
        expect_invalid(lambda: bl.advantage(np.zeros(x.size), observ, -np.ones(n), n, 1))
        expect_invalid(lambda: ctx.set_rollout_from(bl, mean, action))
        # ... as do constant rewards over whole episodes once lambda = 0 (A = delta = reward)
        expect_invalid(lambda: bl.advantage(np.zeros(x.size), observ, -np.ones(n), num_ep, ep_len, 0.995, 0.0))
        # the context's earlier rollout is as it was
        assert_same_update(ctx.update(), r1)
