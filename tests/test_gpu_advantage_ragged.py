"""MI355X tests of the advantage stage for variable-length episodes with truncation bootstrap
(trpo_baseline_advantage_ragged, trpo_baseline_set_data_ragged).

The yardstick is tests/ragged_ref.py: numpy, direct sums per episode, two-pass mean and variance, its
baseline forward pinned to the CPU oracle by tests/test_advantage_ragged_abi.py.  Bounds: the project's fp64
bound 1e-12 (returns relative to max|ret|, standardised advantages absolute, the four statistics relative).
Every parity case asserts on the reference alone that std(A) / max|A| >= 0.05.
"""
import numpy as np
import pytest

import oracle
import ragged_ref as R
import trpo_amd
from trpo_amd import synth

pytestmark = pytest.mark.gpu

BASE, AC = list(R.BASE), R.AC
TOL = 1e-12
TRPO_E_INVALID = -1
STATS = ("ep_rew_mean", "ep_rew_std", "adv_mean", "adv_std")


@pytest.fixture(scope="module")
def bl():
    """One object for the parity cases: its batch changes size and shape from case to case."""
    with trpo_amd.Baseline(BASE, AC) as b:
        yield b


def run(b, lens, horizon, mode, gamma, lam, seed=7):
    x, observ, reward, boot_observ = R.inputs(lens, seed=seed)
    flags = R.boot_flags(mode, len(lens))
    return b.advantage_ragged(x, observ, reward, lens, horizon, gamma, lam,
                              boot_observ=None if flags is None else boot_observ, boot=flags)


def check_against_reference(adv, ret, info, ref):
    e_ret = np.abs(ret - ref["ret"]).max() / np.abs(ref["ret"]).max()
    e_adv = np.abs(adv - ref["adv"]).max()
    e_st = {k: abs(info[k] - ref[k]) / abs(ref[k]) for k in STATS if ref[k] != 0.0}
    print("ret %.3e adv %.3e stats %s" % (e_ret, e_adv, {k: "%.2e" % v for k, v in e_st.items()}))
    assert e_ret <= TOL
    assert e_adv <= TOL
    for k in STATS:
        assert abs(info[k] - ref[k]) <= TOL * abs(ref[k]), k


# 1. parity
@pytest.mark.parametrize("gamma,lam", R.COEFFS)
@pytest.mark.parametrize("name,horizon,mode", R.PARITY_CASES)
def test_parity(bl, name, horizon, mode, gamma, lam):
    lens, horizon = R.LENGTHS[name], R.horizon_of(name, horizon)
    ref = R.reference(lens, horizon, mode, gamma, lam)
    assert ref["conditioning"] >= 0.05, "ill-conditioned case: change its seed"
    adv, ret, info = run(bl, lens, horizon, mode, gamma, lam)
    check_against_reference(adv, ret, info, ref)


# 2. equal lengths, horizon = ep_len, no truncation: the fixed-length stage's bits
@pytest.mark.parametrize("gamma,lam", [(0.995, 0.98), (0.9, 0.0)])
@pytest.mark.parametrize("num_ep,ep_len", [(20, 150), (3, 65), (257, 2), (7, 63)])
def test_equal_lengths_reproduce_the_fixed_stage(num_ep, ep_len, gamma, lam):
    lens = (ep_len,) * num_ep
    x, observ, reward, _ = R.inputs(lens)
    with trpo_amd.Baseline(BASE, AC) as a, trpo_amd.Baseline(BASE, AC) as b:
        adv_r, ret_r, info_r = a.advantage_ragged(x, observ, reward, lens, ep_len, gamma, lam)
        eval_r = a.evaluate(x, want_predict=True)
        adv_f, ret_f, info_f = b.advantage(x, observ, reward, num_ep, ep_len, gamma, lam)
        eval_f = b.evaluate(x, want_predict=True)
    np.testing.assert_array_equal(adv_r, adv_f)
    np.testing.assert_array_equal(ret_r, ret_f)
    for k in STATS:
        np.testing.assert_array_equal(info_r[k], info_f[k])
    assert eval_r[0] == eval_f[0]
    np.testing.assert_array_equal(eval_r[1], eval_f[1])
    np.testing.assert_array_equal(eval_r[2], eval_f[2])


# 3. properties
PROP_LENS = R.LENGTHS["1-128-129-200-7"]


@pytest.mark.parametrize("mode", R.BOOTS)
def test_gamma_zero_returns_are_the_rewards(mode):
    _, _, reward, _ = R.inputs(PROP_LENS)
    with trpo_amd.Baseline(BASE, AC) as b:
        _, ret, _ = run(b, PROP_LENS, 200, mode, 0.0, 0.5)
    np.testing.assert_array_equal(ret, reward)


@pytest.mark.parametrize("mode", ("all", "alternate"))
def test_lambda_one_advantage_is_return_minus_value(mode):
    """lam = 1 telescopes: A[t] = ret[t] - V[t], the bootstrap inside ret."""
    x = R.inputs(PROP_LENS)[0]
    with trpo_amd.Baseline(BASE, AC) as b:
        adv, ret, info = run(b, PROP_LENS, 200, mode, 0.995, 1.0)
        V = b.evaluate(x, want_predict=True)[2]
    raw = adv * info["adv_std"] + info["adv_mean"]
    want = ret - V
    err = np.abs(raw - want).max() / np.abs(want).max()
    print("raw advantage vs ret - V: %.3e" % err)
    assert err <= TOL


def test_a_boot_flag_reaches_no_other_episode():
    """The stage returns the standardised advantages, whose mean and std every episode enters.  So the
    flag moves between two identical episodes put first in the batch (same observations, rewards and
    bootstrap observation): the multiset of raw A is the same in both runs, the per-episode partial sums
    swap places in a commutative first addition, mean A and std A come out with the same bits (asserted),
    and then equal standardised bits of the other episodes are equal raw A.  ret is returned raw: it is
    also compared across a plain flip of one episode's flag."""
    lens = (70, 70, 1, 128, 65, 7)
    x, observ, reward, boot_observ = (np.array(a) for a in R.inputs(lens))
    observ[70:140], reward[70:140], boot_observ[1] = observ[:70], reward[:70], boot_observ[0]
    rest = slice(140, None)
    with trpo_amd.Baseline(BASE, AC) as b:
        def stage(flags):
            return b.advantage_ragged(x, observ, reward, lens, 128, 0.995, 0.98, boot_observ=boot_observ,
                                      boot=np.array(flags, np.uint8))
        adv1, ret1, info1 = stage([1, 0, 0, 1, 0, 0])
        adv2, ret2, info2 = stage([0, 1, 0, 1, 0, 0])
        _, ret3, _ = stage([0, 0, 0, 1, 0, 0])
    assert info1 == info2
    np.testing.assert_array_equal(adv1[rest], adv2[rest])
    np.testing.assert_array_equal(ret1[rest], ret2[rest])
    np.testing.assert_array_equal(ret1[rest], ret3[rest])
    # the flag does act on its own episode, and the twins trade places
    assert not np.array_equal(ret1[:70], ret3[:70])
    np.testing.assert_array_equal(ret1[:70], ret2[70:140])
    np.testing.assert_array_equal(adv1[:70], adv2[70:140])


# 4. repeatability
def test_repeatable():
    lens = R.LENGTHS["1-128-129-200-7"]
    with trpo_amd.Baseline(BASE, AC) as b:
        first = run(b, lens, 200, "alternate", 0.995, 0.98)
        again = run(b, lens, 200, "alternate", 0.995, 0.98)
    np.testing.assert_array_equal(first[0], again[0])
    np.testing.assert_array_equal(first[1], again[1])
    assert first[2] == again[2]


# 5. the fit's data
def test_fit_target_is_set_data_ragged():
    lens, horizon = R.LENGTHS["1-128-129-200-7"], 256
    x, observ, reward, boot_observ = R.inputs(lens)
    x2 = 0.3 * np.random.default_rng(11).normal(0.0, 1.0, x.size)
    with trpo_amd.Baseline(BASE, AC) as b, trpo_amd.Baseline(BASE, AC) as other:
        _, ret, _ = run(b, lens, horizon, "alternate", 0.995, 0.98)
        f, g = b.evaluate(x2)
        other.set_data_ragged(observ, ret, lens, horizon)
        f2, g2 = other.evaluate(x2)
    assert f == f2
    np.testing.assert_array_equal(g, g2)


def test_fit_objective_against_the_oracle():
    """The ragged batch inside a [num_ep][horizon] rectangle has the same t / horizon features; a padding
    sample whose target is the oracle's own prediction there adds exactly nothing to the sums."""
    lens, horizon = R.LENGTHS["1-128-129-200-7"], 200
    x, observ, reward, _ = R.inputs(lens)
    num_ep, n, O = len(lens), sum(lens), BASE[0] - 1
    x2 = 0.3 * np.random.default_rng(11).normal(0.0, 1.0, x.size)
    with trpo_amd.Baseline(BASE, AC) as b:
        _, ret, _ = run(b, lens, horizon, "alternate", 0.995, 0.98)
        f, g = b.evaluate(x2)
    real = np.zeros((num_ep, horizon), bool)
    for e, L in enumerate(lens):
        real[e, :L] = True
    obs_rect = np.random.default_rng(12).normal(0.0, 1.0, (num_ep, horizon, O))
    obs_rect[real] = observ
    tgt_rect = np.zeros((num_ep, horizon))
    tgt_rect[real] = ret
    pred = oracle.baseline_evaluate(BASE, AC, x2, obs_rect, tgt_rect, num_ep, horizon)[2].reshape(num_ep, horizon)
    tgt_rect[~real] = pred[~real]
    fo, go, _ = oracle.baseline_evaluate(BASE, AC, x2, obs_rect, tgt_rect, num_ep, horizon)
    N = num_ep * horizon
    gs, gos = (g - 0.002 * x2) * n, (go - 0.002 * x2) * N
    e_g = np.abs(gs - gos).max() / max(np.abs(gs).max(), np.abs(gos).max())
    l2 = 0.001 * float(x2 @ x2)
    ms, mos = (f - l2) * n, (fo - l2) * N
    e_f = abs(ms - mos) / max(abs(ms), abs(mos))
    print("gradient sums %.3e squared-error sums %.3e" % (e_g, e_f))
    assert e_g <= TOL
    assert e_f <= TOL


# 6. hand-off to the policy update
def test_hand_off_to_update():
    layers, lens, first = [15, 16, 16, 3], (63, 64, 65, 1, 128, 7), 100          # first: inside episode 1
    x, observ, reward, boot_observ = R.inputs(lens)
    n = sum(lens) - first - 28                                                    # ends inside episode 4
    th, obs = synth.make_theta(layers), synth.make_obs(n, layers[0])
    std = np.ones(layers[-1])
    mean, action, _ = synth.make_rollout(layers, "lttl", th, obs, std)
    with trpo_amd.Baseline(BASE, AC) as b:
        adv, _, _ = run(b, lens, 128, "alternate", 0.995, 0.98)
        with trpo_amd.Context(layers, "lttl", th, obs, std, 0.1) as ctx:
            ctx.set_rollout_from(b, mean, action, first)
            r = ctx.update()
    with trpo_amd.Context(layers, "lttl", th, obs, std, 0.1) as host:
        host.set_rollout(mean, action, adv[first:first + n])
        s = host.update()
    for k in ("theta", "b", "x"):
        np.testing.assert_array_equal(r[k], s[k])


# 7. refusals
def expect_invalid(fn):
    with pytest.raises(trpo_amd.TRPOError) as e:
        fn()
    assert e.value.code == TRPO_E_INVALID
    assert trpo_amd.last_error()


def test_refusals():
    layers, lens = [15, 16, 16, 3], (63, 64, 65)
    x, observ, reward, boot_observ = R.inputs(lens)
    n = sum(lens)
    th, obs = synth.make_theta(layers), synth.make_obs(n, layers[0])
    std = np.ones(layers[-1])
    mean, action, _ = synth.make_rollout(layers, "lttl", th, obs, std)
    flags = np.ones(3, np.uint8)
    L = trpo_amd.lib()
    with trpo_amd.Baseline(BASE, AC) as b, trpo_amd.Context(layers, "lttl", th, obs, std, 0.1) as ctx:
        # a zero length (the arrays still hold n samples), a horizon below the longest episode, flags
        # without observations, no lengths at all
        expect_invalid(lambda: b.advantage_ragged(x, observ, reward, (63, 0, 64, 65), 65))
        expect_invalid(lambda: b.advantage_ragged(x, observ, reward, lens, 64))
        expect_invalid(lambda: b.advantage_ragged(x, observ, reward, lens, 65, boot=flags))
        assert L.trpo_baseline_advantage_ragged(b._h, x, observ, reward, 3, None, 65, None, None, 0.995, 0.98, None,
                                                None, None) == TRPO_E_INVALID
        assert trpo_amd.last_error()
        expect_invalid(lambda: b.set_data_ragged(observ, reward, (63, 0, 64, 65), 65))
        expect_invalid(lambda: b.set_data_ragged(observ, reward, lens, 64))
        # the object never completed a stage: nothing to hand off
        expect_invalid(lambda: ctx.set_rollout_from(b, mean, action))
        # a valid call after the refusals works, and so does the hand-off
        ref = R.reference(lens, 65, "all", 0.995, 0.98)
        adv, ret, info = b.advantage_ragged(x, observ, reward, lens, 65, boot_observ=boot_observ, boot=flags)
        check_against_reference(adv, ret, info, ref)
        ctx.set_rollout_from(b, mean, action)
        # a refusal for arguments leaves the completed stage as it is
        expect_invalid(lambda: b.advantage_ragged(x, observ, reward, lens, 64))
        ctx.set_rollout_from(b, mean, action)
