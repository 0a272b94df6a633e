"""The device-resident loop: act / act_record on device arrays, the episode scan, the advantage
stage on device rewards -- bit for bit against the host-pointer calls on a second context.  No tolerance appears:
fp64 device outputs are the host calls' bits, fp32 ones are np.float32() of them (one rounding to nearest even)."""
import numpy as np
import pytest

import devloop_ref
import test_gpu_record as R
import trpo_amd
from trpo_amd import devmem

pytestmark = pytest.mark.gpu

SEED = R.SEED
ARM = R.ARM
same_bits = R.same_bits


def dev(a, dtype=None):
    return devmem.DeviceArray.from_host(np.ascontiguousarray(a, dtype or np.asarray(a).dtype), device=0)


def observations(m, L0, dtype, seed=3, extremes=True):
    """rows for the dtype's path: fp32-representable values when dtype is float32, with zero and normal fp32
    magnitudes from 1e-30 to 1e30 among them"""
    obs = R.draws(m, L0, seed).copy()
    if dtype == np.float32:
        obs = obs.astype(np.float32)
    if dtype == np.float32 and extremes:
        flat = obs.reshape(-1)
        for i, v in enumerate((0.0, 1e-30, 1e30, -1e30, -1e-30)):
            flat[(7 * i + 1) % flat.size] = v
    return obs


def as_dtype(x, dtype):
    """what a device output of `dtype` must hold for the fp64 host result x"""
    return np.asarray(x, np.float64).astype(dtype)


def same_out(got, want64, dtype, what):
    want = as_dtype(want64, dtype)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what


def act_dev_call(ctx, obs, dtype, row0, stride, step=3, sample=True, logp=True, keep=False, stream=None, record=False):
    m, A = obs.shape[0], ctx.layers[-1]
    d_obs = dev(obs, dtype)
    d_mean = devmem.DeviceArray((m, A), dtype, 0)
    d_act = devmem.DeviceArray((m, A), dtype, 0) if sample else None
    d_lp = devmem.DeviceArray((m,), dtype, 0) if sample and logp else None
    if record:
        ctx.act_record_dev(d_obs, d_mean, d_act, d_lp, seed=SEED, step=step, row0=row0, row_stride=stride, dtype=dtype,
                           stream=stream)
    else:
        ctx.act_dev(d_obs, d_mean, d_act, d_lp, seed=SEED, step=step, row0=row0, row_stride=stride, keep=keep,
                    dtype=dtype, stream=stream)
    if stream is None:
        ctx.synchronize()
    else:
        stream.synchronize()
    return (d_mean.to_host(), None if d_act is None else d_act.to_host(), None if d_lp is None else d_lp.to_host())


# ---- 1. act outputs ----------------------------------------------------------------------------------------
SCRATCH = ((376, 128, 64, 17), "lttl")                 # 8 * 585 * 65 B > 160 KiB: the lane form's rows in the global scratch
ACT_CASES = [pytest.param(ARM, f, m, id="%s-%d" % (f, m)) for f in ("lane", "neuron") for m in (1, 5, 65, 4101)] + \
    [pytest.param(ARM, "lane", 65606, id="lane-65606")] + \
    [pytest.param(SCRATCH, "lane", m, id="scratch-lane-%d" % m) for m in (5, 65)]


def test_the_scratch_shape_is_one():
    assert 8 * sum(SCRATCH[0]) * 65 > 160 * 1024 >= 8 * sum(ARM[0]) * 65


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("shape,form,m", ACT_CASES)
def test_act_dev_is_act(shape, form, m, dtype):
    obs = observations(m, shape[0][0], dtype)
    row0, stride = 5, 3
    with R.context(shape, R.old_batch(shape), act_form=form) as a, \
            R.context(shape, R.old_batch(shape), act_form=form) as b:
        want = b.act(obs.astype(np.float64), SEED, 3, row0=row0, row_stride=stride)
        got = act_dev_call(a, obs, dtype, row0, stride)
        for g, w, what in zip(got, want, ("mean", "action", "logp")):
            same_out(g, w, dtype, what)
        if shape is SCRATCH:                            # the plain device path's REC kernels on scratch rows
            a.record_begin(row0 + stride * m)
            b.record_begin(row0 + stride * m)
            want_rec = b.act_record(obs.astype(np.float64), SEED, 3, row0=row0, row_stride=stride)
            got_rec = act_dev_call(a, obs, dtype, row0, stride, record=True)
            for g, w, what in zip(got_rec, want_rec, ("mean", "action", "logp")):
                same_out(g, w, dtype, "recorded " + what)
            assert a.record_info() == b.record_info() == (row0 + stride * m, m)
        if m == 65:
            st = devmem.Stream(0)
            mean_only = act_dev_call(a, obs, dtype, row0, stride, sample=False, stream=st)
            same_out(mean_only[0], want[0], dtype, "means only")
            assert mean_only[1] is None and mean_only[2] is None
            no_logp = act_dev_call(a, obs, dtype, row0, stride, logp=False, stream=st)
            same_out(no_logp[1], want[1], dtype, "action without logp")


# ---- 2. record and commit ----------------------------------------------------------------------------------
def record_dev(ctx, observ, num_ep, ep_len, dtype, stream):
    A = ctx.layers[-1]
    ep = observ.reshape(num_ep, ep_len, -1)
    out = [np.zeros((num_ep, ep_len, A), dtype), np.zeros((num_ep, ep_len, A), dtype), np.zeros((num_ep, ep_len), dtype)]
    for t in range(ep_len):
        got = act_dev_call(ctx, ep[:, t], dtype, t, ep_len, step=t, stream=stream, record=True)
        for o, g in zip(out, got):
            o[:, t] = g
    return out[0].reshape(-1, A), out[1].reshape(-1, A), out[2].reshape(-1)


RECORD_KINDS = {
    "default": dict(shape=ARM, kw={}),
    "wide": dict(shape=ARM, kw=dict(form="wide")),
    "inference": dict(shape=((376, 128, 64, 17), "lttl"), kw={}),
}


@pytest.mark.parametrize("kind,num_ep,ep_len,dtype", [
    ("default", 7, 3, np.float64), ("default", 5, 66, np.float64), ("default", 7, 3, np.float32),
    ("default", 5, 66, np.float32), ("wide", 7, 3, np.float64), ("wide", 7, 3, np.float32),
    ("inference", 7, 3, np.float64)])
def test_record_dev_commit_is_the_host_record(kind, num_ep, ep_len, dtype):
    k = RECORD_KINDS[kind]
    shape, n = k["shape"], num_ep * ep_len
    observ = observations(n, shape[0][0], dtype, seed=9, extremes=False)      # an update follows
    wide64 = observ.astype(np.float64)
    st = devmem.Stream(0)
    old = R.draws(37, shape[0][0], 5)
    with R.context(shape, old, **k["kw"]) as a, R.context(shape, old, **k["kw"]) as b:
        a.record_begin(n)
        b.record_begin(n)
        got = record_dev(a, observ, num_ep, ep_len, dtype, st)
        want = R.record_steps(b, wide64, num_ep, ep_len)
        for g, w, what in zip(got, want, ("mean", "action", "logp")):
            same_out(g, w, dtype, what)
        assert a.record_info() == b.record_info() == (n, n)
        a.record_commit()
        b.record_commit()
        if kind == "inference":
            ma, mb = a.act(wide64[:9], SEED, 1), b.act(wide64[:9], SEED, 1)
            for x, y in zip(ma, mb):
                same_bits(x, y, "act after the commit")
            return
        adv = R.draws(n, 1, 21).reshape(-1)
        for c in (a, b):
            c.set_rollout_acted(adv=adv)
        R.same_update(a.update(), b.update())
        for c in (a, b):
            c.set_theta(R.policy(tuple(shape[0])))
            c.set_rollout_acted(adv=adv)
        R.same_update(a.update(kl_cap=float("inf")), b.update(kl_cap=float("inf")), R.KL_KEYS)


# ---- 3. episode scan ---------------------------------------------------------------------------------------
def flags_case(num_env, slot_rows, seed):
    rng = np.random.default_rng(seed)
    term, trun = np.zeros((num_env, slot_rows), np.uint8), np.zeros((num_env, slot_rows), np.uint8)
    last = slot_rows - 1
    plans = [("t0", 0), ("last", last), ("none", None), ("several", None), ("255", None), ("term", None),
             ("trunc", None), ("both", None), ("trunc_first", None)]
    for e in range(num_env):
        kind, _ = plans[e % len(plans)]
        t = int(rng.integers(0, slot_rows))
        if kind == "t0":
            term[e, 0] = 1
        elif kind == "last":
            trun[e, last] = 1
        elif kind == "several":
            term[e, rng.integers(0, slot_rows, 3)] = 1
            trun[e, rng.integers(0, slot_rows, 3)] = 1
        elif kind == "255":
            term[e, t] = 255
        elif kind == "term":
            term[e, t] = 1
        elif kind == "trunc":
            trun[e, t] = 1
        elif kind == "both":
            term[e, t] = trun[e, t] = 1
        elif kind == "trunc_first":
            trun[e, t] = 1
            term[e, min(t + 1, last)] = 1
    return term.reshape(-1), trun.reshape(-1)


@pytest.mark.parametrize("slot_rows", (1, 63, 64, 65, 130))
@pytest.mark.parametrize("num_env", (1, 5, 9))
def test_episode_scan_is_the_rule(num_env, slot_rows):
    term, trun = flags_case(num_env, slot_rows, 100 * num_env + slot_rows)
    st = devmem.Stream(0)
    with R.context(ARM, R.old_batch(ARM)) as ctx:
        d_term, d_trun = dev(term), dev(trun)
        for tr_h, tr_d in ((trun, d_trun), (None, None)):
            got = ctx.record_episodes_dev(d_term, tr_d, num_env, slot_rows, stream=st)
            want = devloop_ref.episodes(term, tr_h, num_env, slot_rows)
            assert np.array_equal(got[0], want[0]), (got[0], want[0])
            assert np.array_equal(got[1], want[1]), (got[1], want[1])


# ---- 4. advantages -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("num_ep,ep_len", [(7, 3), (3, 130)])
def test_fixed_advantage_on_device_rewards(num_ep, ep_len, dtype):
    n, O = num_ep * ep_len, ARM[0][0]
    observ = R.draws(n, O, 9)
    base, bac, x, reward = R.baseline_problem(O, n)
    reward = reward.astype(dtype)
    st = devmem.Stream(0)
    with R.context(ARM, observ) as a, R.context(ARM, observ) as b, trpo_amd.Baseline(base, bac, 0) as bla, \
            trpo_amd.Baseline(base, bac, 0) as blb:
        d_rew = devmem.DeviceArray((n,), dtype, 0)
        d_rew.copy_from_host(reward, stream=st)
        got = bla.advantage_from_dev(a, x, d_rew, num_ep, ep_len, dtype=dtype, stream=st)
        want = blb.advantage_from(b, x, reward.astype(np.float64), num_ep, ep_len)
        R.same_stage(got, want)
        R.same_baseline_state(bla, blb, x)
        for c, bl in ((a, bla), (b, blb)):
            c.act(observ, SEED, 0, keep=True)
            c.set_rollout_acted(baseline=bl)
        R.same_update(a.update(), b.update())


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
def test_ragged_advantage_from_the_scan(dtype):
    slot, lens_want, O = 66, np.array([1, 64, 65, 66, 2], np.uintp), ARM[0][0]
    num_ep, n = lens_want.size, int(lens_want.sum())
    term, trun = np.zeros((num_ep, slot), np.uint8), np.zeros((num_ep, slot), np.uint8)
    term[0, 0] = 1
    trun[1, 63] = 1                      # truncated by its flag
    term[2, 64] = 1
    term[4, 1] = 1                       # episode 3 never ends: the slot runs out, truncated
    rng = np.random.default_rng(77)
    slots_obs = observations(num_ep * slot, O, dtype, seed=31, extremes=False)
    reward_slots = (-np.abs(rng.normal(1.0, 0.7, (num_ep, slot)))).astype(dtype)
    last_obs = (0.5 * rng.normal(size=(num_ep, O))).astype(dtype)
    base, bac, x, _ = R.baseline_problem(O, n)
    st = devmem.Stream(0)
    old = R.old_batch(ARM)
    with R.context(ARM, old) as a, R.context(ARM, old) as b, trpo_amd.Baseline(base, bac, 0) as bla, \
            trpo_amd.Baseline(base, bac, 0) as blb:
        lens, boot = a.record_episodes_dev(dev(term.reshape(-1)), dev(trun.reshape(-1)), num_ep, slot, stream=st)
        assert np.array_equal(lens, lens_want) and list(boot) == [0, 1, 0, 1, 0]
        a.record_begin(num_ep * slot)
        b.record_begin(num_ep * slot)
        record_dev(a, slots_obs, num_ep, slot, dtype, st)
        R.record_steps(b, slots_obs.astype(np.float64), num_ep, slot)
        a.record_commit_ragged(lens, slot)
        b.record_commit_ragged(lens, slot)
        packed = np.concatenate([reward_slots[e, :lens[e]] for e in range(num_ep)]).astype(np.float64)
        d_rew, d_last = devmem.DeviceArray((num_ep, slot), dtype, 0), devmem.DeviceArray((num_ep, O), dtype, 0)
        d_rew.copy_from_host(reward_slots, stream=st)
        d_last.copy_from_host(last_obs, stream=st)
        got = bla.advantage_ragged_from_dev(a, x, d_rew, lens, slot, slot, last_obs_dev=d_last, boot=boot, dtype=dtype,
                                            stream=st)
        want = blb.advantage_ragged_from(b, x, packed, lens, slot, boot_observ=last_obs.astype(np.float64), boot=boot)
        R.same_stage(got, want)
        R.same_baseline_state(bla, blb, x)
        for c, bl in ((a, bla), (b, blb)):
            c.set_rollout_acted(baseline=bl)
        R.same_update(a.update(), b.update())


# ---- 5. ordering -------------------------------------------------------------------------------------------
def test_stream_order():
    """act_dev runs behind a long copy on the caller's stream and ahead of the copy back; only that stream is
    synchronised.  A smoke of the contract, not a proof."""
    m, L0, A = 65, ARM[0][0], ARM[0][-1]
    obs = R.draws(m, L0, 13)
    big_n = 4 * 1024 * 1024                            # 32 MB of doubles ahead of the rows
    th2 = R.policy(tuple(ARM[0]), 1)
    with R.context(ARM, R.old_batch(ARM)) as a, R.context(ARM, R.old_batch(ARM)) as b:
        want1 = b.act(obs, SEED, 3, row0=2, row_stride=2)
        st = devmem.Stream(0)
        pin = devmem.PinnedArray(big_n + m * L0)
        pin.array[big_n:] = obs.reshape(-1)
        big = devmem.DeviceArray(big_n + m * L0, np.float64, 0)
        d_obs = devmem.DeviceArray((m, L0), np.float64, 0)
        d_out = devmem.DeviceArray(m * (2 * A + 1), np.float64, 0)
        d_mean, d_act, d_lp = d_out.view(0, (m, A)), d_out.view(m * A, (m, A)), d_out.view(2 * m * A, (m,))
        out = devmem.PinnedArray(m * (2 * A + 1))
        big.copy_from_host(pin.array, stream=st)
        d_obs.copy_from_device(big.view(big_n, (m, L0)), stream=st)
        a.act_dev(d_obs, d_mean, d_act, d_lp, seed=SEED, step=3, row0=2, row_stride=2, stream=st)
        d_out.to_host(out.array, stream=st)
        st.synchronize()
        got = out.array.copy()
        same_bits(got[:m * A].reshape(m, A), want1[0], "mean")
        same_bits(got[m * A:2 * m * A].reshape(m, A), want1[1], "action")
        same_bits(got[2 * m * A:], want1[2], "logp")
        # set_theta between two calls: the second runs on the new weights
        b.set_theta(th2)
        want2 = b.act(obs, SEED, 4, row0=2, row_stride=2)
        a.act_dev(d_obs, d_mean, d_act, d_lp, seed=SEED, step=3, row0=2, row_stride=2, stream=st)
        a.set_theta(th2)
        a.act_dev(d_obs, d_mean, d_act, d_lp, seed=SEED, step=4, row0=2, row_stride=2, stream=st)
        d_out.to_host(out.array, stream=st)
        st.synchronize()
        same_bits(out.array[:m * A].reshape(m, A), want2[0], "mean at the new theta")
        same_bits(out.array[m * A:2 * m * A].reshape(m, A), want2[1], "action at the new theta")
        assert not np.array_equal(want1[0], want2[0])
        for p in (pin, out):
            p.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------
class HostPointer:
    """a numpy array posing as device memory"""

    def __init__(self, a):
        self.a = a
        self.__cuda_array_interface__ = dict(shape=a.shape, typestr=a.dtype.str, data=(a.ctypes.data, False), version=3,
                                             strides=None)


def test_refusals_leave_the_context_usable():
    m, L0, A = 4, ARM[0][0], ARM[0][-1]
    obs = R.draws(m, L0, 3)
    with R.context(ARM, R.old_batch(ARM)) as ctx, R.context(ARM, R.old_batch(ARM)) as ref:
        d_obs, d_mean = dev(obs), devmem.DeviceArray((m, A), np.float64, 0)
        d_act, d_lp = devmem.DeviceArray((m, A), np.float64, 0), devmem.DeviceArray((m,), np.float64, 0)
        h = lambda shape: HostPointer(np.zeros(shape))
        call = lambda *a, **kw: (lambda: ctx.act_dev(*a, seed=SEED, **kw))
        R.expect_invalid(call(h((m, L0)), d_mean, d_act, d_lp), "trpo_ctx_act_dev", "obs_dev")
        R.expect_invalid(call(d_obs, h((m, A)), d_act, d_lp), "trpo_ctx_act_dev", "mean_dev")
        R.expect_invalid(call(d_obs, d_mean, h((m, A)), d_lp), "trpo_ctx_act_dev", "action_dev")
        R.expect_invalid(call(d_obs, d_mean, d_act, h((m,))), "trpo_ctx_act_dev", "logp_dev")
        R.expect_invalid(call(d_obs, d_mean, None, d_lp), "trpo_ctx_act_dev", "logp_dev without action_dev")
        R.expect_invalid(call(d_obs, d_mean, d_act, d_lp, keep=True, row0=37), "kept row")
        R.expect_invalid(lambda: ctx.act_record_dev(d_obs, d_mean, d_act, d_lp, seed=SEED), "trpo_ctx_act_record_dev",
                         "no recording")
        ctx.record_begin(6)
        R.expect_invalid(lambda: ctx.act_record_dev(d_obs, d_mean, d_act, d_lp, seed=SEED, row0=3), "beyond the recording")
        L = trpo_amd.lib()
        rc = L.trpo_ctx_act_dev(ctx._h, d_obs.ptr, m, SEED, 0, 0, 1, 0, 7, d_mean.ptr, d_act.ptr, d_lp.ptr, None)
        assert rc == R.TRPO_E_INVALID and "dtype" in trpo_amd.last_error()
        # an output one element longer than its allocation: a view claims m + 1 rows' worth of logp
        short = devmem.DeviceArray((m,), np.float64, 0)
        o5, m5, a5 = dev(R.draws(m + 1, L0, 3)), devmem.DeviceArray((m + 1, A), np.float64, 0), \
            devmem.DeviceArray((m + 1, A), np.float64, 0)
        rc = L.trpo_ctx_act_dev(ctx._h, o5.ptr, m + 1, SEED, 0, 0, 1, 0, 0, m5.ptr, a5.ptr, short.ptr, None)
        assert rc == R.TRPO_E_INVALID and "logp_dev" in trpo_amd.last_error() and "allocation" in trpo_amd.last_error()
        flags = np.zeros(8, np.uint8)
        R.expect_invalid(lambda: ctx.record_episodes_dev(HostPointer(flags), None, 2, 4), "terminated_dev")
        R.expect_invalid(lambda: ctx.record_episodes_dev(dev(flags), HostPointer(flags), 2, 4), "truncated_dev")
        # and the context still works
        ctx.act_dev(d_obs, d_mean, d_act, d_lp, seed=SEED, step=2)
        ctx.synchronize()
        want = ref.act(obs, SEED, 2)
        same_bits(d_mean.to_host(), want[0], "mean")
        same_bits(d_act.to_host(), want[1], "action")
        same_bits(d_lp.to_host(), want[2], "logp")


def test_advantage_refusals():
    num_ep, ep_len, O = 7, 3, ARM[0][0]
    n = num_ep * ep_len
    observ = R.draws(n, O, 9)
    base, bac, x, reward = R.baseline_problem(O, n)
    with R.context(ARM, observ) as a, trpo_amd.Baseline(base, bac, 0) as bl:
        R.expect_invalid(lambda: bl.advantage_from_dev(a, x, HostPointer(np.array(reward)), num_ep, ep_len),
                         "trpo_baseline_advantage_ctx_dev", "reward_dev")
        short = dev(np.array(reward[:n - 1]))
        L = trpo_amd.lib()
        t = L.trpo_baseline_advantage_ctx_dev(bl._h, x.ctypes.data, a._h, short.ptr, 0, num_ep, ep_len, 0.99, 0.95, None,
                                              None, None, None)
        assert t == R.TRPO_E_INVALID and "allocation" in trpo_amd.last_error()
        got = bl.advantage_from_dev(a, x, dev(np.array(reward)), num_ep, ep_len)
        with trpo_amd.Baseline(base, bac, 0) as blb:
            R.same_stage(got, blb.advantage_from(a, x, reward, num_ep, ep_len))
