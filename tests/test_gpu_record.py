"""MI355X tests of the rollout record (trpo_ctx_record_begin / _act_record / _record_commit[_ragged] / _record_info,
trpo_baseline_advantage[_ragged]_ctx).

Every comparison is bit for bit against the project's host path on a second context: context A records and
commits; context B is fed the arrays A's act_record calls returned -- set_obs(Observ), set_rollout(mean, action,
adv) -- and the baseline on B's side gets advantage(Observ, ...).  No tolerance appears anywhere.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import act_edges as E
import ragged_ref as RR
import trpo_amd
from trpo_amd import synth

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
TRPO_E_INVALID = -1
ARM = ((15, 16, 16, 3), "lttl")
UPDATE_KEYS = ("theta", "b", "x", "shs", "lagrange", "gnorm", "fval", "rate", "accepted", "evaluated", "actual",
               "expected", "ratio", "cg_iters")
KL_KEYS = UPDATE_KEYS + ("kl", "entropy_old", "entropy_new", "kl_rejected")


def same_bits(a, b, what=""):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


def same_update(r, s, keys=UPDATE_KEYS):
    for key in keys:
        same_bits(r[key], s[key], key)


def same_stage(r, s):
    """(adv, ret, info) of two advantage calls"""
    same_bits(r[0], s[0], "adv")
    same_bits(r[1], s[1], "ret")
    for key in ("ep_rew_mean", "ep_rew_std", "adv_mean", "adv_std"):
        same_bits(r[2][key], s[2][key], key)


def same_baseline_state(bl_a, bl_b, x):
    """(observ, target) through the objective, its gradient and the predictions; then one fit step"""
    for got, want in zip(bl_a.evaluate(x, want_predict=True), bl_b.evaluate(x, want_predict=True)):
        same_bits(got, want, "evaluate")
    fa, fb = bl_a.fit_tr(x), bl_b.fit_tr(x)
    same_bits(fa[0], fb[0], "fit_tr x_out")
    same_bits(fa[1], fb[1], "fit_tr step")
    assert fa[2].accepted == fb[2].accepted


@functools.lru_cache(maxsize=None)
def policy(layers, seed=0):
    """theta with non-zero biases and LogStd (tests/test_gpu_act.py's recipe)"""
    rng = np.random.default_rng(300 + seed)
    th = synth.make_theta(list(layers)) + 0.05 * rng.normal(size=synth.num_params(list(layers)))
    th[-layers[-1]:] = rng.uniform(-1.0, 0.5, layers[-1])
    th.setflags(write=False)
    return th


@functools.lru_cache(maxsize=None)
def draws(n, width, seed):
    a = 0.5 * np.random.default_rng(seed).normal(size=(n, width))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def vectors(layers):
    P = synth.num_params(list(layers))
    return synth.make_v(P), synth.make_b(P)


@functools.lru_cache(maxsize=None)
def baseline_problem(O, n, seed=11):
    """(layers, activations, x, reward) of a baseline on O observations"""
    rng = np.random.default_rng(seed)
    base = (O + 1, 16, 16, 1)
    x = 0.3 * rng.normal(size=synth.num_params(list(base)) - 1)
    reward = -np.abs(rng.normal(1.0, 0.7, n))
    x.setflags(write=False)
    reward.setflags(write=False)
    return list(base), "lttl", x, reward


@contextlib.contextmanager
def context(shape, obs, act_form=None, **kw):
    """A context on `obs` whose std is the policy's own exp(LogStd); act_form: TRPO_ACT_FORM at its creation."""
    layers, ac = shape
    th = policy(tuple(layers))
    saved = os.environ.pop("TRPO_ACT_FORM", None)
    if act_form:
        os.environ["TRPO_ACT_FORM"] = act_form
    try:
        ctx = trpo_amd.Context(list(layers), ac, th, obs, np.exp(th[-layers[-1]:]), 0.1, **kw)
    finally:
        os.environ.pop("TRPO_ACT_FORM", None)
        if saved is not None:
            os.environ["TRPO_ACT_FORM"] = saved
    with ctx:
        yield ctx


def expect_invalid(fn, *words):
    with pytest.raises(trpo_amd.TRPOError) as e:
        fn()
    assert e.value.code == TRPO_E_INVALID, e.value
    for w in words:
        assert w in str(e.value), e.value


def record_steps(ctx, observ, num_ep, ep_len, seed=SEED, step_of=lambda t: t):
    """Observ [n][L0] episode-major, recorded as a vectorised environment delivers it: one call per time step
    with the num_ep rows t, t + ep_len, ...  Returns (mean [n][A], action [n][A], logp [n]) as the calls gave them."""
    A = ctx.layers[-1]
    ep = observ.reshape(num_ep, ep_len, -1)
    mean, action, logp = np.zeros((num_ep, ep_len, A)), np.zeros((num_ep, ep_len, A)), np.zeros((num_ep, ep_len))
    for t in range(ep_len):
        mean[:, t], action[:, t], logp[:, t] = ctx.act_record(ep[:, t], seed, step_of(t), row0=t, row_stride=ep_len)
    return mean.reshape(-1, A), action.reshape(-1, A), logp.reshape(-1)


def old_batch(shape):
    return draws(37, shape[0][0], 5)


# ------------------------------------------------------------------------------------------------------------
# outputs
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [11000, 12000], ids=["pinned-11000", "staged-12000"])
@pytest.mark.parametrize("form", ["lane", "neuron"])
def test_outputs_are_acts_bits(form, m):
    """(mean, action, logp) of act_record == act's for the same (seed, step, rows), both kernel forms, both
    transfer paths; the rows strided, so the Philox row is not the sample index."""
    assert E.pinned(list(ARM[0]), 11000) and not E.pinned(list(ARM[0]), 12000)
    obs = draws(12000, 15, 21)[:m]
    with context(ARM, old_batch(ARM), act_form=form) as ctx:
        ctx.record_begin(5 + 2 * m)
        got = ctx.act_record(obs, SEED, 3, row0=5, row_stride=2)
        want = ctx.act(obs, SEED, 3, row0=5, row_stride=2)
        assert ctx.record_info() == (5 + 2 * m, m)
    for g, w, name in zip(got, want, ("mean", "action", "logp")):
        same_bits(g, w, name)


def test_inference_only_context_records_and_commits():
    """[376,128,64,17] is beyond the default solver: its context serves inference and the setters, and a commit
    there is what set_obs is there"""
    shape = ((376, 128, 64, 17), "lttl")
    obs = draws(70, 376, 23)
    with context(shape, old_batch(shape)) as ctx:
        ctx.record_begin(70)
        got = [np.concatenate(p) for p in zip(ctx.act_record(obs[:64], SEED, 2), ctx.act_record(obs[64:], SEED, 2, row0=64))]
        ctx.record_commit()
        assert ctx.n == 70 and ctx.record_info() == (0, 0)
        for g, w in zip(got, ctx.act(obs, SEED, 2, keep=True)):          # rows < n = 70 are the context's now
            same_bits(g, w)
        expect_invalid(lambda: ctx.act_record(obs[:1], SEED), "no recording")


# ------------------------------------------------------------------------------------------------------------
# the fixed commit, on every kind of context
# ------------------------------------------------------------------------------------------------------------
KINDS = {
    "default": dict(shape=ARM, num_ep=7, ep_len=47, kw={}),                       # n = 329: no multiple of 16
    "wide": dict(shape=((17, 33, 65, 5), "ltsl"), num_ep=10, ep_len=13, kw=dict(form="wide")),
    # (the generic kernel keeps no forward cache and its launches are not counted)
    "generic": dict(shape=((6, 20, 12, 9, 2), "ltstl"), num_ep=10, ep_len=15, kw={}, fwd=0),
    "fp64": dict(shape=ARM, num_ep=7, ep_len=47, kw=dict(precision="fp64")),
}


def recorded_path(kind, commit="fixed"):
    """record -> commit -> advantage_from -> set_rollout_acted -> fvp, cg, update on context A"""
    k = KINDS[kind]
    shape, num_ep, ep_len = k["shape"], k["num_ep"], k["ep_len"]
    n, L0 = num_ep * ep_len, shape[0][0]
    observ = draws(n, L0, 31)
    base, bac, x, reward = baseline_problem(L0, n)
    v, b = vectors(shape[0])
    out = dict(observ=observ)
    with context(shape, old_batch(shape), **k["kw"]) as A, trpo_amd.Baseline(base, bac) as bl:
        A.fvp(v)                                        # the old batch's forward cache is valid
        A.record_begin(n)
        out["mean"], out["action"], out["logp"] = record_steps(A, observ, num_ep, ep_len)
        assert A.record_info() == (n, n)
        if commit == "fixed":
            A.record_commit()
        else:
            A.record_commit_ragged([ep_len] * num_ep, ep_len)
        assert A.n == n and A.record_info() == (0, 0)
        f0 = A.forward_passes
        out["fvp"] = A.fvp(v)
        out["fwd"] = A.forward_passes - f0
        out["cg"] = A.cg(b, 10, 1e-10)
        out["stage"] = bl.advantage_from(A, x, reward, num_ep, ep_len)
        A.set_rollout_acted(baseline=bl)
        out["update"] = A.update()
        out["predict"] = bl.evaluate(x, want_predict=True)
    return out


def host_path(kind, rec):
    """the same on context B from the arrays A's calls returned"""
    k = KINDS[kind]
    shape, num_ep, ep_len = k["shape"], k["num_ep"], k["ep_len"]
    n, L0 = num_ep * ep_len, shape[0][0]
    base, bac, x, reward = baseline_problem(L0, n)
    v, b = vectors(shape[0])
    out = {}
    with context(shape, old_batch(shape), **k["kw"]) as B, trpo_amd.Baseline(base, bac) as bl:
        B.set_obs(rec["observ"])
        out["acted"] = B.act(rec["observ"], SEED, 0, keep=True)      # (the steps differ: rows compared below)
        out["fvp"] = B.fvp(v)
        out["cg"] = B.cg(b, 10, 1e-10)
        out["stage"] = bl.advantage(x, rec["observ"], reward, num_ep, ep_len)
        B.set_rollout(rec["mean"], rec["action"], out["stage"][0])
        out["update"] = B.update()
        out["predict"] = bl.evaluate(x, want_predict=True)
    return out


def check_paths(rec, host, fwd=1):
    assert rec["fwd"] == fwd                            # the commit invalidated the forward cache
    same_bits(rec["fvp"], host["fvp"], "fvp")
    same_bits(rec["cg"], host["cg"], "cg")
    same_stage(rec["stage"], host["stage"])
    same_update(rec["update"], host["update"])
    for got, want in zip(rec["predict"], host["predict"]):
        same_bits(got, want, "baseline state")
    same_bits(rec["mean"], host["acted"][0], "mean")    # the mean does not depend on the generator


@pytest.mark.parametrize("kind", list(KINDS))
def test_fixed_commit_is_the_host_path(kind):
    rec = recorded_path(kind)
    check_paths(rec, host_path(kind, rec), KINDS[kind].get("fwd", 1))


def test_repeatable():
    r, s = recorded_path("default"), recorded_path("default")
    for key in ("mean", "action", "logp", "fvp", "cg"):
        same_bits(r[key], s[key], key)
    same_stage(r["stage"], s["stage"])
    same_update(r["update"], s["update"])


def test_equal_lengths_ragged_commit_is_the_fixed_commit():
    r, s = recorded_path("default", "ragged"), recorded_path("default", "fixed")
    for key in ("mean", "action", "logp", "fvp", "cg"):
        same_bits(r[key], s[key], key)
    same_stage(r["stage"], s["stage"])
    same_update(r["update"], s["update"])


# ------------------------------------------------------------------------------------------------------------
# grids that wrap
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,m", [("neuron", 4101), ("lane", 65606)], ids=["neuron-4101", "lane-65606"])
def test_one_call_past_the_grid(form, m):
    """one act_record call whose blocks take a second trip (tests/act_edges.py: 1024 blocks of 4 / 64 rows);
    the record's observation and kept rows through fvp and the policy gradient"""
    assert m > E.GRID * (E.NEURON_ROWS if form == "neuron" else E.LANE_ROWS)
    obs = draws(65606, 15, 41)[:m]
    adv = synth.normal(synth.SEED, synth.STREAM_ADV, m)
    v, _ = vectors(ARM[0])
    with context(ARM, old_batch(ARM), act_form=form) as A:
        A.record_begin(m)
        mean, action, logp = A.act_record(obs, SEED, 9)
        A.record_commit()
        z = A.fvp(v)
        A.set_rollout_acted(adv)
        r = A.update()
    with context(ARM, obs, act_form=form) as B:
        for g, w in zip((mean, action, logp), B.act(obs, SEED, 9)):
            same_bits(g, w)
        same_bits(z, B.fvp(v), "fvp")
        B.set_rollout(mean, action, adv)
        same_update(r, B.update())


# ------------------------------------------------------------------------------------------------------------
# the ragged commit
# ------------------------------------------------------------------------------------------------------------
def test_ragged_commit_packs_the_slots():
    """episodes of 1, 128, 129, 200 and 7 steps in slots of 200 rows (1 and slot_rows among the lengths, every
    other one shorter); the first ten steps are recorded for every slot, so episode 0 holds nine rows past its
    length, which must not appear; alternate episodes truncated"""
    lens = RR.LENGTHS["1-128-129-200-7"]
    slot, num_ep, n = 200, len(lens), sum(lens)
    assert 1 in lens and slot in lens and sorted(lens)[-2] < slot
    x, observ, reward, boot_observ = RR.inputs(lens)
    boot = RR.boot_flags("alternate", num_ep)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    junk = draws(num_ep * slot, 15, 51).reshape(num_ep, slot, 15)
    v, _ = vectors(ARM[0])
    mean, action = np.zeros((n, 3)), np.zeros((n, 3))
    with context(ARM, old_batch(ARM)) as A, trpo_amd.Baseline(list(RR.BASE), RR.AC) as bl:
        A.record_begin(num_ep * slot + 3)               # rows beyond the slots are nobody's
        for t in range(slot):
            live = [e for e in range(num_ep) if t < lens[e] or t < 10]
            assert live == list(range(live[0], live[-1] + 1))
            rows = np.stack([observ[off[e] + t] if t < lens[e] else junk[e, t] for e in live])
            m, a, _ = A.act_record(rows, SEED, t, row0=live[0] * slot + t, row_stride=slot)
            for i, e in enumerate(live):
                if t < lens[e]:
                    mean[off[e] + t], action[off[e] + t] = m[i], a[i]
        assert A.record_info() == (num_ep * slot + 3, n + 9 + 3)     # episode 0: 9 rows, episode 4: 3 rows past
        A.record_commit_ragged(lens, slot)
        assert A.n == n and A.record_info() == (0, 0)
        z = A.fvp(v)
        stage = bl.advantage_ragged_from(A, x, reward, lens, slot, boot_observ=boot_observ, boot=boot)
        A.set_rollout_acted(baseline=bl)
        r = A.update(kl_cap=float("inf"))
        pred = bl.evaluate(x, want_predict=True)
    with context(ARM, old_batch(ARM)) as B, trpo_amd.Baseline(list(RR.BASE), RR.AC) as bl:
        B.set_obs(observ)
        same_bits(z, B.fvp(v), "fvp")
        want = bl.advantage_ragged(x, observ, reward, lens, slot, boot_observ=boot_observ, boot=boot)
        same_stage(stage, want)
        B.set_rollout(mean, action, want[0])
        same_update(r, B.update(kl_cap=float("inf")), KL_KEYS)
        for got, w in zip(pred, bl.evaluate(x, want_predict=True)):
            same_bits(got, w, "baseline state")


# ------------------------------------------------------------------------------------------------------------
# advantage_from on a batch that came up by set_obs
# ------------------------------------------------------------------------------------------------------------
def test_advantage_from_after_set_obs():
    num_ep, ep_len = 9, 23
    n = num_ep * ep_len
    observ = draws(n, 15, 61)
    base, bac, x, reward = baseline_problem(15, n)
    with context(ARM, old_batch(ARM)) as ctx, trpo_amd.Baseline(base, bac) as bl_a, \
            trpo_amd.Baseline(base, bac) as bl_b:
        ctx.set_obs(observ)
        same_stage(bl_a.advantage_from(ctx, x, reward, num_ep, ep_len), bl_b.advantage(x, observ, reward, num_ep, ep_len))
        same_baseline_state(bl_a, bl_b, x)
        lens = [ep_len] * num_ep                        # and the ragged entry point on the same batch
        same_stage(bl_a.advantage_ragged_from(ctx, x, reward, lens, 30), bl_b.advantage_ragged(x, observ, reward, lens, 30))
        same_baseline_state(bl_a, bl_b, x)


# ------------------------------------------------------------------------------------------------------------
# overwrite and order
# ------------------------------------------------------------------------------------------------------------
def test_partition_and_overwrite_do_not_show():
    """the rows step by step, and episode by episode in reverse with row 100 recorded first on another
    observation: the same committed state (one step number throughout, so a row's draw is its row's)"""
    num_ep, ep_len = 7, 47
    n = num_ep * ep_len
    observ = draws(n, 15, 31)
    adv = synth.normal(synth.SEED, synth.STREAM_ADV, n)
    v, _ = vectors(ARM[0])
    with context(ARM, old_batch(ARM)) as A:
        A.record_begin(n)
        first = record_steps(A, observ, num_ep, ep_len, step_of=lambda t: 4)
        A.record_commit()
        z = A.fvp(v)
        A.set_rollout_acted(adv)
        r = A.update()
    with context(ARM, old_batch(ARM)) as A:
        A.record_begin(n)
        wrong = A.act_record(draws(1, 15, 77), SEED, 4, row0=100)
        assert A.record_info() == (n, 1)
        second = [np.zeros_like(a) for a in first]
        for e in reversed(range(num_ep)):
            rows = slice(e * ep_len, (e + 1) * ep_len)
            for dst, src in zip(second, A.act_record(observ[rows], SEED, 4, row0=e * ep_len)):
                dst[rows] = src
        assert A.record_info() == (n, n)                # row 100 counts once
        assert not np.array_equal(wrong[0][0], second[0][100])
        A.record_commit()
        same_bits(z, A.fvp(v), "fvp")
        A.set_rollout_acted(adv)
        same_update(r, A.update())
    for a, b in zip(first, second):
        same_bits(a, b)


# ------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    num_ep, ep_len = 5, 8
    n = num_ep * ep_len
    old = old_batch(ARM)
    observ = draws(n, 15, 71)
    adv_old = synth.normal(synth.SEED, synth.STREAM_ADV, old.shape[0])
    v, _ = vectors(ARM[0])
    base, bac, x, reward = baseline_problem(15, n)
    L = trpo_amd.lib()
    with context(ARM, old) as A, trpo_amd.Baseline(base, bac) as bl:
        A.act(old, SEED, 1, keep=True)
        A.set_rollout_acted(adv_old)
        z0, r0 = A.fvp(v), A.update()
        # no recording in progress
        expect_invalid(lambda: A.act_record(observ[:3], SEED), "trpo_ctx_act_record", "no recording")
        expect_invalid(A.record_commit, "trpo_ctx_record_commit", "no recording")
        expect_invalid(lambda: A.record_commit_ragged([1], 1), "trpo_ctx_record_commit_ragged", "no recording")
        expect_invalid(lambda: A.record_begin(0), "trpo_ctx_record_begin")
        assert A.record_info() == (0, 0)
        A.record_begin(n)
        # act_record: a row >= rows, action_out == NULL, and what trpo_ctx_act refuses
        expect_invalid(lambda: A.act_record(observ[:2], SEED, row0=n - 1), "trpo_ctx_act_record", "beyond")
        expect_invalid(lambda: A.act_record(observ[:2], SEED, row0=0, row_stride=n), "trpo_ctx_act_record")
        mean = np.zeros((2, 3))
        assert L.trpo_ctx_act_record(A._h, observ.ctypes.data, 2, 1, 0, 0, 1, mean.ctypes.data, None,
                                     None) == TRPO_E_INVALID
        assert "trpo_ctx_act_record" in trpo_amd.last_error() and "action_out" in trpo_amd.last_error()
        expect_invalid(lambda: A.act_record(np.zeros((0, 15)), SEED), "trpo_ctx_act_record")
        expect_invalid(lambda: A.act_record(observ[:2], SEED, row_stride=0), "trpo_ctx_act_record")
        expect_invalid(lambda: A.act_record(observ[:2], SEED, step=1 << 48), "trpo_ctx_act_record")
        assert A.record_info() == (n, 0)                # none of them recorded anything
        # all rows but row 13
        for first, m in ((0, 13), (14, n - 14)):
            A.act_record(observ[first:first + m], SEED, 2, row0=first)
        assert A.record_info() == (n, n - 1)
        expect_invalid(A.record_commit, "trpo_ctx_record_commit", "row 13 ")
        # the ragged commit's own refusals (episode 1, step 5 is row 13)
        expect_invalid(lambda: A.record_commit_ragged([ep_len] * num_ep, ep_len), "row 13 ")
        expect_invalid(lambda: A.record_commit_ragged([3, 0, 2], ep_len), "ep_len[1]")
        expect_invalid(lambda: A.record_commit_ragged([3, ep_len + 1], ep_len), "ep_len[1]")
        expect_invalid(lambda: A.record_commit_ragged([1] * (num_ep + 1), ep_len), "exceed")
        expect_invalid(lambda: A.record_commit_ragged([], ep_len))
        # (a sum above INT_MAX needs lengths above the slot rows or more slots than rows: refused by those checks)
        # the refused commits changed nothing: the old batch, its rollout and its kept rows serve as before
        assert A.n == old.shape[0] and A.record_info() == (n, n - 1)
        same_bits(A.fvp(v), z0, "fvp on the old batch")
        same_update(A.update(), r0)
        A.set_rollout_acted(adv_old)
        same_update(A.update(), r0)
        # advantage_from: the context still holds the old batch, not this one
        expect_invalid(lambda: bl.advantage_from(A, x, reward, num_ep, ep_len), "trpo_baseline_advantage_ctx", "sample count")
        # filling the gap makes the commit succeed
        A.act_record(observ[13], SEED, 2, row0=13)
        A.record_commit()
        assert A.n == n
        with context(ARM, observ) as B:
            same_bits(A.fvp(v), B.fvp(v), "fvp after the commit")
        # the rollout went with the old batch
        with pytest.raises(trpo_amd.TRPOError):
            A.update()
        # *_ctx refusals: NULL arguments, the observation width, the sample count, and the host calls' own
        for args in ((None, x.ctypes.data, A._h, reward.ctypes.data), (bl._h, None, A._h, reward.ctypes.data),
                     (bl._h, x.ctypes.data, None, reward.ctypes.data), (bl._h, x.ctypes.data, A._h, None)):
            assert L.trpo_baseline_advantage_ctx(*args, num_ep, ep_len, 0.99, 0.95, None, None, None) == TRPO_E_INVALID
            assert "trpo_baseline_advantage_ctx" in trpo_amd.last_error()
        lens = np.array([ep_len] * num_ep, np.uintp)
        assert L.trpo_baseline_advantage_ragged_ctx(bl._h, x.ctypes.data, None, reward.ctypes.data, num_ep,
                                                    lens.ctypes.data, ep_len, None, None, 0.99, 0.95, None, None,
                                                    None) == TRPO_E_INVALID
        assert "trpo_baseline_advantage_ragged_ctx" in trpo_amd.last_error()
        expect_invalid(lambda: bl.advantage_from(A, x, reward[:n - ep_len], num_ep - 1, ep_len), "sample count")
        expect_invalid(lambda: bl.advantage_ragged_from(A, x, reward[:n - 1], [ep_len] * (num_ep - 1) + [ep_len - 1],
                                                        ep_len), "sample count")
        expect_invalid(lambda: bl.advantage_ragged_from(A, x, reward, [ep_len] * num_ep, ep_len - 1), "horizon")
        expect_invalid(lambda: bl.advantage_ragged_from(A, x, reward, [ep_len] * num_ep, ep_len,
                                                        boot=np.ones(num_ep, np.uint8)), "boot_observ")
        expect_invalid(lambda: bl.advantage_from(A, x, reward[:0], 0, ep_len), "trpo_baseline_advantage_ctx")
        with trpo_amd.Baseline([10, 8, 1], "ltl") as other:
            xo = np.zeros(synth.num_params([10, 8, 1]) - 1)
            expect_invalid(lambda: other.advantage_from(A, xo, reward, num_ep, ep_len), "observation width")
        # and after all of them the stage still runs
        bl.advantage_from(A, x, reward, num_ep, ep_len)
        A.set_rollout_acted(baseline=bl)
        A.update()


def test_what_discards_a_recording():
    obs = draws(20, 15, 81)
    with context(ARM, old_batch(ARM)) as A:
        for discard in (lambda: A.set_obs(obs), A.act_clear, lambda: A.record_begin(7)):
            A.record_begin(20)
            A.act_record(obs[:10], SEED)
            assert A.record_info() == (20, 10)
            discard()
            assert A.record_info() in ((0, 0), (7, 0))
            expect_invalid(lambda: A.act_record(obs[10:], SEED, row0=10), "trpo_ctx_act_record")
        assert A.record_info() == (7, 0)
        # set_theta does not: the two halves of a recording may straddle it
        A.record_begin(20)
        first = A.act_record(obs[:10], SEED)
        A.set_theta(policy(ARM[0]))
        assert A.record_info() == (20, 10)
        second = A.act_record(obs[10:], SEED, row0=10)
        A.record_commit()
        v, _ = vectors(ARM[0])
        z = A.fvp(v)
    with context(ARM, obs) as B:
        same_bits(z, B.fvp(v))
        whole = B.act(obs, SEED)
    for a, b, w in zip(first, second, whole):
        same_bits(np.concatenate([a, b]), w)
