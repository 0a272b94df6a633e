"""Trust-region check: the mean KL(old || candidate) of the line-search candidates from the surrogate
kernels' KL variants (trpo_ctx_surrogate_kl) and the KL-capped update (trpo_ctx_update_kl); DESIGN §5.8.

Reference: numpy, direct sums.  Old policy N(rollout Mean, diag(std^2)); candidate k: theta_k = theta +
0.5^(k0 + k) fullstep, mean from synth.policy_mean, ls = theta_k's LogStd:
    kl[k] = sum_i [ls_i - log std_i + std_i^2 / (2 e^{2 ls_i}) - 1/2] + (1 / 2N) sum_s sum_i (dmean)^2 e^{-2 ls_i}

Parity bound for k0 + k <= 5: |dev - ref| <= 1e-10 ref + 1e-14.  Relative term: the device's candidate means
differ from numpy's by a few ulp of |mean|, amplified by 2 |mean| / |dmean|; at these steps |dmean| / |mean| is
at least ~1e-3, i.e. ~1e-12, and two decades are left for the device's tanh through two layers.  Absolute term:
the sigma-only term cancels O(1) quantities over A <= 17 outputs.  Each parity test prints the worst figure
it measured.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import trpo_amd
from trpo_amd import synth

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-10, 1e-14


def kl_ref(L, ac, th_k, obs, mean_old, std, parts=False):
    """KL(old || N(mean(th_k), exp(2 LogStd_k))) averaged over the samples, as direct sums (parts: the
    sigma-only term and the sample term apart)."""
    A = L[-1]
    mu = synth.policy_mean(L, ac, th_k, obs)
    ls = th_k[-A:]
    w = np.exp(-2.0 * ls)
    q = 0.0
    for s in range(obs.shape[0]):
        for i in range(A):
            d = mean_old[s, i] - mu[s, i]
            q += d * d * w[i]
    sig = 0.0
    for i in range(A):
        sig += ls[i] - np.log(std[i]) + std[i] * std[i] / (2.0 * np.exp(2.0 * ls[i])) - 0.5
    smp = q / (2.0 * obs.shape[0]) if obs.shape[0] else 0.0
    return (sig, smp) if parts else sig + smp


@functools.lru_cache(maxsize=None)
def _problem(L, ac, n):
    """test_gpu_surrogate.py::_problem's inputs (std != exp(LogStd): the sigma-only term is live) and the
    numpy KL of the candidates k = 0 .. 5, computed once per shape."""
    L = list(L)
    th = synth.make_theta(L)
    obs = synth.make_obs(n, L[0])
    std = np.linspace(0.7, 1.3, L[-1])
    mean, action, adv = synth.make_rollout(L, ac, th, obs, std)
    fs = 0.05 * np.random.default_rng(5).standard_normal(th.size) * np.abs(th).mean()
    ref = np.array([kl_ref(L, ac, th + 0.5 ** k * fs, obs, mean, std, parts=True) for k in range(6)])
    for a in (th, obs, std, mean, action, adv, fs, ref):
        a.setflags(write=False)
    return th, obs, std, mean, action, adv, fs, ref


def _check(tag, got, ref):
    """ref: the KL, or its (sigma-only, sample) terms per candidate.  With std != exp(LogStd) the sigma-only
    term, which the host forms, dominates the KL, so the device's part is also held to the bound on its own:
    the bound's relative term is about the sample term, its absolute term covers the subtraction."""
    ref = np.asarray(ref)
    if ref.ndim == 2:
        sig, smp = ref[:, 0], ref[:, 1]
        err_s = np.abs((got - sig) - smp)
        print("trust parity %s: sample term worst |dev - ref| = %.3e abs, %.3e of ref (the subtraction of the "
              "sigma-only term included)" % (tag, float(err_s.max()), float(np.max(err_s / smp))))
        assert np.all(err_s <= RTOL * smp + ATOL), (tag, got - sig, smp)
        ref = sig + smp
    err = np.abs(got - ref)
    worst = float(np.max(err / ref))
    print("trust parity %s: worst |dev - ref| / ref = %.3e (bound %.0e ref + %.0e)" % (tag, worst, RTOL, ATOL))
    assert np.all(err <= RTOL * ref + ATOL), (tag, got, ref)


# (layers, activations, environment): the kernel families.  Widths <= 16 take surr_mfma_kernel<1, 1, 1>
# (TRPO_UPDATE_GENERIC=1 alone changes the policy gradient's kernel, not the surrogate's); TRPO_SURR_GENERIC=1
# sends them to the register kernel, and with TRPO_UPDATE_GENERIC=1 as well to the generic one-lane kernel.
FAMILIES = {
    "arm_mfma_1x1": ([15, 16, 16, 3], "lttl", {}),
    "register": ([15, 16, 16, 3], "lttl", {"TRPO_SURR_GENERIC": "1"}),
    "generic_arm": ([15, 16, 16, 3], "lttl", {"TRPO_SURR_GENERIC": "1", "TRPO_UPDATE_GENERIC": "1"}),
    "mfma_1x4": ([15, 64, 64, 3], "lttl", {}),
    "mfma_1x3": ([15, 48, 48, 3], "lttl", {}),
    "mfma_2x4": ([20, 64, 64, 5], "lttl", {}),
    "generic_lds": ([15, 16, 16, 16, 3], "ltttl", {}),
    "generic_ws": ([376, 64, 64, 17], "lttl", {}),
    "one_lane_2x64": ([15, 64, 64, 3], "lttl", {"TRPO_SURR_GENERIC": "1"}),
    "arm_update_generic": ([15, 16, 16, 3], "lttl", {"TRPO_UPDATE_GENERIC": "1"}),
}


def _ctx(L, ac, th, obs, std, mean, action, adv):
    ctx = trpo_amd.Context(L, ac, th, obs, std, 0.1)
    ctx.set_rollout(mean, action, adv)
    return ctx


@pytest.mark.parametrize("n", [1, 17, 65])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_kl_matches_numpy(family, n, monkeypatch):
    L, ac, env = FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    th, obs, std, mean, action, adv, fs, ref = _problem(tuple(L), ac, n)
    with _ctx(L, ac, th, obs, std, mean, action, adv) as ctx:
        s, kl = ctx.surrogate_kl(fs, 0, 6)
        s2, kl2 = ctx.surrogate_kl(fs, 3, 2)
        s_again, kl_again = ctx.surrogate_kl(fs, 0, 6)
        plain, plain2 = ctx.surrogate(fs, 0, 6), ctx.surrogate(fs, 3, 2)
    _check("%s n=%d k0=0" % (family, n), kl, ref)
    _check("%s n=%d k0=3" % (family, n), kl2, ref[3:5])
    np.testing.assert_array_equal(s, plain)                 # the surrogate's own bits
    np.testing.assert_array_equal(s2, plain2)
    np.testing.assert_array_equal(kl, kl_again)             # fixed-order sums: the same bits every call
    np.testing.assert_array_equal(s, s_again)


@pytest.mark.parametrize("family,n", [("mfma_1x4", 1100), ("arm_mfma_1x1", 2100), ("register", 2100),
                                      ("one_lane_2x64", 2100)])
def test_kl_strided_grids(family, n, monkeypatch):
    """nk = 64 caps the grid: the MFMA kernel at 512 / 64 = 8 blocks x 8 waves x 16 samples = 1024 < 1100 (the
    tile loop strides), the one-lane kernels at 2048 / 64 = 32 blocks x 64 = 2048 < 2100 (the pass loop strides)."""
    L, ac, env = FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    th, obs, std, mean, action, adv, fs, ref = _problem(tuple(L), ac, n)
    with _ctx(L, ac, th, obs, std, mean, action, adv) as ctx:
        s, kl = ctx.surrogate_kl(fs, 0, 64)
        plain = ctx.surrogate(fs, 0, 64)
    _check("%s n=%d nk=64" % (family, n), kl[:6], ref)
    np.testing.assert_array_equal(s, plain)
    assert np.all(np.isfinite(kl))


def test_kl_mfma_matches_one_lane(monkeypatch):
    L, ac, n = [15, 64, 64, 3], "lttl", 4099
    th = synth.make_theta(L)
    obs = synth.make_obs(n, L[0])
    std = np.linspace(0.7, 1.3, L[-1])
    mean, action, adv = synth.make_rollout(L, ac, th, obs, std)
    fs = 0.05 * np.random.default_rng(5).standard_normal(th.size) * np.abs(th).mean()
    out = []
    for generic in ("0", "1"):
        monkeypatch.setenv("TRPO_SURR_GENERIC", generic)
        with _ctx(L, ac, th, obs, std, mean, action, adv) as ctx:
            out.append(ctx.surrogate_kl(fs, 0, 6)[1])
    sig = np.array([kl_ref(L, ac, th + 0.5 ** k * fs, obs[:0], mean[:1], std, parts=True)[0] for k in range(6)])
    _check("mfma vs one-lane n=4099", out[0], np.c_[sig, out[1] - sig])


@pytest.mark.parametrize("L", [[15, 16, 16, 3], [15, 64, 64, 3]])
def test_kl_is_zero_at_the_old_policy(L):
    th = synth.make_theta(L, logstd=-0.3)
    obs = synth.make_obs(65, L[0])
    std = np.exp(th[-L[-1]:])
    mean, action, adv = synth.make_rollout(L, "lttl", th, obs, std)
    with _ctx(L, "lttl", th, obs, std, mean, action, adv) as ctx:
        _, kl = ctx.surrogate_kl(np.zeros(th.size), 0, 3)
    assert np.all(np.abs(kl) <= 1e-14), kl


@pytest.mark.parametrize("n", [65, 1000])
@pytest.mark.parametrize("L", [[15, 16, 16, 3], [15, 64, 64, 3]])
def test_kl_curvature_is_the_fisher_matrix(L, n):
    """kl(theta + 2^-k v) 4^k -> v.Fv / 2 with F the matrix the FVP kernels apply.  The numpy KL against the
    oracle's FVP on exactly these inputs deviates by at most 2.0e-2 at k = 0 and 6.4e-5 at k = 8 (the
    deviation halves with each k); the fp32 FVP's 1e-7 is far inside the bounds."""
    damping = 0.1
    th = synth.make_theta(L, logstd=-0.3)
    obs = synth.make_obs(n, L[0])
    std = np.exp(th[-L[-1]:])
    mean, action, adv = synth.make_rollout(L, "lttl", th, obs, std)
    v = 0.05 * np.random.default_rng(5).standard_normal(th.size) * np.abs(th).mean()
    with trpo_amd.Context(L, "lttl", th, obs, std, damping) as ctx:
        ctx.set_rollout(mean, action, adv)
        Fv = ctx.fvp(v) - damping * v
        _, kl = ctx.surrogate_kl(v, 0, 9)
    h = 0.5 * float(v @ Fv)
    dev = np.abs(kl * 4.0 ** np.arange(9) / h - 1.0)
    print("curvature %s n=%d: |kl 4^k / h - 1| = %s" % (L, n, " ".join("%.2e" % d for d in dev)))
    assert dev[0] <= 4e-2 and dev[8] <= 2e-4, dev


# --------------------------------------------------------------------------
# KL-capped update
# --------------------------------------------------------------------------
def _update_problem(name):
    if name == "fix_update_n3150":                    # the update goldens' smallest N
        return cases.update_inputs(cases.case(name)), {}
    if name == "later_backtrack":                     # test_update_later_backtrack_accepted's problem
        L, n, std, kw = [15, 16, 16, 3], 3000, np.ones(3), dict(max_kl=20.0)
        th = synth.make_theta(L)
    else:                                             # test_update_ragged_sample_counts' 2x64 problem
        L, n, std, kw = [15, 64, 64, 3], 65, np.array([0.6065306597126334, 1.0, 1.2840254166877414]), {}
        th = synth.make_theta(L)
        th[-3:] = [-0.5, 0.0, 0.25]
    obs = synth.make_obs(n, L[0])
    mean, action, adv = synth.make_rollout(L, "lttl", th, obs, std)
    return dict(layers=L, acfunc="lttl", theta=th, obs=obs, std=std, mean=mean, action=action, adv=adv,
                damping=0.1), kw


def _predict(ctx, x, r, fullstep, max_bt, accept, cap):
    """First k the three conditions accept, from surrogate_kl's own surr and kl arrays."""
    s, kl = ctx.surrogate_kl(fullstep, 0, max_bt)
    N = x["obs"].shape[0]
    rejected = 0
    for k in range(max_bt):
        actual = r["fval"] - (-s[k] / N)
        ratio = actual / (r["rate"] * 0.5 ** k)
        if ratio > accept and actual > 0:
            if kl[k] <= cap:
                return k, rejected, kl
            rejected += 1
    return -1, rejected, kl


@pytest.mark.parametrize("name", ["fix_update_n3150", "later_backtrack", "ragged_2x64"])
def test_kl_capped_update(name):
    x, kw = _update_problem(name)
    th, A, max_bt, accept = x["theta"], x["layers"][-1], 10, 0.1
    ctx = trpo_amd.Context(x["layers"], x["acfunc"], th, x["obs"], x["std"], x["damping"])
    with ctx:
        ctx.set_rollout(x["mean"], x["action"], x["adv"])
        plain = ctx.update(**kw)
        # no cap: trpo_ctx_update's results bit for bit, and the KL of every evaluated candidate
        r = ctx.update(kl_cap=float("inf"), **kw)
        for key in ("theta", "b", "x", "actual", "expected", "ratio"):
            np.testing.assert_array_equal(r[key], plain[key], err_msg=key)
        for key in ("shs", "lagrange", "gnorm", "fval", "rate", "accepted", "evaluated", "cg_iters"):
            assert r[key] == plain[key], key
        assert r["kl_cap"] == float("inf") and r["kl_rejected"] == 0
        fullstep = r["x"] / r["lagrange"]
        _, kl_eval = ctx.surrogate_kl(fullstep, 0, r["evaluated"])
        np.testing.assert_array_equal(r["kl"], kl_eval)
        ent = 0.5 * np.log(2.0 * np.pi * np.e)
        assert abs(r["entropy_old"] - sum(np.log(s) + ent for s in x["std"])) <= 1e-15
        assert r["accepted"] >= 0
        assert abs(r["entropy_new"] - sum(t + ent for t in r["theta"][-A:])) <= 1e-15
        # a cap just below the accepted candidate's KL: the first fraction the three conditions accept
        cap = 0.9 * r["kl"][r["accepted"]]
        want, rejected, kl_all = _predict(ctx, x, r, fullstep, max_bt, accept, cap)
        c = ctx.update(kl_cap=cap, **kw)
        assert c["accepted"] == want and want > r["accepted"]
        assert c["kl_rejected"] == rejected >= 1
        np.testing.assert_array_equal(c["theta"], th + 0.5 ** want * fullstep)
        np.testing.assert_array_equal(c["kl"], kl_all[:c["evaluated"]])
        assert c["kl"][want] <= cap < c["kl"][r["accepted"]]
        assert abs(c["entropy_new"] - sum(t + ent for t in c["theta"][-A:])) <= 1e-15
        # a cap below every candidate's KL: nothing accepted, the reference's quirk kept
        none = ctx.update(kl_cap=0.5 * kl_all.min(), **kw)
        assert none["accepted"] == -1 and none["evaluated"] == max_bt
        np.testing.assert_array_equal(none["theta"], none["x"])
        assert none["entropy_new"] == none["entropy_old"]
        # the plain entry is what it was
        again = ctx.update(**kw)
        np.testing.assert_array_equal(again["theta"], plain["theta"])
        assert "kl" not in again


def test_kl_capped_update_verbose_lines(capfd):
    x, kw = _update_problem("later_backtrack")
    with trpo_amd.Context(x["layers"], x["acfunc"], x["theta"], x["obs"], x["std"], x["damping"]) as ctx:
        ctx.set_rollout(x["mean"], x["action"], x["adv"])
        libc = C.CDLL(None)                          # the library prints through C stdio
        ctx.update(verbose=True, **kw)
        libc.fflush(None)
        plain = capfd.readouterr().out
        r = ctx.update(verbose=True, kl_cap=float("inf"), **kw)
        libc.fflush(None)
        capped = capfd.readouterr().out
    assert "kl " not in plain
    lines = capped.splitlines()
    assert [l for l in lines if not l.startswith("kl ")] == plain.splitlines()
    kls = [i for i, l in enumerate(lines) if l.startswith("kl ")]
    assert len(kls) == r["evaluated"] == 3 and all(lines[i - 1].startswith("a/e/r ") for i in kls)
    assert [float(lines[i].split()[1]) for i in kls] == [float("%.14f" % k) for k in r["kl"]]


def test_kl_on_the_stall_guard_problem():
    """Random draw 23 (tests/test_gpu_stall_guard.py): the update is re-solved on the fp64 twin, which then
    serves the line search's KL too."""
    from test_gpu_random_shapes import _draw
    layers, acts, n, std = _draw(23)
    th = synth.make_theta(layers, seed=123)
    obs = synth.make_obs(n, layers[0], seed=223)
    mean, action, adv = synth.make_rollout(layers, acts, th, obs, std, seed=523)
    with trpo_amd.Context(layers, acts, th, obs, std, 0.1) as ctx:
        ctx.set_rollout(mean, action, adv)
        plain = ctx.update()
        r = ctx.update(kl_cap=float("inf"))
    assert r["fp64_rerun"] and plain["fp64_rerun"]
    np.testing.assert_array_equal(r["theta"], plain["theta"])
    assert r["accepted"] == plain["accepted"] and r["evaluated"] == plain["evaluated"]
    std = np.asarray(std, dtype=np.float64)
    # the KL at the returned theta' when a step was accepted; this draw's line search accepts none (the
    # reference's neither: theta' is the step direction x), so every evaluated candidate the parity bound
    # covers (k <= 5) is held against numpy at theta + 0.5^k fullstep instead
    fullstep = r["x"] / r["lagrange"]
    ks = [r["accepted"]] if r["accepted"] >= 0 else list(range(min(r["evaluated"], 6)))
    assert ks
    for k in ks:
        th_k = r["theta"] if r["accepted"] >= 0 else th + 0.5 ** k * fullstep
        _check("stall guard k=%d" % k, r["kl"][k:k + 1], [kl_ref(layers, acts, th_k, obs, mean, std, parts=True)])


@pytest.mark.parametrize("L", [[15, 16, 16, 3], [15, 64, 64, 3]])
def test_kl_sharded(L):
    """Two contexts of one process over a host group, shards of 40 and 25 samples: one all-reduce of the
    2 nk sums, identical bits on both ranks."""
    from test_gpu_shard import run_ranks
    th, obs, std, mean, action, adv, fs, ref = _problem(tuple(L), "lttl", 65)
    # the update runs on a rollout drawn with std = 1 = exp(LogStd), where the line search accepts the full step
    one_std = np.ones(L[-1])
    mean1, action1, adv1 = synth.make_rollout(L, "lttl", th, obs, one_std)
    with _ctx(L, "lttl", th, obs, std, mean, action, adv) as one:
        _, kl1 = one.surrogate_kl(fs, 0, 6)
        one.set_std(one_std)
        one.set_rollout(mean1, action1, adv1)
        u1 = one.update(kl_cap=float("inf"))
    assert u1["accepted"] >= 0
    cap = 0.9 * u1["kl"][u1["accepted"]]
    bounds = [(0, 40), (40, 65)]
    ctxs = [trpo_amd.Context(L, "lttl", th, obs[lo:hi], std, 0.1) for lo, hi in bounds]
    for ctx, (lo, hi) in zip(ctxs, bounds):
        ctx.set_rollout(mean[lo:hi], action[lo:hi], adv[lo:hi])

    def rank(ctx, r):
        lo, hi = bounds[r]
        out = [ctx.surrogate_kl(fs, 0, 6), ctx.surrogate(fs, 0, 6)]
        ctx.set_std(one_std)
        ctx.set_rollout(mean1[lo:hi], action1[lo:hi], adv1[lo:hi])
        return out + [ctx.update(kl_cap=float("inf")), ctx.update(kl_cap=cap)]

    try:
        res = run_ranks(ctxs, rank)
    finally:
        for ctx in ctxs:
            ctx.close()
    (sa, kla), pa, fa, ua = res[0]
    (sb, klb), pb, fb, ub = res[1]
    np.testing.assert_array_equal(kla, klb)
    np.testing.assert_array_equal(sa, sb)
    np.testing.assert_array_equal(sa, pa)
    assert np.all(np.abs(kla - kl1) <= 1e-13 * kl1 + 1e-14), (kla, kl1)
    _check("sharded %s" % L, kla, ref)
    np.testing.assert_array_equal(fa["kl"], fb["kl"])
    assert fa["accepted"] == fb["accepted"] == u1["accepted"]
    assert np.all(np.abs(fa["kl"] - u1["kl"]) <= 1e-4 * u1["kl"])     # the sharded solve's step: the update's 1e-4
    assert ua["accepted"] == ub["accepted"] and ua["accepted"] > u1["accepted"]
    np.testing.assert_array_equal(ua["kl"], ub["kl"])
    np.testing.assert_array_equal(ua["theta"], ub["theta"])
    assert ua["kl_rejected"] == ub["kl_rejected"] >= 1


def test_refusals():
    L = [15, 16, 16, 3]
    th, obs, std, mean, action, adv, fs, _ = _problem(tuple(L), "lttl", 17)
    lib = trpo_amd.lib()
    with trpo_amd.Context(L, "lttl", th, obs, std, 0.1) as ctx:
        with pytest.raises(trpo_amd.TRPOError):            # no rollout
            ctx.surrogate_kl(fs, 0, 1)
        with pytest.raises(trpo_amd.TRPOError):
            ctx.update(kl_cap=0.02)
        ctx.set_rollout(mean, action, adv)
        for cap in (0.0, -0.01, float("nan")):
            with pytest.raises(trpo_amd.TRPOError):
                ctx.update(kl_cap=cap)
        f = np.ascontiguousarray(fs)
        assert lib.trpo_ctx_surrogate_kl(ctx._h, f.ctypes.data, 0, 1, None, None) == -1     # both outputs NULL
        out = np.zeros(2)
        assert lib.trpo_ctx_surrogate_kl(ctx._h, f.ctypes.data, 0, 2, None, out.ctypes.data) == 0
        np.testing.assert_array_equal(out, ctx.surrogate_kl(fs, 0, 2)[1])
        assert lib.trpo_ctx_surrogate_kl(ctx._h, f.ctypes.data, 0, 2, out.ctypes.data, None) == 0
        np.testing.assert_array_equal(out, ctx.surrogate(fs, 0, 2))
        # trust may be NULL
        th_out, info = np.zeros(th.size), trpo_amd.UpdateInfo()
        assert lib.trpo_ctx_update_kl(ctx._h, 10, 1e-10, 0.01, 10, 0.1, 0.02, th_out.ctypes.data, None, None,
                                      C.byref(info), None, 0) >= 0
