"""Wall time of the ragged advantage stage (Baseline.advantage_ragged), two questions:
  equal   what the offsets cost: Baseline.advantage at 20 x 150 against Baseline.advantage_ragged at
          [150] * 20, horizon 150, no truncation -- the same work and the same bits.  The arms alternate in
          this process: the two Python wrappers (fixed, ragged) and the two C entry points called directly
          with prepared pointers (fixed_c, ragged_c), which leaves the wrappers' numpy work out.
          With --parent-lib LIB (the library of the commit before the ragged stage) the fixed
          arm is also timed on that build: child processes, the two builds in alternating rounds.
  ragged  a batch of 20 episodes of 30 .. 150 steps, every second one truncated, from (observ, reward, mean,
          action, x) to a context ready for update():
            host    the caller's work without the stage: a numpy forward for the bootstrap values, numpy
                    recurrences over the padded batch, Baseline.set_data_ragged + evaluate(want_predict=True)
                    for V, the standardisation, Context.set_rollout;
            device  Baseline.advantage_ragged + Context.set_rollout_from.
Prints one JSON line (microseconds: median, p10, p90 over the repetitions after 5 warm-ups).
    python tools/advantage_ragged_timing.py [reps] [--parent-lib LIB]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "trpo-robot-control_amd")]
import numpy as np  # noqa: E402
import trpo_amd  # noqa: E402
from trpo_amd import synth  # noqa: E402

BASE, POLICY, GAMMA, LAM, WARMUP = [16, 16, 16, 1], [15, 16, 16, 3], 0.995, 0.98, 5


def batch(lens, seed=7):
    rng = np.random.default_rng(seed)
    n, O = int(np.sum(lens)), BASE[0] - 1
    reward = -np.abs(rng.normal(1.0, 0.7, n))
    observ = rng.normal(0.0, 1.0, (n, O))
    x = 0.3 * rng.normal(0.0, 1.0, synth.num_params(BASE) - 1)
    boot_observ = rng.normal(0.0, 1.0, (len(lens), O))
    return x, observ, reward, boot_observ


def stats(t):
    t = np.sort(np.asarray(t)) * 1e6
    return dict(med=round(float(t[len(t) // 2]), 1), p10=round(float(t[len(t) // 10]), 1),
                p90=round(float(t[len(t) * 9 // 10]), 1))


def alternate(paths, reps):
    """paths: (name, callable) pairs; they alternate, so all see the same machine."""
    res, t = {}, {name: [] for name, _ in paths}
    for _ in range(WARMUP):
        for _, fn in paths:
            fn()
    for _ in range(reps):
        for name, fn in paths:
            t0 = time.perf_counter()
            res[name] = fn()
            t[name].append(time.perf_counter() - t0)
    return res, {name: stats(v) for name, v in t.items()}


def forward(x, rows):
    y, at = rows, 0
    for i in range(len(BASE) - 1):
        a, b = BASE[i], BASE[i + 1]
        z = y @ x[at:at + a * b].reshape(a, b) + x[at + a * b:at + a * b + b]
        at += a * b + b
        y = np.tanh(z) if "lttl"[i + 1] == "t" else z
    return y[:, 0]


def host_path(bl, ctx, x, observ, reward, boot_observ, boot, lens, horizon, mean, action):
    num_ep, T = len(lens), int(lens.max())
    live = np.arange(T)[None, :] < lens[:, None]
    vb = np.where(boot != 0, forward(x, np.column_stack([boot_observ, lens / float(horizon)])), 0.0)
    r = np.zeros((num_ep, T))
    r[live] = reward
    ret = np.empty_like(r)
    acc = np.zeros(num_ep)
    for t in range(T - 1, -1, -1):                     # an episode's walk starts at its own last step
        acc = np.where(t == lens - 1, vb, acc)
        acc = r[:, t] + GAMMA * acc
        ret[:, t] = acc
    ret = ret[live]
    bl.set_data_ragged(observ, ret, lens, horizon)
    V = np.zeros((num_ep, T))
    V[live] = bl.evaluate(x, want_predict=True)[2]
    A = np.empty_like(r)
    acc, vn = np.zeros(num_ep), np.zeros(num_ep)
    for t in range(T - 1, -1, -1):
        last = t == lens - 1
        vn, acc = np.where(last, vb, vn), np.where(last, 0.0, acc)
        acc = r[:, t] + GAMMA * vn - V[:, t] + GAMMA * LAM * acc
        A[:, t] = acc
        vn = V[:, t]
    A = A[live]
    adv = (A - A.mean()) / A.std()
    ctx.set_rollout(mean, action, adv)
    return adv


def device_path(bl, ctx, x, observ, reward, boot_observ, boot, lens, horizon, mean, action):
    adv, _, _ = bl.advantage_ragged(x, observ, reward, lens, horizon, GAMMA, LAM, boot_observ=boot_observ, boot=boot)
    ctx.set_rollout_from(bl, mean, action)
    return adv


def fixed_arm(lib, reps):
    """trpo_baseline_advantage at 20 x 150 alone, what Baseline.advantage does, on the library file `lib`
    (bound here by hand: an older build lacks the entry points trpo_amd.lib() binds)."""
    import ctypes as C
    L = C.CDLL(lib)
    dp, sz = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS"), C.c_size_t
    L.trpo_baseline_create.restype = C.c_void_p
    L.trpo_baseline_create.argtypes = [sz, C.POINTER(sz), C.c_char_p, C.c_int]
    L.trpo_baseline_destroy.argtypes = [C.c_void_p]
    L.trpo_baseline_advantage.restype = C.c_double
    L.trpo_baseline_advantage.argtypes = [C.c_void_p, dp, dp, dp, sz, sz, C.c_double, C.c_double, dp, dp,
                                          C.POINTER(trpo_amd.AdvInfo)]
    x, observ, reward, _ = batch([150] * 20)
    h = L.trpo_baseline_create(len(BASE), (sz * len(BASE))(*BASE), b"lttl", 0)
    assert h, "trpo_baseline_create failed"

    def call():
        adv, ret, info = np.zeros(3000), np.zeros(3000), trpo_amd.AdvInfo()
        assert L.trpo_baseline_advantage(h, x, observ, reward, 20, 150, GAMMA, LAM, adv, ret, C.byref(info)) >= 0
        return adv
    _, t = alternate([("fixed", call)], reps)
    L.trpo_baseline_destroy(h)
    return t["fixed"]


def child(lib, reps):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), str(reps), "--fixed-arm", lib], check=True,
                         capture_output=True, text=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args and args[0].isdigit() else 50
    if "--fixed-arm" in args:
        print(json.dumps(fixed_arm(args[args.index("--fixed-arm") + 1], reps)), flush=True)
        return
    out = dict(tool="advantage_ragged_timing", unit="us", reps=reps, warmup=WARMUP)
    # equal lengths: the fixed stage against the ragged one, same work
    lens = np.full(20, 150, np.uintp)
    x, observ, reward, _ = batch(lens)
    with trpo_amd.Baseline(BASE, "lttl", device=0) as bf, trpo_amd.Baseline(BASE, "lttl", device=0) as br:
        # ... through the Python wrappers, and the two C entry points alone (same arguments every call,
        # pointers taken once: the wrappers' own numpy work is not in these two)
        import ctypes as C
        L, info = trpo_amd.lib(), trpo_amd.AdvInfo()
        adv, ret = np.zeros(3000), np.zeros(3000)
        pa, pr, pl, pi = adv.ctypes.data, ret.ctypes.data, lens.ctypes.data, C.byref(info)
        res, t = alternate([("fixed", lambda: bf.advantage(x, observ, reward, 20, 150, GAMMA, LAM)),
                            ("ragged", lambda: br.advantage_ragged(x, observ, reward, lens, 150, GAMMA, LAM)),
                            ("fixed_c", lambda: L.trpo_baseline_advantage(bf._h, x, observ, reward, 20, 150, GAMMA,
                                                                          LAM, pa, pr, pi)),
                            ("ragged_c", lambda: L.trpo_baseline_advantage_ragged(br._h, x, observ, reward, 20, pl,
                                                                                  150, None, None, GAMMA, LAM, pa,
                                                                                  pr, pi))], reps)
    out["equal"] = dict(num_ep=20, ep_len=150, fixed=t["fixed"], ragged=t["ragged"], fixed_c=t["fixed_c"],
                        ragged_c=t["ragged_c"],
                        same_bits=bool(np.array_equal(res["fixed"][0], res["ragged"][0]) and
                                       np.array_equal(res["fixed"][1], res["ragged"][1])))
    if "--parent-lib" in args:
        parent, this = os.path.abspath(args[args.index("--parent-lib") + 1]), trpo_amd.LIB_PATH
        rounds = [dict(parent_fixed=child(parent, reps), this_fixed=child(this, reps)) for _ in range(3)]
        out["equal"]["across_builds"] = rounds
    # a ragged batch, half of it truncated: the device path against the caller's host path
    rng = np.random.default_rng(3)
    lens = rng.integers(30, 151, 20).astype(np.uintp)
    boot = (np.arange(20) % 2 == 0).astype(np.uint8)
    horizon, n = 150, int(lens.sum())
    x, observ, reward, boot_observ = batch(lens)
    th, obs, std = synth.make_theta(POLICY), synth.make_obs(n, POLICY[0]), np.ones(POLICY[-1])
    mean, action, _ = synth.make_rollout(POLICY, "lttl", th, obs, std)
    with trpo_amd.Baseline(BASE, "lttl", device=0) as bl, \
            trpo_amd.Context(POLICY, "lttl", th, obs, std, 0.1, device=0) as ctx:
        a = (bl, ctx, x, observ, reward, boot_observ, boot, lens, horizon, mean, action)
        res, t = alternate([("host", lambda: host_path(*a)), ("device", lambda: device_path(*a))], reps)
    out["ragged"] = dict(num_ep=20, n=n, min_len=int(lens.min()), max_len=int(lens.max()), truncated=int(boot.sum()),
                         host=t["host"], device=t["device"],
                         adv_max_diff=float(np.abs(res["host"] - res["device"]).max()),
                         host_over_device=round(t["host"]["med"] / t["device"]["med"], 2))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
