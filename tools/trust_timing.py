"""What the trust-region check costs, on one MI355X, at armDOF_0 [15,16,16,3] and [15,64,64,3], N = 50 000
(DESIGN §5.8 / §7).  Host wall time of synchronous calls on ONE library and ONE context per shape, the two
sides of each pair alternating; medians over the repetitions after a warm-up:
  update      trpo_ctx_update_kl(kl_cap = INFINITY)  against  trpo_ctx_update
  surrogate   trpo_ctx_surrogate_kl                   against  trpo_ctx_surrogate, nk = 1 and nk = 10
With --parent-lib PATH (a libtrpo_mi355x.so built from the parent commit) also trpo_ctx_update of this library
against the parent's, and the parent against itself (two contexts of the parent library: its own spread).
With --launches the kernel launches of one update, with and without the cap, counted from rocprofv3 kernel
traces of child processes (the difference of a 14-update and a 4-update run, over 10).
Prints one JSON line (profiles/trust_region.json).
    python tools/trust_timing.py [--reps R] [--parent-lib PATH] [--launches]"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "trpo-robot-control_amd")]
import numpy as np  # noqa: E402
import trpo_amd  # noqa: E402
from trpo_amd import synth  # noqa: E402

SHAPES = ([15, 16, 16, 3], [15, 64, 64, 3])
N = 50000


def problem(L, n=N):
    th, obs, std = synth.make_theta(L), synth.make_obs(n, L[0]), np.ones(L[-1])
    mean, action, adv = synth.make_rollout(L, "lttl", th, obs, std)
    return th, obs, std, mean, action, adv


class RawCtx:
    """trpo_ctx_update through the C ABI of any build of the library (the parent's has no KL entries)."""

    def __init__(self, lib, L, th, obs, std, mean, action, adv):
        self.lib, self.P = lib, th.size
        lib.trpo_ctx_create.restype = C.c_void_p
        lib.trpo_ctx_create.argtypes = [C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p, C.c_double, C.c_int]
        lib.trpo_ctx_destroy.argtypes = [C.c_void_p]
        lib.trpo_ctx_set_rollout.argtypes = [C.c_void_p] * 4
        lib.trpo_ctx_update.restype = C.c_double
        lib.trpo_ctx_update.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_int, C.c_double,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        ls = (C.c_size_t * len(L))(*L)
        self.h = lib.trpo_ctx_create(len(L), ls, b"lttl", th.ctypes.data, obs.ctypes.data, obs.shape[0],
                                     std.ctypes.data, 0.1, 0)
        assert self.h, "trpo_ctx_create failed"
        assert lib.trpo_ctx_set_rollout(self.h, mean.ctypes.data, action.ctypes.data, adv.ctypes.data) == 0
        self.th = np.zeros(self.P)

    def update(self):
        t = self.lib.trpo_ctx_update(self.h, 10, 1e-10, 0.01, 10, 0.1, self.th.ctypes.data, None, None, None, 0)
        assert t >= 0, t
        return self.th

    def close(self):
        self.lib.trpo_ctx_destroy(self.h)


def pairs(fa, fb, reps, warmup=5):
    """Alternate fa and fb; microseconds: the two medians and the median of the per-pair differences b - a."""
    for _ in range(warmup):
        fa(), fb()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fa()
        t1 = time.perf_counter()
        fb()
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
    ta, tb = np.asarray(ta) * 1e6, np.asarray(tb) * 1e6
    d = np.sort(tb - ta)
    return dict(a_med=round(float(np.median(ta)), 2), b_med=round(float(np.median(tb)), 2),
                diff_med=round(float(np.median(d)), 2), diff_p10=round(float(d[len(d) // 10]), 2),
                diff_p90=round(float(d[len(d) * 9 // 10]), 2),
                b_over_a=round(float(np.median(tb) / np.median(ta)), 4))


def time_shape(L, reps, parent):
    th, obs, std, mean, action, adv = problem(L)
    row = dict(layers=L, n=N)
    with trpo_amd.Context(L, "lttl", th, obs, std, 0.1, device=0) as ctx:
        ctx.set_rollout(mean, action, adv)
        r = ctx.update(kl_cap=float("inf"))
        fs = r["x"] / r["lagrange"]
        row["kl_full_step"], row["accepted"] = float(r["kl"][0]), int(r["accepted"])
        row["update"] = dict(a="trpo_ctx_update", b="trpo_ctx_update_kl(INFINITY)",
                             **pairs(lambda: ctx.update(), lambda: ctx.update(kl_cap=float("inf")), reps))
        for nk in (1, 10):
            row["surrogate_nk%d" % nk] = dict(a="trpo_ctx_surrogate", b="trpo_ctx_surrogate_kl",
                                              **pairs(lambda: ctx.surrogate(fs, 0, nk),
                                                      lambda: ctx.surrogate_kl(fs, 0, nk), reps))
    if parent is not None:
        args = (L, th, obs, std, mean, action, adv)
        here = C.CDLL(trpo_amd.LIB_PATH)
        new, old, old2 = RawCtx(here, *args), RawCtx(parent, *args), RawCtx(parent, *args)
        same = bool(np.array_equal(new.update().copy(), old.update().copy()))
        row["plain_update_vs_parent"] = dict(a="parent trpo_ctx_update", b="this trpo_ctx_update", same_bits=same,
                                             **pairs(old.update, new.update, reps))
        row["parent_vs_parent"] = dict(a="parent trpo_ctx_update", b="parent trpo_ctx_update (second context)",
                                       **pairs(old.update, old2.update, reps))
        for c in (new, old, old2):
            c.close()
    return row


def child(L, mode, updates):
    th, obs, std, mean, action, adv = problem(L)
    with trpo_amd.Context(L, "lttl", th, obs, std, 0.1, device=0) as ctx:
        ctx.set_rollout(mean, action, adv)
        for _ in range(updates):
            ctx.update(kl_cap=float("inf")) if mode == "kl" else ctx.update()


def traced_kernels(L, mode, updates):
    """Kernel names of one traced child run (rocprofv3 --kernel-trace), as a list."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child", mode, str(updates), ",".join(map(str, L))]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240)
        names = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                names += [r["Kernel_Name"] for r in csv.DictReader(f)]         # rocprofv3's column
    assert names, "no kernel trace written"
    return names


def launches(L):
    out = {}
    for mode in ("plain", "kl"):
        few, many = traced_kernels(L, mode, 4), traced_kernels(L, mode, 14)
        per = {}
        for name in set(many):
            d = many.count(name) - few.count(name)
            if d:
                per[name.split("(")[0]] = per.get(name.split("(")[0], 0) + d / 10.0
        out[mode] = dict(per_update=(len(many) - len(few)) / 10.0, kernels=dict(sorted(per.items())))
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child([int(x) for x in sys.argv[4].split(",")], sys.argv[2], int(sys.argv[3]))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--parent-lib")
    ap.add_argument("--launches", action="store_true")
    a = ap.parse_args()
    trpo_amd.lib()
    parent = C.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    out = dict(tool="trust_timing", unit="us", reps=a.reps, warmup=5, shapes=[])
    # the traced children first, while this process has not touched the GPU; tracing and timing never overlap
    counts = [launches(L) if a.launches else None for L in SHAPES]
    for L, cnt in zip(SHAPES, counts):
        row = time_shape(L, a.reps, parent)
        if cnt is not None:
            row["launches_per_update"] = cnt
        out["shapes"].append(row)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
