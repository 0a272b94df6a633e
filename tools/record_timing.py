#!/usr/bin/env python3
"""What the rollout record costs and saves on one MI355X.

Per shape, at NumEp x EpLen samples:
  * the post-rollout stage, from the last environment step's results to the end of the update, host clock around
    calls that each end in a device synchronise:
      current   set_obs + batched act(keep=1) + advantage + set_rollout_acted + update      
      recorded  record_commit + advantage_from + set_rollout_acted + update
    The two are timed alternately, rep by rep; the recording of the next rep (record_begin + EpLen act_record
    calls) happens outside the timed window, as the rollout does.
  * the per-step cost: act_record against act at m = NumEp rows, alternately, the price paid EpLen times.
  * the device memory an open recording holds (hipMemGetInfo before and after record_begin).
Medians with the range over the timed reps; the warm-up reps are stated and discarded.  Writes
<out>/rollout_record.json and .md.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "trpo-robot-control_amd"))
import trpo_amd                                                                     # noqa: E402
from trpo_amd import synth                                                          # noqa: E402

SHAPES = {
    "armDOF_0": dict(layers=[15, 16, 16, 3], ac="lttl", form=None, base=[16, 16, 16, 1]),
    "Humanoid": dict(layers=[376, 128, 64, 17], ac="lttl", form="wide", base=[377, 64, 64, 1]),
}
SEED = 20261021


def stats(ts):
    a = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), reps=int(a.size))


def free_bytes():
    hip = C.CDLL(trpo_amd.runtime_path())
    free, total = C.c_size_t(0), C.c_size_t(0)
    if hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return free.value


def measure(name, num_ep, ep_len, warmup, reps, step_reps):
    s = SHAPES[name]
    layers, base = s["layers"], s["base"]
    L0, A, n = layers[0], layers[-1], num_ep * ep_len
    rng = np.random.default_rng(7)
    theta = synth.make_theta(layers) + 0.05 * rng.normal(size=synth.num_params(layers))
    theta[-A:] = rng.uniform(-1.0, 0.0, A)
    observ = 0.5 * rng.normal(size=(n, L0))
    ep = observ.reshape(num_ep, ep_len, L0)
    steps = [np.ascontiguousarray(ep[:, t]) for t in range(ep_len)]
    reward = -np.abs(rng.normal(1.0, 0.7, n))
    x = 0.3 * rng.normal(size=synth.num_params(base) - 1) / np.sqrt(base[0] / 16.0)
    std = np.exp(theta[-A:])
    out = dict(shape=layers, form=s["form"] or "default", baseline=base, num_ep=num_ep, ep_len=ep_len, n=n,
               warmup=warmup, obs_megabytes=n * L0 * 8 / 1e6)
    with trpo_amd.Context(layers, s["ac"], theta, observ[:64], std, 0.1, form=s["form"]) as rec, \
            trpo_amd.Context(layers, s["ac"], theta, observ[:64], std, 0.1, form=s["form"]) as cur, \
            trpo_amd.Baseline(base, "lttl") as bl_r, trpo_amd.Baseline(base, "lttl") as bl_c:

        def record():
            rec.record_begin(n)
            for t in range(ep_len):
                rec.act_record(steps[t], SEED, t, row0=t, row_stride=ep_len)

        def stage_recorded():
            t0 = time.perf_counter()
            rec.record_commit()
            bl_r.advantage_from(rec, x, reward, num_ep, ep_len)
            rec.set_rollout_acted(baseline=bl_r)
            r = rec.update()
            return time.perf_counter() - t0, r

        def stage_current():
            t0 = time.perf_counter()
            cur.set_obs(observ)
            cur.act(observ, SEED, 0, keep=True)
            bl_c.advantage(x, observ, reward, num_ep, ep_len)
            cur.set_rollout_acted(baseline=bl_c)
            r = cur.update()
            return time.perf_counter() - t0, r

        f0 = free_bytes()
        rec.record_begin(n)
        out["record_device_bytes"] = f0 - free_bytes()
        out["record_device_bytes_by_shape"] = n * (L0 + 2 * A) * 8
        tr, tc = [], []
        for i in range(warmup + reps):
            record()
            a, ra = stage_recorded()
            b, rb = stage_current()
            if i >= warmup:
                tr.append(a)
                tc.append(b)
        out["stage_recorded"], out["stage_current"] = stats(tr), stats(tc)
        out["update_accepted"] = [int(ra["accepted"]), int(rb["accepted"])]
        # the per-step price: one step of num_ep rows, with and without the record
        rec.record_begin(n)
        ta, tb = [], []
        for i in range(warmup + step_reps):
            t = i % ep_len
            t0 = time.perf_counter()
            cur.act(steps[t], SEED, t, row0=t, row_stride=ep_len)
            t1 = time.perf_counter()
            rec.act_record(steps[t], SEED, t, row0=t, row_stride=ep_len)
            t2 = time.perf_counter()
            if i >= warmup:
                ta.append(t1 - t0)
                tb.append(t2 - t1)
        out["step_act"], out["step_act_record"] = stats(ta), stats(tb)
    d_stage = out["stage_current"]["median_ms"] - out["stage_recorded"]["median_ms"]
    d_step = out["step_act_record"]["median_ms"] - out["step_act"]["median_ms"]
    out["stage_saving_ms"] = d_stage
    out["steps_extra_ms"] = ep_len * d_step
    out["net_saving_ms"] = d_stage - ep_len * d_step
    return out


def fmt(s):
    return "%.3f (%.3f .. %.3f)" % (s["median_ms"], s["min_ms"], s["max_ms"])


def markdown(results, args):
    lines = ["# Rollout record: the post-rollout stage and the per-step price", "",
             "`tools/record_timing.py --num-ep %d --ep-len %d --warmup %d --reps %d --step-reps %d` on one MI355X; host "
             "clock around synchronous calls, the two variants alternating rep by rep; median (min .. max) in ms over "
             "the timed reps, %d warm-up reps discarded." % (args.num_ep, args.ep_len, args.warmup, args.reps,
                                                             args.step_reps, args.warmup), "",
             "| shape | n | obs MB | stage, current | stage, recorded | act, m = NumEp | act_record, m = NumEp | "
             "stage saving | EpLen x step extra | net | record HBM |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in results.items():
        lines.append("| %s %s (%s) | %d | %.1f | %s | %s | %s | %s | %.3f | %.3f | %.3f | %.1f MB |" % (
            name, "-".join(map(str, r["shape"])), r["form"], r["n"], r["obs_megabytes"], fmt(r["stage_current"]),
            fmt(r["stage_recorded"]), fmt(r["step_act"]), fmt(r["step_act_record"]), r["stage_saving_ms"],
            r["steps_extra_ms"], r["net_saving_ms"], r["record_device_bytes"] / 1e6))
    lines += ["", "current = set_obs + batched act(keep=1) + advantage + set_rollout_acted + update; recorded = "
              "record_commit + advantage_from + set_rollout_acted + update.  net = stage saving - EpLen x (act_record - act): "
              "positive means the recorded loop is faster end to end.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--num-ep", type=int, default=1000)
    ap.add_argument("--ep-len", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--step-reps", type=int, default=200)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    results = {}
    for name in args.shapes.split(","):
        results[name] = measure(name, args.num_ep, args.ep_len, args.warmup, args.reps, args.step_reps)
        print(json.dumps({name: results[name]}), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "rollout_record.json"), "w") as f:
        json.dump(dict(args={k: v for k, v in vars(args).items() if k != "out"}, results=results), f, indent=1)
    with open(os.path.join(args.out, "rollout_record.md"), "w") as f:
        f.write(markdown(results, args))


if __name__ == "__main__":
    main()
