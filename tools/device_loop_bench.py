#!/usr/bin/env python3
"""Timings of the device-resident loop against the host-array calls it stands beside, written to
profiles/device_loop.json (profiles/device_loop.md explains it).

  python tools/device_loop_bench.py [--rounds 30] [--out profiles/device_loop.json]

Per-step cost at m rows, on armDOF_0 15-16-16-3, 2x64 15-64-64-3 and Humanoid 376-128-64-17: act_record on
host arrays (the call from entry to return) against act_record_dev (from the enqueue to the caller stream's
synchronise), each with the lane and the neuron form forced.  The four arms alternate inside every round; the
table holds medians with the 10th / 90th percentiles.  Post-rollout stage at 1 000 x 50: advantage_from with
host rewards against advantage_from_dev."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "trpo-robot-control_amd")]
import numpy as np  # noqa: E402

import trpo_amd  # noqa: E402
from trpo_amd import devmem, synth  # noqa: E402

NETS = {"armDOF_0": [15, 16, 16, 3], "2x64": [15, 64, 64, 3], "humanoid": [376, 128, 64, 17]}
ROWS = (1, 16, 256, 1000, 4096, 50000)


def make_ctx(layers, form):
    os.environ["TRPO_ACT_FORM"] = form
    try:
        th = synth.make_theta(layers)
        return trpo_amd.Context(layers, "lttl", th, synth.make_obs(64, layers[0]), np.ones(layers[-1]), 0.1, device=0)
    finally:
        os.environ.pop("TRPO_ACT_FORM", None)


def stats(ts):
    a = np.sort(np.asarray(ts)) * 1e6
    return dict(median_us=float(np.median(a)), p10_us=float(a[int(0.1 * (a.size - 1))]),
                p90_us=float(a[int(np.ceil(0.9 * (a.size - 1)))]))


def step_cost(layers, m, rounds):
    L0, A = layers[0], layers[-1]
    obs = synth.make_obs(m, L0, seed=7)
    st = devmem.Stream(0)
    d_obs = devmem.DeviceArray.from_host(obs, 0)
    d_mean, d_act, d_lp = (devmem.DeviceArray((m, A), np.float64, 0), devmem.DeviceArray((m, A), np.float64, 0),
                           devmem.DeviceArray((m,), np.float64, 0))
    arms, times = {}, {}
    for form in ("lane", "neuron"):
        ctx = make_ctx(layers, form)
        ctx.record_begin(m)
        arms["host_" + form] = (ctx, False)
        arms["dev_" + form] = (ctx, True)
    for k in arms:
        times[k] = []
    for r in range(rounds + 5):
        for k, (ctx, on_dev) in arms.items():
            t0 = time.perf_counter()
            if on_dev:
                ctx.act_record_dev(d_obs, d_mean, d_act, d_lp, seed=1, step=r, stream=st)
                st.synchronize()
            else:
                ctx.act_record(obs, 1, r)
            dt = time.perf_counter() - t0
            if r >= 5:                                   # five warm-up rounds
                times[k].append(dt)
    for ctx in {id(c): c for c, _ in arms.values()}.values():
        ctx.close()
    return {k: stats(v) for k, v in times.items()}


def stage_cost(rounds, num_ep=1000, ep_len=50):
    layers, n = NETS["armDOF_0"], num_ep * ep_len
    O = layers[0]
    base = [O + 1, 16, 16, 1]
    rng = np.random.default_rng(5)
    x = 0.3 * rng.normal(size=synth.num_params(base) - 1)
    reward = -np.abs(rng.normal(1.0, 0.7, n))
    obs = synth.make_obs(n, O, seed=9)
    ctx = trpo_amd.Context(layers, "lttl", synth.make_theta(layers), obs, np.ones(layers[-1]), 0.1, device=0)
    st = devmem.Stream(0)
    d_rew = devmem.DeviceArray.from_host(reward, 0)
    times = {"host_rewards": [], "device_rewards": []}
    with trpo_amd.Baseline(base, "lttl", 0) as bl:
        for r in range(rounds + 3):
            for k in times:
                t0 = time.perf_counter()
                if k == "host_rewards":
                    bl.advantage_from(ctx, x, reward, num_ep, ep_len)
                else:
                    bl.advantage_from_dev(ctx, x, d_rew, num_ep, ep_len, stream=st)
                dt = time.perf_counter() - t0
                if r >= 3:
                    times[k].append(dt)
    ctx.close()
    return {k: stats(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_loop.json"))
    a = ap.parse_args()
    res = dict(rounds=a.rounds, step={}, stage=None)
    for name, layers in NETS.items():
        for m in ROWS:
            res["step"]["%s m=%d" % (name, m)] = row = step_cost(layers, m, a.rounds)
            print("%-9s m=%-6d " % (name, m) + "  ".join("%s %.1f us" % (k, v["median_us"]) for k, v in row.items()),
                  flush=True)
    res["stage"] = stage_cost(a.rounds)
    print("stage 1000x50: " + "  ".join("%s %.1f us" % (k, v["median_us"]) for k, v in res["stage"].items()))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
