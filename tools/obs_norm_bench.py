#!/usr/bin/env python3
"""What the observation filter costs a rollout step, written to profiles/obs_norm.json
(profiles/obs_norm.md explains it; profiles/act_launch.md is the same tool comparing two builds).

  python tools/obs_norm_bench.py [--rounds 40] [--arms disabled,fused] [--host] [--out profiles/obs_norm.json]
  python tools/obs_norm_bench.py --parent-pkg PARENT_TREE/trpo-robot-control_amd      (a build of the parent commit)

Per-step act_record_dev at m rows (from the enqueue to the caller stream's synchronise), fp64 device rows -- with
--host, act_record on host rows, from the call to its return -- on armDOF_0 15-16-16-3 and Humanoid 376-128-64-17,
the arms of --arms alternating inside every round:
  disabled   no filter: the call as it was
  fused      filter enabled: the normalise inside the act kernel, the statistics launch beside it
(The third arm of profiles/obs_norm.md, the normalise as a launch of its own, went with the library's switch for
it.)  Medians with the 10th / 90th percentiles, and the difference fused - disabled as the median (and
percentiles) of the per-round differences.  --arms disabled needs nothing of the filter, so --pkg can point it
at a build from before the filter.  --parent-pkg: behind the arms' own run, four child processes time the same
arms alone -- this tree, the parent's, this tree, the parent's -- stored as solo and parent (two runs each:
their disagreement is the run-to-run spread the two builds are compared within)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NETS = {"armDOF_0": [15, 16, 16, 3], "humanoid": [376, 128, 64, 17]}
ROWS = (1, 64, 1000, 4096)


def stats(ts):
    import numpy as np
    a = np.sort(np.asarray(ts)) * 1e6
    return dict(median_us=float(np.median(a)), p10_us=float(a[int(0.1 * (a.size - 1))]),
                p90_us=float(a[int(np.ceil(0.9 * (a.size - 1)))]))


ARMS = ("disabled", "fused")


def make_ctx(trpo_amd, layers, arm):
    import numpy as np
    from trpo_amd import synth
    ctx = trpo_amd.Context(layers, "lttl", synth.make_theta(layers), synth.make_obs(64, layers[0]),
                           np.ones(layers[-1]), 0.1, device=0)
    if arm != "disabled":
        ctx.obsnorm_enable(5.0, 1e-8)
    return ctx


def step_cost(trpo_amd, layers, m, rounds, arms, host):
    import numpy as np
    from trpo_amd import devmem, synth
    L0, A = layers[0], layers[-1]
    obs = 3.0 + 2.0 * synth.make_obs(m, L0, seed=7)
    if host:
        def call(ctx, step):
            ctx.act_record(obs, seed=1, step=step)
    else:
        st = devmem.Stream(0)
        d_obs = devmem.DeviceArray.from_host(obs, 0)
        d_mean, d_act, d_lp = (devmem.DeviceArray((m, A), np.float64, 0), devmem.DeviceArray((m, A), np.float64, 0),
                               devmem.DeviceArray((m,), np.float64, 0))

        def call(ctx, step):
            ctx.act_record_dev(d_obs, d_mean, d_act, d_lp, seed=1, step=step, stream=st)
            st.synchronize()
    ctxs = {k: make_ctx(trpo_amd, layers, k) for k in arms}
    for k, ctx in ctxs.items():
        ctx.record_begin(m)
        if k != "disabled":                             # a real pair, not the identity: one batch folded
            call(ctx, 0)
            ctx.obsnorm_fold()
            ctx.synchronize()
    times = {k: [] for k in arms}
    for r in range(rounds + 5):
        for k, ctx in ctxs.items():
            t0 = time.perf_counter()
            call(ctx, r)
            dt = time.perf_counter() - t0
            if r >= 5:                                   # five warm-up rounds
                times[k].append(dt)
    for ctx in ctxs.values():
        ctx.close()
    row = {k: stats(v) for k, v in times.items()}
    if "fused" in times and "disabled" in times:
        row["fused_minus_disabled"] = stats(np.asarray(times["fused"]) - np.asarray(times["disabled"]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_norm.json"))
    ap.add_argument("--pkg", default=os.path.join(ROOT, "trpo-robot-control_amd"))
    ap.add_argument("--arms", default=",".join(ARMS), help="comma-separated, of: " + ", ".join(ARMS))
    ap.add_argument("--host", action="store_true", help="act_record on host rows instead of act_record_dev")
    ap.add_argument("--parent-pkg", default=None)
    a = ap.parse_args()
    arms = tuple(a.arms.split(","))
    if not arms or any(k not in ARMS for k in arms):
        ap.error("--arms takes " + ", ".join(ARMS))
    sys.path[:0] = [a.pkg]
    import trpo_amd
    res = dict(rounds=a.rounds, arms=list(arms), rows="host" if a.host else "device", step={})
    for name, layers in NETS.items():
        for m in ROWS:
            res["step"]["%s m=%d" % (name, m)] = row = step_cost(trpo_amd, layers, m, a.rounds, arms, a.host)
            print("%-9s m=%-5d " % (name, m) + "  ".join("%s %.1f" % (k, v["median_us"]) for k, v in row.items()) + "  us",
                  flush=True)
    if a.parent_pkg:
        import subprocess
        import tempfile
        res["solo"], res["parent"] = [], []
        for i in range(4):
            key, pkg = ("solo", a.pkg) if i % 2 == 0 else ("parent", a.parent_pkg)
            with tempfile.TemporaryDirectory() as tmp:
                out = os.path.join(tmp, "r.json")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", pkg, "--arms", a.arms, "--rounds",
                                str(a.rounds), "--out", out] + (["--host"] if a.host else []), check=True,
                               stdout=subprocess.DEVNULL)
                with open(out) as f:
                    res[key].append({k: {arm: v[arm] for arm in arms} for k, v in json.load(f)["step"].items()})
        for k in res["step"]:
            for arm in arms:
                print("%-16s %-8s alone, this tree %s   parent %s  us" % (
                    k, arm, " ".join("%.1f" % r[k][arm]["median_us"] for r in res["solo"]),
                    " ".join("%.1f" % r[k][arm]["median_us"] for r in res["parent"])), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
