#!/usr/bin/env python3
"""What the observation filter costs a device-resident rollout step, written to profiles/obs_norm.json
(profiles/obs_norm.md explains it).

  python tools/obs_norm_bench.py [--rounds 40] [--out profiles/obs_norm.json]
  python tools/obs_norm_bench.py --parent-pkg PARENT_TREE/trpo-robot-control_amd      (a build of the parent commit)

Per-step act_record_dev at m rows (from the enqueue to the caller stream's synchronise), fp64 rows, on armDOF_0
15-16-16-3 and Humanoid 376-128-64-17, three arms that alternate inside every round:
  disabled   no filter: the call as it was
  fused      filter enabled: the normalise inside the act kernel, the statistics launch behind it
  split      filter enabled with TRPO_OBSNORM_SPLIT=1: the normalise as a launch of its own into a scratch array,
             then the plain act kernel, then the same statistics launch -- what a caller could do without the fusion
Medians with the 10th / 90th percentiles, and the differences fused - disabled and split - fused as the median
(and percentiles) of the per-round differences.  --only-disabled times the first arm alone and needs nothing of the
filter, so --pkg can point it at a build of the parent commit.  --parent-pkg does that: behind the three arms it
runs four child processes, each timing the disabled arm alone -- this tree, the parent's, this tree, the parent's --
and stores them as solo_disabled and parent_disabled (two runs each: their disagreement is the run-to-run spread
the two builds are compared within)."""
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


def make_ctx(trpo_amd, layers, arm):
    import numpy as np
    from trpo_amd import synth
    ctx = trpo_amd.Context(layers, "lttl", synth.make_theta(layers), synth.make_obs(64, layers[0]),
                           np.ones(layers[-1]), 0.1, device=0)
    if arm != "disabled":
        if arm == "split":
            os.environ["TRPO_OBSNORM_SPLIT"] = "1"
        try:
            ctx.obsnorm_enable(5.0, 1e-8)
        finally:
            os.environ.pop("TRPO_OBSNORM_SPLIT", None)
    return ctx


def step_cost(trpo_amd, layers, m, rounds, arms):
    import numpy as np
    from trpo_amd import devmem, synth
    L0, A = layers[0], layers[-1]
    obs = 3.0 + 2.0 * synth.make_obs(m, L0, seed=7)
    st = devmem.Stream(0)
    d_obs = devmem.DeviceArray.from_host(obs, 0)
    d_mean, d_act, d_lp = (devmem.DeviceArray((m, A), np.float64, 0), devmem.DeviceArray((m, A), np.float64, 0),
                           devmem.DeviceArray((m,), np.float64, 0))
    ctxs = {k: make_ctx(trpo_amd, layers, k) for k in arms}
    for k, ctx in ctxs.items():
        ctx.record_begin(m)
        if k != "disabled":                             # a real pair, not the identity: one batch folded
            ctx.act_record_dev(d_obs, d_mean, d_act, d_lp, seed=1, step=0, stream=st)
            ctx.obsnorm_fold()
            ctx.synchronize()
    times = {k: [] for k in arms}
    for r in range(rounds + 5):
        for k, ctx in ctxs.items():
            t0 = time.perf_counter()
            ctx.act_record_dev(d_obs, d_mean, d_act, d_lp, seed=1, step=r, stream=st)
            st.synchronize()
            dt = time.perf_counter() - t0
            if r >= 5:                                   # five warm-up rounds
                times[k].append(dt)
    for ctx in ctxs.values():
        ctx.close()
    row = {k: stats(v) for k, v in times.items()}
    if "fused" in times:
        t = {k: np.asarray(v) for k, v in times.items()}
        row["fused_minus_disabled"] = stats(t["fused"] - t["disabled"])
        row["split_minus_fused"] = stats(t["split"] - t["fused"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_norm.json"))
    ap.add_argument("--pkg", default=os.path.join(ROOT, "trpo-robot-control_amd"))
    ap.add_argument("--only-disabled", action="store_true")
    ap.add_argument("--parent-pkg", default=None)
    a = ap.parse_args()
    sys.path[:0] = [a.pkg]
    import trpo_amd
    arms = ("disabled",) if a.only_disabled else ("disabled", "fused", "split")
    res = dict(rounds=a.rounds, arms=list(arms), step={})
    for name, layers in NETS.items():
        for m in ROWS:
            res["step"]["%s m=%d" % (name, m)] = row = step_cost(trpo_amd, layers, m, a.rounds, arms)
            print("%-9s m=%-5d " % (name, m) + "  ".join("%s %.1f" % (k, v["median_us"]) for k, v in row.items()) + "  us",
                  flush=True)
    if a.parent_pkg:
        import subprocess
        import tempfile
        res["solo_disabled"], res["parent_disabled"] = [], []
        for i in range(4):
            key, pkg = ("solo_disabled", a.pkg) if i % 2 == 0 else ("parent_disabled", a.parent_pkg)
            with tempfile.TemporaryDirectory() as tmp:
                out = os.path.join(tmp, "r.json")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", pkg, "--only-disabled", "--rounds",
                                str(a.rounds), "--out", out], check=True, stdout=subprocess.DEVNULL)
                with open(out) as f:
                    res[key].append({k: v["disabled"] for k, v in json.load(f)["step"].items()})
        for k in res["step"]:
            print("%-16s alone, this tree %s   parent %s  us" % (
                k, " ".join("%.1f" % r[k]["median_us"] for r in res["solo_disabled"]),
                " ".join("%.1f" % r[k]["median_us"] for r in res["parent_disabled"])), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
