#!/usr/bin/env python3
"""Timings of the wide-policy path (Context(form="wide")) through the context API and
trpo_ctx_time only, written to profiles/wide_policy.json (profiles/wide_policy.md explains it).

  python tools/wide_bench.py [--n 50000] [--rounds 5] [--out profiles/wide_policy.json] [--oracle]
  python tools/wide_bench.py --trace-target        # a few FVPs and one solve, for a kernel trace of its own:
      rocprofv3 --kernel-trace --stats -d DIR -- python tools/wide_bench.py --trace-target

Humanoid 376-128-64-17: forward sweep + FVP against FVP on a valid cache, 10-iteration CG, one full update and
its split between the generic fp64 policy gradient / surrogate and the solve, the FVP's algorithmic FLOPs over
its time as a share of the 157.3 TF fp32-MFMA peak, and (--oracle) the oracle's one-core time of the same CG.
The gate: on 180-128-64-17 a default context (the generic kernel) and a wide context, both timed interleaved
in this one process, the 10-iteration CG of each and the ratio."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "trpo-robot-control_amd"), os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402

import trpo_amd  # noqa: E402
from trpo_amd import synth  # noqa: E402

HUMANOID, GATE, ACTS = [376, 128, 64, 17], [180, 128, 64, 17], "lttl"
PEAK_TF = 157.3


def problem(layers, n, seed=1):
    rng = np.random.default_rng(seed)
    th = synth.make_theta(layers, seed=100 + seed)
    obs = 12.0 * synth.make_obs(n, layers[0], seed=200 + seed)
    std = rng.uniform(0.5, 1.6, size=layers[-1])
    P = synth.num_params(layers)
    return dict(layers=layers, n=n, theta=th, obs=obs, std=std, P=P, v=synth.make_v(P, seed=300 + seed),
                b=synth.make_b(P, seed=400 + seed))


def fvp_flops(layers, n):
    """algorithmic FLOPs of one FVP on a valid cache: R-forward 2 products, backward 1, contraction 1 per weight
    (2 FLOP each) per sample; the last layer has no backward product into the observations"""
    w = [layers[i] * layers[i + 1] for i in range(len(layers) - 1)]
    return 2.0 * n * (2 * sum(w) - w[0] + sum(w[1:]) + sum(w))


def ctx_of(p, form):
    c = trpo_amd.Context(p["layers"], ACTS, p["theta"], p["obs"], p["std"], 0.1, form=form)
    c.upload_b(p["b"])
    c.upload_v(p["v"])
    return c


def med(xs):
    return float(np.median(xs))


def humanoid(n, rounds, with_oracle):
    p = problem(HUMANOID, n)
    out = dict(layers=HUMANOID, acts=ACTS, n=n, P=p["P"])
    with ctx_of(p, "wide") as c:
        out["kernel_name"] = c.kernel_name
        cold, warm, cg = [], [], []
        for _ in range(rounds):
            c.set_theta(p["theta"])                       # invalidates the forward cache
            c.upload_v(p["v"])
            c.synchronize()
            t0 = time.perf_counter()
            c.enqueue_fvp()
            c.synchronize()
            cold.append((time.perf_counter() - t0) * 1e3)
            warm.append(c.time_ms(1, 20))
            cg.append(c.time_ms(2, 5, 10, 0.0))
        out["fvp_with_forward_sweep_ms_host_clock"] = med(cold)
        out["fvp_cached_ms"] = med(warm)
        out["cg10_ms"] = med(cg)
        out["fvp_flops"] = fvp_flops(HUMANOID, n)
        out["fvp_tflops"] = out["fvp_flops"] / (out["fvp_cached_ms"] * 1e-3) / 1e12
        out["fvp_share_of_fp32_mfma_peak"] = out["fvp_tflops"] / PEAK_TF
        mean, action, adv = synth.make_rollout(HUMANOID, ACTS, p["theta"], p["obs"], p["std"], seed=501)
        c.set_rollout(mean, action, adv)
        c.update()
        upd = []
        for _ in range(rounds):
            upd.append(c.update()["seconds"] * 1e3)
        out["update_ms"] = med(upd)
        # the solve's share: the CG plus the FVP(x) behind it; the rest is the generic fp64 policy gradient,
        # the surrogates and the host's step arithmetic
        out["update_solve_ms"] = out["cg10_ms"] + out["fvp_cached_ms"]
        out["update_pg_surrogate_ms"] = out["update_ms"] - out["update_solve_ms"]
    if with_oracle:
        import oracle
        t0 = time.perf_counter()
        oracle.cg(HUMANOID, ACTS, p["theta"], p["obs"], p["std"], p["b"], 10, 0.0)
        out["oracle_cg10_one_core_s"] = time.perf_counter() - t0
    return out


def gate(n, rounds):
    p = problem(GATE, n)
    out = dict(layers=GATE, acts=ACTS, n=n, P=p["P"])
    with ctx_of(p, None) as d, ctx_of(p, "wide") as w:
        out["default_kernel"], out["wide_kernel"] = d.kernel_name, w.kernel_name
        td, tw = [], []
        d.time_ms(2, 1, 10, 0.0)
        w.time_ms(2, 1, 10, 0.0)
        for _ in range(rounds):                           # interleaved, one process
            td.append(d.time_ms(2, 1, 10, 0.0))
            tw.append(w.time_ms(2, 5, 10, 0.0))
        xd, xw = d.cg(p["b"], 10, 0.0), w.cg(p["b"], 10, 0.0)
    out["default_cg10_ms"], out["wide_cg10_ms"] = td, tw
    out["default_cg10_ms_median"], out["wide_cg10_ms_median"] = med(td), med(tw)
    out["ratio_default_over_wide"] = med(td) / med(tw)
    out["x_rel_l2_wide_vs_default"] = float(np.linalg.norm(xw - xd) / np.linalg.norm(xd))
    return out


def trace_target(n):
    p = problem(HUMANOID, n)
    with ctx_of(p, "wide") as c:
        for _ in range(4):
            c.enqueue_fvp()
        c.enqueue_cg(10, 0.0)
        c.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_policy.json"))
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--trace-target", action="store_true")
    a = ap.parse_args()
    if a.trace_target:
        trace_target(a.n)
        sys.exit(0)
    res = dict(humanoid=humanoid(a.n, a.rounds, a.oracle), gate=gate(a.n, a.rounds))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    if not res["gate"]["ratio_default_over_wide"] > 1.0:
        sys.exit("the wide path's CG is not faster than the generic kernel's on %s" % GATE)
