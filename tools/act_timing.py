"""Host-visible time of one trpo_ctx_act call (mean, action, logp back on the host) in both kernel forms,
next to the caller's host path the call replaces: a numpy fp64 forward pass plus numpy normals, on the CPUs
the process may use and on one core.  Shapes ARM, [11,64,64,3] and [376,64,64,17]; m in 1, 16, 256, 4096,
50000; median (and p10 / p90) of 200 calls after 20 warm-up calls, microseconds.

Every measurement runs in a child process of its own under `timeout`: one (shape, form) per GPU child, one
(shape, thread count) per host child.  The first child that fails ends the run: nothing more is started.
Writes profiles/act_stage.json (or --out PATH).
    python tools/act_timing.py [--out PATH] [--reps N]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "trpo-robot-control_amd")]

SHAPES = [("arm", [15, 16, 16, 3]), ("2x64", [11, 64, 64, 3]), ("wide-in", [376, 64, 64, 17])]
MS = [1, 16, 256, 4096, 50000]
WARMUP = 20
THREAD_VARS = ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")


def stats(t):
    import numpy as np
    t = np.sort(np.asarray(t)) * 1e6
    return dict(med=round(float(t[len(t) // 2]), 1), p10=round(float(t[len(t) // 10]), 1),
                p90=round(float(t[len(t) * 9 // 10]), 1))


def problem(layers, m):
    import numpy as np
    from trpo_amd import synth
    rng = np.random.default_rng(11)
    th = synth.make_theta(layers) + 0.05 * rng.normal(size=synth.num_params(layers))
    th[-layers[-1]:] = rng.uniform(-1.0, 0.5, layers[-1])
    return th, 0.5 * rng.normal(size=(m, layers[0]))


def gpu_child(k, form, reps):
    import numpy as np
    import trpo_amd
    layers = SHAPES[k][1]
    os.environ["TRPO_ACT_FORM"] = form
    th, obs = problem(layers, max(MS))
    out = {}
    with trpo_amd.Context(layers, "lttl", th, obs[:1], np.exp(th[-layers[-1]:]), 0.1, device=0) as ctx:
        for m in MS:
            o = np.ascontiguousarray(obs[:m])
            t = []
            for i in range(WARMUP + reps):
                t0 = time.perf_counter()
                ctx.act(o, 7, i)
                t.append(time.perf_counter() - t0)
            out[str(m)] = stats(t[WARMUP:])
    print(json.dumps(out), flush=True)


def host_child(k, reps):
    """What a trainer without the call does per step: forward pass, normals, action, log-density."""
    import numpy as np
    layers = SHAPES[k][1]
    th, obs = problem(layers, max(MS))
    A, W, pos = layers[-1], [], 0
    for i in range(len(layers) - 1):
        a, b = layers[i], layers[i + 1]
        W.append((th[pos:pos + a * b].reshape(a, b), th[pos + a * b:pos + a * b + b]))
        pos += a * b + b
    logstd, rng, out = th[-A:], np.random.default_rng(3), {}
    for m in MS:
        o = np.ascontiguousarray(obs[:m])
        t = []
        for _ in range(WARMUP + reps):
            t0 = time.perf_counter()
            y = o
            for i, (w, b) in enumerate(W):
                y = y @ w + b
                if i + 1 < len(W):
                    y = np.tanh(y)
            z = rng.standard_normal((m, A))
            action = y + np.exp(logstd) * z
            logp = -0.5 * (z * z).sum(axis=1) - logstd.sum() - 0.5 * A * np.log(2.0 * np.pi)
            t.append(time.perf_counter() - t0)
        assert action.shape == (m, A) and logp.shape == (m,)
        out[str(m)] = stats(t[WARMUP:])
    print(json.dumps(out), flush=True)


def run_child(args, limit, env=None):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args,
                       capture_output=True, text=True, env=env)
    if p.returncode != 0:
        return None, "exit %d: %s" % (p.returncode, (p.stderr or p.stdout)[-400:])
    return json.loads(p.stdout.strip().splitlines()[-1]), None


def main():
    argv = sys.argv[1:]
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 200
    if argv[:1] == ["--gpu-child"]:
        return gpu_child(int(argv[1]), argv[2], reps)
    if argv[:1] == ["--host-child"]:
        return host_child(int(argv[1]), reps)
    path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "act_stage.json")
    threads = os.environ.get("OMP_NUM_THREADS", "16")
    out = dict(tool="act_timing", unit="us", reps=reps, warmup=WARMUP, host_threads=int(threads), shapes=[])
    err = None
    for k, (name, layers) in enumerate(SHAPES):
        row = dict(shape=name, layers=layers)
        steps = [("host", ["--host-child", str(k)], {v: threads for v in THREAD_VARS}, 300),
                 ("host_1core", ["--host-child", str(k)], {v: "1" for v in THREAD_VARS}, 300),
                 ("lane", ["--gpu-child", str(k), "lane"], {}, 240),
                 ("neuron", ["--gpu-child", str(k), "neuron"], {}, 240)]
        for key, args, env, limit in steps:
            row[key], err = run_child(args + ["--reps", str(reps)], limit, dict(os.environ, **env))
            if err:
                row[key] = dict(error=err)
                break
        out["shapes"].append(row)
        if err:
            break
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    return 1 if err else 0


if __name__ == "__main__":
    sys.exit(main())
