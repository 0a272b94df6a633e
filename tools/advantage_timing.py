"""Wall time from (observ, reward, mean, action, x) to a context ready for update(), two ways, at the
trainer's batch (20 x 150) and at 334 x 150:
  host    the caller's work on the API without the advantage stage: a numpy recurrence for the returns,
          Baseline.set_data + evaluate(want_predict=True) for V, a numpy recurrence for the advantages,
          their standardisation, Context.set_rollout;
  device  Baseline.advantage + Context.set_rollout_from.
Both end with the returns as the baseline's fit target and the rollout on the device.  Prints one JSON
line (microseconds: median, p10, p90 over the repetitions after a warm-up).
    python tools/advantage_timing.py [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "trpo-robot-control_amd")]
import numpy as np  # noqa: E402
import trpo_amd  # noqa: E402
from trpo_amd import synth  # noqa: E402

BASE, POLICY, GAMMA, LAM = [16, 16, 16, 1], [15, 16, 16, 3], 0.995, 0.98


def host_path(bl, ctx, x, observ, reward, mean, action, num_ep, ep_len):
    r = reward.reshape(num_ep, ep_len)
    ret = np.empty_like(r)
    acc = np.zeros(num_ep)
    for t in range(ep_len - 1, -1, -1):
        acc = r[:, t] + GAMMA * acc
        ret[:, t] = acc
    bl.set_data(observ, ret.ravel(), num_ep, ep_len)
    V = bl.evaluate(x, want_predict=True)[2].reshape(num_ep, ep_len)
    A = np.empty_like(r)
    acc, vn = np.zeros(num_ep), np.zeros(num_ep)
    for t in range(ep_len - 1, -1, -1):
        acc = r[:, t] + GAMMA * vn - V[:, t] + GAMMA * LAM * acc
        A[:, t] = acc
        vn = V[:, t]
    A = A.ravel()
    adv = (A - A.mean()) / A.std()
    ctx.set_rollout(mean, action, adv)
    return adv


def device_path(bl, ctx, x, observ, reward, mean, action, num_ep, ep_len):
    adv, _, _ = bl.advantage(x, observ, reward, num_ep, ep_len, GAMMA, LAM)
    ctx.set_rollout_from(bl, mean, action)
    return adv


def stats(t):
    t = np.sort(np.asarray(t)) * 1e6
    return dict(med=round(float(t[len(t) // 2]), 1), p10=round(float(t[len(t) // 10]), 1),
                p90=round(float(t[len(t) * 9 // 10]), 1))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out = dict(tool="advantage_timing", unit="us", reps=reps, warmup=5, batches=[])
    for num_ep, ep_len in ((20, 150), (334, 150)):
        n = num_ep * ep_len
        rng = np.random.default_rng(7)
        reward = -np.abs(rng.normal(1.0, 0.7, n))
        observ = rng.normal(0.0, 1.0, (n, BASE[0] - 1))
        x = 0.3 * rng.normal(0.0, 1.0, synth.num_params(BASE) - 1)
        th, obs, std = synth.make_theta(POLICY), synth.make_obs(n, POLICY[0]), np.ones(POLICY[-1])
        mean, action, _ = synth.make_rollout(POLICY, "lttl", th, obs, std)
        row = dict(num_ep=num_ep, ep_len=ep_len)
        with trpo_amd.Baseline(BASE, "lttl", device=0) as bl, \
                trpo_amd.Context(POLICY, "lttl", th, obs, std, 0.1, device=0) as ctx:
            args = (bl, ctx, x, observ, reward, mean, action, num_ep, ep_len)
            paths = (("host", host_path), ("device", device_path))
            res, t = {}, dict(host=[], device=[])
            for _ in range(5):
                for _, fn in paths:
                    fn(*args)
            for _ in range(reps):                      # the two paths alternate: both see the same machine
                for name, fn in paths:
                    t0 = time.perf_counter()
                    res[name] = fn(*args)
                    t[name].append(time.perf_counter() - t0)
            for name, _ in paths:
                row[name] = stats(t[name])
            row["adv_max_diff"] = float(np.abs(res["host"] - res["device"]).max())
            row["host_over_device"] = round(row["host"]["med"] / row["device"]["med"], 2)
        out["batches"].append(row)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
