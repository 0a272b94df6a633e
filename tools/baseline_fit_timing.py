"""The value fit of one trainer iteration, two ways, on the trainer's problem ([16,16,16,1] baseline, 20 x 150
samples of trpo_amd.synth-style data, the fit target left by the advantage stage):
  fit_tr  Baseline.fit_tr: the device-resident trust-region step (cg_max_iter 10, max_backtracks 10, eps 0.01,
          damping 1e-3, shift_cap 1.5 eps), one host wait;
  lbfgs   the caller's liblbfgs fit (25 iterations, the reference's own optimiser from oracle/_ref, where that
          is built) on this library's drop-in evaluate, from the same weights on the same data.
The two alternate, so both see the same machine; the medians of the pairs are reported (microseconds), with
the plain loss L = mean (V - y)^2 before, after one and after three successive fit_tr steps, after one uncapped
step at eps = 0.01, 0.1 and 1, and after the liblbfgs fit.  Prints one JSON line.
    [TRPO_LIB=lib.so] python tools/baseline_fit_timing.py [pairs]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "trpo-robot-control_amd")]
import numpy as np  # noqa: E402
import trpo_amd  # noqa: E402
from trpo_amd import synth  # noqa: E402

BASE, AC, NUM_EP, EP_LEN, GAMMA, LAM = [16, 16, 16, 1], "lttl", 20, 150, 0.995, 0.98
EPS, CG_ITERS, CG_TH, DAMPING, BACKTRACKS = 0.01, 10, 1e-10, 1e-3, 10
REF_LBFGS = os.path.join(ROOT, "oracle", "_ref", "libref_lbfgs.so")


def stats(t):
    t = np.sort(np.asarray(t)) * 1e6
    return dict(med=round(float(t[len(t) // 2]), 1), p10=round(float(t[len(t) // 10]), 1),
                p90=round(float(t[len(t) * 9 // 10]), 1))


def loss(bl, x, target):
    return float(((bl.evaluate(x, want_predict=True)[2] - target) ** 2).mean())


def main():
    pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    n = NUM_EP * EP_LEN
    rng = np.random.default_rng(7)
    reward = -np.abs(rng.normal(1.0, 0.7, n))
    observ = rng.normal(0.0, 1.0, (n, BASE[0] - 1))
    npar = synth.num_params(BASE) - 1
    x = 0.3 * rng.normal(0.0, 1.0, npar)
    out = dict(tool="baseline_fit_timing", unit="us", pairs=pairs, warmup=5, library=os.path.basename(trpo_amd.LIB_PATH),
               settings=dict(eps=EPS, cg_max_iter=CG_ITERS, cg_residual_th=CG_TH, damping=DAMPING,
                             max_backtracks=BACKTRACKS, shift_cap=1.5 * EPS))
    ref = C.CDLL(REF_LBFGS) if os.path.exists(REF_LBFGS) else None
    with trpo_amd.Baseline(BASE, AC, device=0) as bl:
        _, ret, _ = bl.advantage(x, observ, reward, NUM_EP, EP_LEN, GAMMA, LAM)

        def fit_tr(x0):
            return bl.fit_tr(x0, EPS, CG_ITERS, CG_TH, DAMPING, BACKTRACKS, 1.5 * EPS)

        if ref is not None:
            ref.ref_lbfgs_fit.restype = C.c_int
            ref.ref_lbfgs_fit.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p,
                                          C.c_void_p, C.c_int]
            param = trpo_amd.make_baseline_param(BASE, AC, observ, ret, NUM_EP, EP_LEN)
            proc = C.cast(trpo_amd.lib().evaluate, C.c_void_p)
            x_pad = np.zeros(param.PaddedParams)
            x_pad[:npar] = x

            def lbfgs():
                xf, fx = np.array(x_pad), C.c_double(0.0)
                rc = ref.ref_lbfgs_fit(xf.size, xf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(fx), proc,
                                       C.byref(param), 25)
                return rc, xf[:npar]

        t_tr, t_c, t_lb = [], [], []
        for r in range(5 + pairs):
            t0 = time.perf_counter()
            x1, _, info = fit_tr(x)
            t1 = time.perf_counter()
            if ref is not None:
                rc, x_lb = lbfgs()
            t2 = time.perf_counter()
            if r >= 5:
                t_tr.append(t1 - t0)
                t_c.append(info.seconds)
                t_lb.append(t2 - t1)
        out["fit_tr"] = stats(t_tr)                      # around the Python call
        out["fit_tr_c_call"] = stats(t_c)                # what trpo_baseline_fit_tr itself returns
        out["fit_tr_info"] = dict(cg_iters=int(info.cg_iters), accepted=int(info.accepted), alpha_tr=info.alpha_tr,
                                  alpha0=info.alpha0, loss_k=list(info.loss[:BACKTRACKS]),
                                  shift_k=list(info.shift[:BACKTRACKS]))
        q = dict(before=loss(bl, x, ret), fit_tr_1=loss(bl, x1, ret))
        assert q["before"] == info.loss_before or abs(q["before"] - info.loss_before) <= 1e-12 * q["before"]
        xs = x
        for _ in range(3):
            xs = fit_tr(xs)[0]
        q["fit_tr_3"] = loss(bl, xs, ret)
        # how far one uncapped step goes as the trust region widens
        q["fit_tr_1_by_eps"] = {str(e): loss(bl, bl.fit_tr(x, e, CG_ITERS, CG_TH, DAMPING, BACKTRACKS)[0], ret)
                                for e in (0.01, 0.1, 1.0)}
        if ref is not None:
            out["lbfgs"] = stats(t_lb)
            out["lbfgs_rc"] = int(rc)
            out["lbfgs_over_fit_tr"] = round(out["lbfgs"]["med"] / out["fit_tr"]["med"], 2)
            q["lbfgs_25"] = loss(bl, x_lb, ret)
        out["loss"] = q
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
