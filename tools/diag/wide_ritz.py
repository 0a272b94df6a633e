"""CPU: the stall condition of the wide-policy tests (tests/test_gpu_wide.py).  The wide path never re-solves
in fp64, so every CG / update case it is compared on must be one where the reference's own fp64 CG is not a
stalled solve: for each problem of tests/wide_cases.py the reference's recurrence on the oracle FVP
(tools/diag/ritz_probe.py's computation) and the smallest relative Ritz residual of its Lanczos matrices, for
the CG test's solve (b, 10 iterations, threshold 0) and the update's (the policy gradient, threshold 1e-10).
Both must stay >= 1e-13, ten times the guard's threshold; a case below it gets another seed."""
import os
import sys
import time

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path[:0] = [os.path.join(R, "tests"), os.path.join(R, "trpo-robot-control_amd"), os.path.join(R, "oracle")]
import wide_cases as W  # noqa: E402

if __name__ == "__main__":
    probs = [(name, W.case(name)) for name in W.CASES]
    layers, acts, seed = W.EDGE_SHAPE
    probs += [("edge n=%d" % n, W.make(layers, acts, n, seed)) for n in W.EDGE_N]
    for name, p in probs:
        t0 = time.time()
        cg = W.ritz_of(p, p["b"], 10, 0.0)
        if name in W.CASES:
            up = W.ritz_of(p, W.reference(name)["pg"], 10, 1e-10)
            print("%-12s %s %s n=%d: cg %.2e update %.2e  (%.1f s with the references)"
                  % (name, p["layers"], p["acts"], p["n"], cg, up, time.time() - t0), flush=True)
        else:
            print("%-12s cg %.2e" % (name, cg), flush=True)
