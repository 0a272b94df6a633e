"""Record tests/golden/step_trim_solves.txt and step_trim_update.txt from the library TRPO_LIB names (or the
built one): the solves and updates of tests/test_gpu_step_trim.py, run by that module's own functions.

    TRPO_LIB=/path/to/parent/libtrpo_mi355x.so python tools/record_step_trim.py "commit 4a0ae4d" OUTDIR
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "trpo-robot-control_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))

import test_gpu_step_trim as T  # noqa: E402


def main():
    what, outdir = sys.argv[1], sys.argv[2]
    os.makedirs(outdir, exist_ok=True)
    head = "# recorded from %s by tools/record_step_trim.py; lines `case %s column value`\n"
    with open(os.path.join(outdir, os.path.basename(T.GOLDEN)), "w") as f:
        f.write(head % (what, "maxiter"))
        for key, case in T.CASES.items():
            f.write("\n".join(T.golden_lines(key, case["solves"], T.run_case(case))) + "\n")
    with open(os.path.join(outdir, os.path.basename(T.GOLDEN_UPDATE)), "w") as f:
        f.write(head % (what, "update"))
        for key, (net, n) in T.UPDATE_CASES.items():
            f.write("\n".join(T.update_lines(key, T.updates(net, n))) + "\n")


if __name__ == "__main__":
    main()
