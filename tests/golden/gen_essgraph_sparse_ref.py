"""Writes tests/golden/essgraph_sparse_ref.npz: the cases of tests/essgraph_sparse_cases.py (maps
above the dense solver's 878 keyframes) run by the reference's own g2o, by the driver, the three
difference steps and the conditions of tests/golden/gen_essgraph_ref.py, all imported from there
and none weakened: the three runs share every integer output, no edge sits within 10 % of a 1e-5
branch threshold, the one trial is accepted in all three and at least 90 % of the free keyframes
move by more than 100 x the case's `sim3` tolerance.  The keys are those of essgraph_ref.npz, so
essgraph_cases.compare reads this file unchanged.

--host adds the host replica's tier (`host_<case>_*`) as gen_essgraph_ref.py does; its dense
LDL^T of the 6993-row system takes minutes per run.

    python tests/golden/gen_essgraph_sparse_ref.py [--host]      # needs the reference checkout
"""
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "multicol-slam-annotation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import essgraph_cases as ec  # noqa: E402
from tests import essgraph_sparse_cases as sc  # noqa: E402
from tests.golden.gen_essgraph_ref import (build_driver, build_host, check_and_measure, check_one_trial,  # noqa: E402
                                           run_host, run_reference, spread_of)

OUT = os.path.join(HERE, "essgraph_sparse_ref.npz")


def generate(with_host):
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        host = build_host(tmp) if with_host else None
        for name in sc.SPARSE_CASES:
            case = sc.make_sparse_case(name)
            t0 = time.perf_counter()
            runs = run_reference(exe, case, tmp)
            dt = (time.perf_counter() - t0) / 3
            spread = check_and_measure(name, runs)
            frac = check_one_trial(name, case, runs, spread)
            data[name + "_sha256"] = np.array(ec.digest(case))
            for f in ec.INTS + ec.REALS + ("lambda", "chi2_initial"):
                data["%s_%s" % (name, f)] = np.asarray(runs[0][f])
            for f in ec.REALS:
                data["measured_%s_%s" % (name, f)] = np.float64(spread[f])
            print(name, "E", len(runs[0]["edges"]), "counts", runs[0]["counts"].tolist(), "iterations",
                  runs[0]["iterations"], "trials", runs[0]["trials"].tolist(), "chi2 %.6g -> %.6g" %
                  (runs[0]["chi2_initial"], runs[0]["chi2"][-1]), "margin %.3g" % min(r["branch_margin"] for r in runs),
                  "%.2f s per run" % dt)
            print("  spread", {f: float(spread[f]) for f in ec.REALS})
            print("  moved %.3f of the free keyframes" % frac)
            if with_host:
                t0 = time.perf_counter()
                hruns = run_host(host, case, tmp)
                print("  host replica %.1f s per run" % ((time.perf_counter() - t0) / 3))
                for f in ("edges", "counts", "iterations", "trials"):
                    for r in hruns:
                        assert np.array_equal(r[f], runs[0][f]), "%s: %s of the host replica differs" % (name, f)
                hspread = spread_of(hruns)
                for f in ("iterations", "trials") + ec.REALS:
                    data["host_%s_%s" % (name, f)] = np.asarray(hruns[0][f])
                for f in ec.REALS:
                    data["measured_host_%s_%s" % (name, f)] = np.float64(hspread[f])
                print("  host spread", {f: float(hspread[f]) for f in ec.REALS})
                print("  host - g2o", {f: ec.diff(f, hruns[0][f], runs[0][f]) for f in ec.REALS})
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    generate("--host" in sys.argv[1:])
