#!/usr/bin/env python3
"""Kernel phase breakdown (diagnostic; GPU box).

Runs the batched driver against libabpoa_amd_kprof.so (make kprof), which
carries s_memtime counters around each phase of the convex DP kernel's row
loop and each pass of the per-round fold kernel, then prints where the
cycles go. Relative shares are the point; the absolute clock of s_memtime
is not calibrated here.

Usage: python tools/kprof_run.py [n_sets] [depth] [qlen]
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("ABPOA_AMD_LIB", os.path.join(
    ROOT, "abpoa_amd", "csrc", "libabpoa_amd_kprof.so"))  # or another kprof build

import abpoa_amd  # noqa: E402
import bench  # noqa: E402
import numpy as np  # noqa: E402


def fetch(lib, name):
    out = (ctypes.c_uint64 * 32)()
    getattr(lib, name)(out)
    return list(out)


def main():
    n_sets = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    depth = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    qlen = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
    L = abpoa_amd.lib()
    rng = np.random.default_rng(7)
    sets = bench.gen_sets(rng, n_sets, depth=depth, qlen=qlen)
    L.abamd_kprof_reset()
    L.abamd_kprof_fold_reset()
    abpoa_amd.msa_batch_consensus(sets, n_threads=8)
    k = fetch(L, "abamd_kprof_fetch")
    f = fetch(L, "abamd_kprof_fold_fetch")

    mwa, mwb, mwc, mwtot, mwrows = k[11], k[12], k[13], k[14], k[15]
    if mwrows:
        print("== cg MULTI-WAVE kernel (%d rows, %.0f cyc/row total) ==" %
              (mwrows, mwtot / mwrows))
        for name, v in (("gather+hpre", mwa), ("B1+scan+B2+fold", mwb),
                        ("carry+B3", mwc), ("epilogue", mwtot - mwa - mwb - mwc)):
            print("  %-16s %12d cyc  (%.0f cyc/row)" % (name, v, v / mwrows))
        # rows by predecessor class; the class is what a full-depth ring can
        # serve, so a run with ABPOA_AMD_DP_RING=1 shows what each class costs
        # without the ring
        print("  ring depth in use: %s" % os.environ.get("ABPOA_AMD_DP_RING", "default"))
        print("  %-22s %9s %6s %12s %12s %12s %6s" %
              ("row class", "rows", "%rows", "gather/row", "epilogue/row", "total/row", "%cyc"))
        for c, name in enumerate(("fast1 (only r-1)", "all preds in ring",
                                  ">=1 arena gather")):
            n, ga, ep, tot = k[16 + c], k[19 + c], k[22 + c], k[25 + c]
            print("  %-22s %9d %5.1f%% %12.0f %12.0f %12.0f %5.1f%%" %
                  (name, n, 100.0 * n / mwrows, ga / max(n, 1), ep / max(n, 1),
                   tot / max(n, 1), 100.0 * tot / max(mwtot, 1)))
        print("  rows wider than a ring slot: %d (%.2f%%)" % (k[28], 100.0 * k[28] / mwrows))
        print("  rows with more predecessors than are rolled ahead: %d (%.2f%%); "
              "mean in-degree %.3f" % (k[29], 100.0 * k[29] / mwrows, k[30] / mwrows))

    fjobs, fapply, findeg, fbfs, fsort, fremspan, fbuild = f[:7]
    ftot = fapply + findeg + fbfs + fsort + fremspan + fbuild
    print("== fold kernel (%d jobs) ==" % fjobs)
    for name, v in (("apply", fapply), ("in_deg", findeg), ("bfs", fbfs),
                    ("sort", fsort), ("remain+nspan", fremspan), ("build_rows", fbuild)):
        print("  %-14s %12d cyc  %5.1f%%  (%.0f cyc/job)" %
              (name, v, 100.0 * v / max(ftot, 1), v / max(fjobs, 1)))


if __name__ == "__main__":
    main()
