#!/usr/bin/env python3
"""A batch of small registrations (mopt_batch) against the same solves one after another.

    python scripts/batch_solve_timing.py [--sizes 1 16 256 1024 4096] [--limit-s 120]

B problems of 1000 fp64 correspondences each (the fixture pose, noise 0.01, a seed per problem), analytic
Jacobian, start at 0.  Per B: the median of 20 timed Point2PointBatch.minimize calls after 3 warm-ups, and,
for B <= 256, the median of 20 rounds of B sequential mopt_lm_minimize calls on B lone costs in the same
process.  Creation (upload + re-layout of the batch) is timed apart and is never part of a solve time.
Each B runs in a child process of its own under a time limit, so that one stuck size ends that size only;
the parent prints one line per B.  MOPT_LIBRARY selects another build of the library, as everywhere."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 1000
TIMED, WARMUPS = 20, 3
SEQUENTIAL_UP_TO = 256


def one_size(B):
    import numpy as np

    import moptimizer_0_amd as mo
    from tests import datasets as ds

    pairs = [ds.synthetic_pair(N, seed=100 + i, noise=0.01) for i in range(B)]
    srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
    warm = mo.Point2PointBatch(srcs[:1], tgts[:1])  # context, streams, code objects
    warm.minimize(np.zeros((1, 6)), mo.JAC_ANALYTIC)
    warm.close()
    created = []
    for _ in range(3):
        t0 = time.perf_counter()
        batch = mo.Point2PointBatch(srcs, tgts)
        created.append(time.perf_counter() - t0)
        batch.close()
    batch = mo.Point2PointBatch(srcs, tgts)
    x0s = np.zeros((B, 6))
    times = []
    for k in range(WARMUPS + TIMED):
        t0 = time.perf_counter()
        xs, reps = batch.minimize(x0s, mo.JAC_ANALYTIC)
        times.append(time.perf_counter() - t0)
    batch_ms = statistics.median(times[WARMUPS:]) * 1e3
    err = float(np.abs(xs - ds.FIXTURE_X).max())
    line = "B=%5d  batch minimize %9.3f ms (%7.2f us a problem; min %.3f max %.3f)  iterations %d..%d  max |x - fixture| %.1e" % (
        B, batch_ms, batch_ms * 1e3 / B, min(times[WARMUPS:]) * 1e3, max(times[WARMUPS:]) * 1e3,
        min(r["iterations"] for r in reps), max(r["iterations"] for r in reps), err)
    if B <= SEQUENTIAL_UP_TO:
        costs = [mo.Point2PointCost(s, t) for s, t in pairs]
        rounds = []
        for k in range(WARMUPS + TIMED):
            t0 = time.perf_counter()
            for c in costs:
                mo.capi.lm_minimize([c], [mo.JAC_ANALYTIC], np.zeros(6))
            rounds.append(time.perf_counter() - t0)
        seq_ms = statistics.median(rounds[WARMUPS:]) * 1e3
        line += "  |  %d sequential mopt_lm_minimize %9.3f ms (%7.2f us each): batch %.1fx" % (
            B, seq_ms, seq_ms * 1e3 / B, seq_ms / batch_ms)
        for c in costs:
            c.close()
    line += "  |  create (upload + re-layout of %d x %d) %.2f ms (best of 3; first %.2f)" % (
        B, N, min(created) * 1e3, created[0] * 1e3)
    batch.close()
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 16, 256, 1024, 4096])
    ap.add_argument("--limit-s", type=int, default=120, help="time limit of each size's child process")
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        one_size(args.one)
        return 0
    for B in args.sizes:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(B)],
                                timeout=args.limit_s).returncode
        except subprocess.TimeoutExpired:
            print("B=%5d  no result within %d s: stopping here" % (B, args.limit_s), flush=True)
            return 1
        if rc != 0:  # a fault ends the run: nothing more is started on the device
            print("B=%5d  child ended with status %d: stopping here" % (B, rc), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
