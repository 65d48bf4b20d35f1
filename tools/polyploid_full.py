#!/usr/bin/env python3
"""Rate of the full enumeration of the polyploid haplotype posteriors (rpvg_hip_group_full_posteriors) next to the Gibbs
conditionals kernel (rpvg_hip_group_conditionals) on the same matrices, and, optionally, the CPU oracle.

    python tools/polyploid_full.py [--g 6] [--cols 40] [--rows 2000] [--problems 16] [--reps 3]
                                   [--oracle-problems N] [--oracle-threads 16]

Prints one JSON line.  Kernel times are the HIP-event spans of the calls (rpvg_hip_stats_get: loglik_ms, the enumeration
kernel and its normalisation); row evaluations = sets x rows (one log argument of one row of one set).  --oracle-problems N
times the oracle's `-i haplotypes` on the first N problems with --oracle-threads threads (0: skipped; the oracle needs no
GPU).
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from rpvg_amd.batch import ClusterBatch, make_params  # noqa: E402


def cluster(rng, rows, paths):
    """`rows` distinct rows over `paths` single-path columns, 1 .. 4 paths per row, counts 1 .. 4."""
    rs = []
    for _ in range(rows):
        k = int(rng.integers(1, 5))
        idx = sorted(rng.choice(paths, size=k, replace=False).tolist())
        noise = float(rng.choice([1e-4, 1e-3, 1e-2]))
        w = rng.random(k) + 0.1
        w = w / w.sum() * (1 - noise)
        order = np.argsort(w)
        rs.append((int(rng.integers(1, 5)), noise, [(float(w[i]) + 1e-7 * j, [idx[i]]) for j, i in enumerate(order)]))
    return dict(paths=[dict(group_id=0, source_count=1, source_ids=[h], effective_length=100.0) for h in range(paths)], rows=rs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, default=6)
    ap.add_argument("--cols", type=int, default=40)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--problems", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--oracle-problems", type=int, default=0)
    ap.add_argument("--oracle-threads", type=int, default=16)
    ap.add_argument("--no-gpu", action="store_true", help="the oracle only")
    a = ap.parse_args()

    rng = np.random.default_rng(2026)
    clusters = [cluster(rng, a.rows, a.cols) for _ in range(a.problems)]
    batch = ClusterBatch.from_clusters(clusters)
    sets = math.comb(a.cols + a.g - 1, a.g)
    out = dict(g=a.g, cols=a.cols, rows=a.rows, problems=a.problems, sets_per_problem=sets)

    if not a.no_gpu:
        from rpvg_amd import hip
        ctx = hip.Context(0)
        dev = ctx.upload(batch)
        mats = list(range(a.problems))
        dg = ctx.groups(dev, mats, None, False)
        num_cols = [a.cols] * a.problems
        lf = [np.log(np.full(a.cols, 1.0 / a.cols))] * a.problems
        dg.full_posteriors(mats[:1], a.g, lf[:1], num_cols)  # warm-up (code objects, pools)
        full_ms, walls = [], []
        for _ in range(a.reps):
            ctx.reset_stats()
            t0 = time.perf_counter()
            post = dg.full_posteriors(mats, a.g, lf, num_cols)
            walls.append(time.perf_counter() - t0)
            full_ms.append(ctx.stats()["loglik_ms"])
        assert all(abs(p.sum() - 1.0) < 1e-9 for p in post)
        evals = float(sets) * a.rows * a.problems
        best = min(full_ms)
        out.update(full_kernel_ms=best, full_wall_s=min(walls), full_sets_per_s=sets * a.problems / (best * 1e-3),
                   full_row_evals_per_s=evals / (best * 1e-3))
        # the conditionals of the Gibbs route, width g: every candidate column given g - 1 others, over the same rows
        nreq = 4096
        req_m = [int(x) for x in rng.integers(0, a.problems, size=nreq)]
        req_o = [[int(x) for x in rng.integers(0, a.cols, size=a.g - 1)] for _ in req_m]
        dg.conditionals(req_m[:8], req_o[:8], a.g, float(a.g), num_cols)
        cond_ms = []
        for _ in range(a.reps):
            ctx.reset_stats()
            dg.conditionals(req_m, req_o, a.g, float(a.g), num_cols)
            cond_ms.append(ctx.stats()["loglik_ms"])
        cevals = float(nreq) * a.cols * a.rows
        out.update(conditionals_kernel_ms=min(cond_ms), conditionals_row_evals_per_s=cevals / (min(cond_ms) * 1e-3))
        out["full_vs_conditionals_rate"] = out["full_row_evals_per_s"] / out["conditionals_row_evals_per_s"]
        dg.free()
        ctx.close()

    if a.oracle_problems > 0:
        from oracle import pyoracle
        sub = ClusterBatch.from_clusters(clusters[:a.oracle_problems])
        t0 = time.perf_counter()
        pyoracle.run("haplotypes", make_params(ploidy=a.g), sub, a.oracle_threads)
        secs = time.perf_counter() - t0
        out.update(oracle_problems=a.oracle_problems, oracle_threads=a.oracle_threads, oracle_s=secs,
                   oracle_row_evals_per_s=float(sets) * a.rows * a.oracle_problems / secs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
