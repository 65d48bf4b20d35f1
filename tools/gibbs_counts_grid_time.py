#!/usr/bin/env python3
"""Time per Gibbs iteration of rpvg_hip_gibbs_read_counts on single large clusters (tests/large_cases.py), on one workgroup and
over the whole GPU (rpvg_amd/csrc/gibbs_grid.hip).

    python tools/gibbs_counts_grid_time.py [TREE] [LABEL] [THRESHOLDS]

TREE: the root of the tree whose librpvg_hip.so is timed (default: this one; a build of another commit for an A/B on one box).
THRESHOLDS: comma-separated values of RPVG_HIP_EM_GRID_MIN_WORK to take in turn (default "0,1000": one workgroup, grid).
Per case and threshold: the EM estimate as the start, then 20 samples thinned by 5 (100 iterations), one warm-up and five timed
calls.  Prints one JSON line each: the wall time of the call and the device span of its sampler kernels (em_sparse_ms), both per
iteration, as medians."""
import ctypes as C
import json
import os
import statistics
import sys
import time

root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
label = sys.argv[2] if len(sys.argv) > 2 else os.path.basename(root)
thresholds = (sys.argv[3] if len(sys.argv) > 3 else "0,1000").split(",")
sys.path.insert(0, root)
import numpy as np  # noqa: E402

from rpvg_amd import hip  # noqa: E402
from tests import large_cases  # noqa: E402

CASES = [("60000x150x3", (60000, 150, 3, 1)), ("200000x400x3", (200000, 400, 3, 2)), ("8000x400x40", (8000, 400, 40, 4)),
         # smaller ones, for the break-even of one problem
         ("16000x100x3", (16000, 100, 3, 6)), ("4000x60x3", (4000, 60, 3, 7)), ("1000x40x3", (1000, 40, 3, 8)), ("400x100x40", (400, 100, 40, 9))]
N, THIN = 20, 5

ctx = hip.Context(0)
for name, (rows, paths, per_row, seed) in CASES:
    batch = large_cases.cluster_batch(rows, paths, per_row, seed=seed, noise_only_frac=0.01)
    dev = ctx.upload(batch)
    cols = [list(range(paths))]
    os.environ["RPVG_HIP_EM_GRID_MIN_WORK"] = "100000"
    abund, noise, total, _ = ctx.em_solve(dev, [0], cols, max_em_its=50)
    cl = np.zeros(1, dtype=np.uint32)
    col_off = np.array([0, paths], dtype=np.uint64)
    col_path = np.arange(paths, dtype=np.uint32)
    init = np.ascontiguousarray(abund[0], dtype=np.float64)
    init_noise = np.ascontiguousarray(noise, dtype=np.float64)
    n = np.array([N], dtype=np.uint32)
    seeds = np.array([12345], dtype=np.uint64)
    out_noise = np.zeros(N, dtype=np.float64)
    out_abund = np.zeros(N * paths, dtype=np.float64)
    probs = hip.CEmProblems(1, cl.ctypes.data, col_off.ctypes.data, col_path.ctypes.data, 0.0)
    for threshold in thresholds:
        os.environ["RPVG_HIP_EM_GRID_MIN_WORK"] = threshold
        wall, span = [], []
        for run in range(6):
            ctx.reset_stats()
            t0 = time.perf_counter()
            hip._check(hip.lib().rpvg_hip_gibbs_read_counts(ctx.handle, dev.handle, C.byref(probs), C.c_void_p(init.ctypes.data),
                                                            C.c_void_p(init_noise.ctypes.data), C.c_void_p(n.ctypes.data),
                                                            C.c_void_p(seeds.ctypes.data), C.c_uint32(THIN), C.c_double(1.0),
                                                            C.c_void_p(out_noise.ctypes.data), C.c_void_p(out_abund.ctypes.data)),
                       "rpvg_hip_gibbs_read_counts")
            wall.append(time.perf_counter() - t0)
            st = ctx.stats()
            span.append(st["em_sparse_ms"])
        conserved = float(np.max(np.abs(out_abund.reshape(N, paths).sum(axis=1) + out_noise - total[0])) / total[0])
        print(json.dumps(dict(label=label, case=name, min_work=threshold, grid_problems=int(st.get("gibbs_count_grid_problems", 0)),
                              wall_us_per_iteration=round(statistics.median(wall[1:]) * 1e6 / (N * THIN), 1),
                              span_us_per_iteration=round(statistics.median(span[1:]) * 1e3 / (N * THIN), 1),
                              warmup_wall_ms=round(wall[0] * 1e3, 2), runs_wall_ms=[round(w * 1e3, 2) for w in wall[1:]],
                              mass_error=conserved)), flush=True)
    dev.free()
ctx.close()
