#!/usr/bin/env python3
"""Wall time of engine.run("haplotypes", use_hap_gibbs=1) at ploidy 4 and 8 on one fixed synthetic batch — 500 clusters of the
configs[4] shape (rpvg_amd/synth.py) cut to at most 200 columns — one warm-up and three runs each.

    RPVG_AMD_TRACE=1 python tools/gibbs_polyploid_time.py [TREE] [LABEL]

TREE: the root of the tree whose libraries are timed (default: this one; a build of another commit for an A/B on one box).
With RPVG_AMD_TRACE=1 the phase trace on stderr carries the round and conditional counts of every sampler call.
Prints one JSON line per run and one per ploidy."""
import json
import os
import sys
import time

root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
label = sys.argv[2] if len(sys.argv) > 2 else os.path.basename(root)
sys.path.insert(0, root)
import numpy as np  # noqa: E402

from rpvg_amd import engine as eng_mod, synth  # noqa: E402
from rpvg_amd.batch import make_params  # noqa: E402

batch = synth.generate(seed=5, num_clusters=500, total_paths=50000, total_reads=1000000, max_cluster_paths=200)
cols = np.diff(batch.cluster_path_off)
print(json.dumps(dict(label=label, clusters=int(batch.num_clusters), columns=int(cols.sum()), widest=int(cols.max()))), flush=True)
e = eng_mod.Engine(0)
prep = e.prepare(batch)
for ploidy in (4, 8):
    params = make_params(use_hap_gibbs=1, ploidy=ploidy, rng_seed=5)
    times = []
    for r in range(4):
        e.reset_stats()
        t0 = time.perf_counter()
        e.run_raw("haplotypes", params, prep)
        times.append(time.perf_counter() - t0)
        st = e.stats()
        print(json.dumps(dict(label=label, ploidy=ploidy, run=r, seconds=round(times[-1], 4), gibbs_ms=round(st["gibbs_ms"], 2),
                              loglik_ms=round(st["loglik_ms"], 2))), flush=True)
    print(json.dumps(dict(label=label, ploidy=ploidy, warmup=round(times[0], 4), runs=[round(t, 4) for t in times[1:]])), flush=True)
e.close()
