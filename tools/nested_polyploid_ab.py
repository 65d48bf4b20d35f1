#!/usr/bin/env python3
"""`haplotype-transcripts` at ploidy 5, 6 and 8 with exact posteriors: the one-call route (rpvg_hip_nested_full_subset_em: enumeration,
retained sets, subsets, EM and merge on the device) against the separate calls — on this tree with and without
RPVG_HIP_NO_DEVICE_SUBSETS=1, and on a build of the parent commit (which has the separate calls only) in the same job on the same box.

    python tools/nested_polyploid_ab.py [--parent TREE] [--out profiles/nested_polyploid/ab.txt] [--shapes small,mid,large]
    python tools/nested_polyploid_ab.py --resources [profiles/nested_polyploid/resource_usage.txt]     (cross-compiles; needs no GPU)

Shapes: synth-generated batches (rpvg_amd/synth.py) whose number of haplotypes bounds the haplotype columns of a cluster so that a
cluster has about 10^3 (small), 10^5 (mid) and 10^6 (large) sets; 500 clusters, fewer for `large` (--large-clusters: the separate calls
hold 8 + 4 x ploidy bytes per set on the host).  Every (tree, route) runs in a process of its own (--child): one warm-up, then three
timed calls of estimateBatch (Engine.run: wall time around the call, which waits for the device); the median and the spread are
listed.  The estimates of every process are compared with the one-call route's before a time is written: sets and posteriors equal,
EM iterations and columns equal, abundances and noise at rel 1e-12.  The retain pass alone is the difference of the two routes'
loglik_ms on this tree (HIP events around enumeration + normalisation, + the retain pass on the one-call route): a figure inside the
spans' own run-to-run spread (it comes out negative then) says the pass is not resolved by this method."""
import argparse
import json
import math
import os
import pickle
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from _resources import resource_usage  # noqa: E402

# haplotypes of the generator (an upper bound of a cluster's columns) by ploidy and shape
HAPLOTYPES = {5: dict(small=8, mid=24, large=40), 6: dict(small=7, mid=18, large=28), 8: dict(small=6, mid=13, large=18)}


def make_batch(ploidy, shape, clusters):
    from rpvg_amd import synth
    haps = HAPLOTYPES[ploidy][shape]
    return synth.generate(seed=11 + ploidy, num_clusters=clusters, total_paths=clusters * max(haps, 4), total_reads=200 * clusters,
                          num_haplotypes=haps, max_cluster_paths=64)


def columns_of(batch):
    """Haplotype columns of every cluster: distinct path lists over the haplotypes (findPathSourceGroups)."""
    import numpy as np
    out = []
    for k in range(batch.num_clusters):
        p0, p1 = int(batch.cluster_path_off[k]), int(batch.cluster_path_off[k + 1])
        by_source = {}
        for p in range(p0, p1):
            for s in batch.source_id[int(batch.path_source_off[p]):int(batch.path_source_off[p + 1])]:
                by_source.setdefault(int(s), []).append(p - p0)
        out.append(len({tuple(v) for v in by_source.values()}))
    return np.asarray(out)


def child(args):
    """One (tree, route): every shape, a warm-up and three timed runs each; estimates and figures pickled to --child-out."""
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    from rpvg_amd import engine as eng_mod
    from rpvg_amd.batch import make_params
    results = {}
    e = eng_mod.Engine(0)
    try:
        for ploidy in (5, 6, 8):
            for shape in args.shapes.split(","):
                clusters = args.large_clusters if shape == "large" else args.clusters
                batch = make_batch(ploidy, shape, clusters)
                cols = columns_of(batch)
                sets = [math.comb(int(c) + ploidy - 1, ploidy) if c else 0 for c in cols]
                prep = e.prepare(batch)
                params = make_params(ploidy=ploidy)
                times, stats, est = [], None, None
                for r in range(4):
                    e.reset_stats()
                    t0 = time.perf_counter()
                    est, _ = e.run("haplotype-transcripts", params, prep)
                    times.append(time.perf_counter() - t0)
                    stats = e.stats()
                prep.free()
                results[(ploidy, shape)] = dict(
                    clusters=clusters, total_sets=int(sum(sets)), mean_sets=float(np.mean(sets)), max_sets=int(max(sets)), times=times[1:],
                    warmup=times[0], loglik_ms=stats["loglik_ms"], calls=stats.get("nested_full_calls", 0), retained=stats.get("nested_full_retained", 0),
                    estimates=[(x.path_group_sets, np.asarray(x.posteriors), np.asarray(x.abundances), x.noise_count, x.total_count, list(x.em_iters),
                                x.em_cols) for x in est])
                print(json.dumps(dict(label=args.label, ploidy=ploidy, shape=shape, seconds=[round(t, 4) for t in times])), flush=True)
    finally:
        e.close()
    with open(args.child_out, "wb") as f:
        pickle.dump(results, f)
    return 0


def same_estimates(a, b):
    import numpy as np

    def close(x, y):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        return x.shape == y.shape and bool(np.all(np.abs(x - y) <= np.maximum(1e-12 * np.maximum(np.abs(x), np.abs(y)), 1e-300)))
    return len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) and close(x[2], y[2]) and close(x[3], y[3]) and x[4] == y[4] and
                                    x[5] == y[5] and x[6] == y[6] for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="root of a built tree of the parent commit")
    ap.add_argument("--shapes", default="small,mid,large")
    ap.add_argument("--clusters", type=int, default=500)
    ap.add_argument("--large-clusters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nested_polyploid", "ab.txt"))
    ap.add_argument("--resources", nargs="?", const=os.path.join(ROOT, "profiles", "nested_polyploid", "resource_usage.txt"), default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--child-out", default=None)
    args = ap.parse_args()
    if args.resources:
        resource_usage("subset_full.hip", args.resources, width=32, spills=True,
                       header_note=" (subsetOffsetsKernel and packResultsKernel: subset_pack.hpp, shared with subset_em.hip)",
                       footer=("No kernel uses scratch memory.  fullSelectKernel<8> parks 6 scalar registers in lanes of a vector register (two list walks of eight",
                               "cursors each are live in a comparison): no memory traffic, accepted."))
        return 0
    if args.child:
        return child(args)

    import numpy as np
    runs = [("one call", ROOT, {}), ("separate calls, this tree", ROOT, {"RPVG_HIP_NO_DEVICE_SUBSETS": "1"})]
    if args.parent:
        runs.append(("parent commit", os.path.abspath(args.parent), {}))
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        for label, tree, env in runs:
            out = os.path.join(tmp, label.replace(" ", "_").replace(",", "") + ".pickle")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--label", label, "--child-out", out, "--shapes", args.shapes,
                   "--clusters", str(args.clusters), "--large-clusters", str(args.large_clusters)]
            child_env = dict(os.environ, **env)
            child_env.pop("PYTHONPATH", None)
            subprocess.run(cmd, check=True, env=child_env, cwd=tree, timeout=900)
            with open(out, "rb") as f:
                results[label] = pickle.load(f)
    lines = ["haplotype-transcripts, exact posteriors, -n 0: wall time of estimateBatch (Engine.run, inputs on the device), seconds; median of 3 after a",
             "warm-up, (min .. max).  one call: rpvg_hip_nested_full_subset_em; separate calls: posteriors of every set to the host, subsets on the host,",
             "EM on the device, merge on the host (this tree with RPVG_HIP_NO_DEVICE_SUBSETS=1, and the parent commit's build in the same job).",
             "posterior D2H: bytes of posteriors copied device -> host per batch (8 B per set on the separate route, none on the one-call route, whose",
             "one packed block is proportional to the retained subsets).  retain pass: loglik_ms (HIP events) of the one-call route minus that of the",
             "separate calls on this tree — enumeration and normalisation are the same kernels on both, the retain pass is the difference, where it",
             "exceeds the run-to-run spread of the spans (a negative figure says it does not).", ""]
    ok = True
    one = results["one call"]
    for key in sorted(one):
        ploidy, shape = key
        r = one[key]
        lines.append(f"ploidy {ploidy}, {shape}: {r['clusters']} clusters, {r['total_sets']} sets ({r['mean_sets']:.0f} per cluster, largest {r['max_sets']}), "
                     f"{r['retained']} retained, one-call calls {r['calls']}")
        med_one = float(np.median(r["times"]))
        for label, _, _ in runs:
            x = results[label][key]
            med = float(np.median(x["times"]))
            same = same_estimates(one[key]["estimates"], x["estimates"])
            ok = ok and same
            d2h = 0 if label == "one call" else 8 * x["total_sets"]
            lines.append(f"  {label:<28} {med:9.4f}  ({min(x['times']):.4f} .. {max(x['times']):.4f})   x{med / med_one:6.2f} of one call   "
                         f"posterior D2H {d2h / 1e6:10.2f} MB   loglik_ms {x['loglik_ms']:9.3f}   estimates equal: {same}")
        sep = results["separate calls, this tree"][key]
        lines.append(f"  loglik_ms, one call minus separate calls (the retain pass, if it shows above the spans' own spread): "
                     f"{r['loglik_ms'] - sep['loglik_ms']:.3f} ms of {r['loglik_ms']:.3f} ms; fused into the normalisation: not built, not measured")
        lines.append("")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
