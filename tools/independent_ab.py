#!/usr/bin/env python3
"""`haplotype-transcripts --ind-hap-inference` with exact posteriors at ploidy 2: the one-call route
(rpvg_hip_nested_independent_subset_em: posteriors, draws, subsets, EM and merge on the device) against the separate route
(posteriors to the host, draws and maps on the host, EM on the device, merge on the host), which RPVG_HIP_NO_DEVICE_SUBSETS=1 forces
— both in one process, on the batch of the BASELINE.json configs[2] generator and on a twentieth of it.

    python tools/independent_ab.py [--out profiles/independent_subsets/ab.txt] [--scales 1.0,0.05] [--label TEXT]

Per (scale, route): one warm-up, then three timed calls of estimateBatch (Engine.run: wall time around the call, which waits for the
device) with the process's CPU time (all threads) next to it; medians and (min .. max) are listed.  The estimates of the two routes
are compared for equality — sets, posteriors, abundances, noise, EM iterations and columns, bit for bit — before a time is written.
A build of the parent commit has the separate route only: run the tool there with --label to write its line down next to these."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bits(estimates):
    import numpy as np
    return [(e.path_group_sets, np.asarray(e.posteriors).tobytes(), np.asarray(e.abundances).tobytes(), e.noise_count, e.total_count,
             list(e.em_iters), e.em_cols) for e in estimates]


def measure(engine, params, prep, runs=3):
    wall, cpu, est = [], [], None
    for r in range(runs + 1):
        c0, t0 = time.process_time(), time.perf_counter()
        est, _ = engine.run("haplotype-transcripts", params, prep)
        t1, c1 = time.perf_counter(), time.process_time()
        if r > 0:  # (the first call is the warm-up)
            wall.append((t1 - t0) * 1e3)
            cpu.append((c1 - c0) * 1e3)
    return wall, cpu, est


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "independent_subsets", "ab.txt"))
    ap.add_argument("--scales", default="1.0,0.05")
    ap.add_argument("--label", default="this tree")
    args = ap.parse_args()

    import numpy as np
    from rpvg_amd import engine as eng_mod, synth
    from rpvg_amd.batch import make_params

    lines = ["haplotype-transcripts --ind-hap-inference, ploidy 2, exact posteriors, -n 0: estimateBatch (Engine.run, inputs on the device), milliseconds per",
             "batch; median of 3 after a warm-up, (min .. max).  wall: around the call, which waits for the device; host CPU: CPU time of the process, all",
             "threads.  device route: rpvg_hip_nested_independent_subset_em; separate route: RPVG_HIP_NO_DEVICE_SUBSETS=1, the parent commit's code.", ""]
    ok = True
    engine = eng_mod.Engine(0)
    try:
        for scale in (float(x) for x in args.scales.split(",")):
            K = max(8, int(round(5000 * scale)))
            batch = synth.generate(seed=3, num_clusters=K, total_paths=max(K, int(round(200000 * scale))), total_reads=int(round(10000000 * scale)))
            prep = engine.prepare(batch)
            params = make_params(ind_hap_inference=1, rng_seed=7)
            results = {}
            for route, env in (("device route", None), ("separate route", "1")):
                if env is None:
                    os.environ.pop("RPVG_HIP_NO_DEVICE_SUBSETS", None)
                else:
                    os.environ["RPVG_HIP_NO_DEVICE_SUBSETS"] = env
                engine.reset_stats()
                wall, cpu, est = measure(engine, params, prep)
                stats = engine.independent_stats() if hasattr(engine, "independent_stats") else dict(calls_completed=0, draws=0, subsets=0)
                results[route] = (wall, cpu, bits(est), stats)
            os.environ.pop("RPVG_HIP_NO_DEVICE_SUBSETS", None)
            prep.free()
            same = results["device route"][2] == results["separate route"][2]
            ok = ok and same
            lines.append(f"{args.label}, scale {scale:g}: {batch.num_clusters} clusters, {int(batch.cluster_path_off[-1])} paths; estimates of the two routes equal bit for bit: {same}")
            for route in ("device route", "separate route"):
                wall, cpu, _, stats = results[route]
                lines.append(f"  {route:<15} wall {np.median(wall):10.2f} ms ({min(wall):.2f} .. {max(wall):.2f})   host CPU {np.median(cpu):10.2f} ms "
                             f"({min(cpu):.2f} .. {max(cpu):.2f})   device calls {stats['calls_completed'] // 4}, draws per batch {stats['draws'] // 4}, "
                             f"subsets per batch {stats['subsets'] // 4}")
            lines.append("")
    finally:
        engine.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
