#!/usr/bin/env python3
"""The Gibbs samples table (rpvg_amd/csrc/gibbs_table.hip) on the samples of a run with -n, next to the writer's host loops it takes
over.

Shapes (all of them in one invocation; the file is written after every block): x<scale>, synth.generate at the configs[2] shape
(5 000 clusters, 200 000 paths) times the scale, estimated with `-i haplotype-transcripts`; transcripts, the same batch at scale 1
with `-i transcripts` (one block of all paths per cluster).  Every shape at every N of --n.  The sampler runs with
--gibbs-thin-its 1: the table does not care how far apart the recorded states are, and the run stays short.  Measured, wall time
around calls that wait for the device, R runs each after one that is not listed:
  build from the containers (flatten on the host + rpvg_hip_gibbs_table_build from host arrays), from host arrays alone, from
  device arrays; the kernels' own time is the context's build span (HIP events around them); the view's download; the clusters
  per route; the writer's loops on ONE host thread with stores into a dense table instead of stream insertions
  (rpvg_amd_gibbs_from_containers), which must equal the device's table byte for byte before any time is written.
  transcripts only: rpvg_hip_gibbs_read_counts against rpvg_hip_gibbs_read_counts_resident on the EM problems of the clusters (one
  problem of all paths per cluster), and the build from the resident handle against the build from the downloaded arrays.
Bandwidth: the algorithmic bytes 8 (abundance samples + noise samples + P N) + P over the kernels' time, as a fraction of the HBM
peak docs/design/measurement.md uses.

    python tools/gibbs_table_ab.py [--shapes x0.05,x1,transcripts] [--n 100,1000] [--repeats R] [--out profiles/gibbs_table/ab.txt]
    python tools/gibbs_table_ab.py --resources [profiles/gibbs_table/resource_usage.txt]    (cross-compiles; needs no GPU)
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _resources import resource_usage  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second: docs/design/measurement.md


def ms(f, repeats):
    out, result = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        result = f()
        out.append(1e3 * (time.perf_counter() - t0))
    return out, result


def fmt(values):
    return " ".join(f"{v:9.3f}" for v in values)


def flat_of_result(e, prepared, model, params, cluster_path_off, N):
    """The run's result as a FlatGibbs, its arrays copied out of the result view as they lie (no Python lists)."""
    from rpvg_amd import engine as eng_mod, hip
    from rpvg_amd.batch import CEstimatesView
    from rpvg_amd.gibbs_table import FlatGibbs
    secs = C.c_double(0)
    h = eng_mod.lib().rpvg_amd_run(e.handle, prepared.handle, model.encode(), C.byref(params), C.byref(secs))
    if not h:
        raise hip.EngineError(f"run({model}) failed: {eng_mod._err()}")
    try:
        v = CEstimatesView()
        eng_mod.lib().rpvg_amd_result_view(h, C.byref(v))
        K = int(v.num_clusters)

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)

        goff = arr(v.gibbs_off, K + 1, np.uint64)
        B = int(goff[-1])
        poff, noff, aoff = (arr(p, B + 1, np.uint64) if B else np.zeros(1, np.uint64) for p in (v.gibbs_path_off, v.gibbs_noise_off, v.gibbs_abund_off))
        flat = FlatGibbs(goff, poff, arr(v.gibbs_path, int(poff[-1]), np.uint32), noff, arr(v.gibbs_noise, int(noff[-1]), np.float64), aoff,
                         arr(v.gibbs_abund, int(aoff[-1]), np.float64), cluster_path_off, arr(v.total_count, K, np.float64), N)
    finally:
        eng_mod.lib().rpvg_amd_result_free(h)
    return flat, secs.value


def device_flat(ctx, flat):
    pointers = {}
    for name in ("gibbs_off", "gibbs_path_off", "gibbs_path", "gibbs_noise_off", "gibbs_noise", "gibbs_abund_off", "gibbs_abund",
                 "cluster_path_off", "total_count"):
        a = getattr(flat, name)
        pointers[name] = ctx.malloc(max(a.nbytes, 8))
        if a.nbytes:
            ctx.h2d(pointers[name], a)
    return pointers, flat.as_c(device_pointers=pointers)


def same_table(a, b):
    return all(a[n].tobytes() == b[n].tobytes() for n in ("samples", "listed", "noise_counts"))


def run_shape(shape, N, R):
    from rpvg_amd import engine as eng_mod, hip, synth
    from rpvg_amd.batch import make_params
    from rpvg_amd.gibbs_table import GibbsSamples, GibbsTable, HarnessGibbsTable, from_containers, limits

    model = "transcripts" if shape == "transcripts" else "haplotype-transcripts"
    scale = 1.0 if shape == "transcripts" else float(shape.lstrip("x"))
    K = max(8, int(round(5000 * scale)))
    P = max(K, int(round(200000 * scale)))
    batch = synth.generate(seed=3, num_clusters=K, total_paths=P, total_reads=int(round(10000000 * scale)))
    params = make_params(num_gibbs_samples=N, gibbs_thin_its=1)
    lim = limits()
    ok = True
    e = eng_mod.Engine(0)
    try:
        prepared = e.prepare(batch)
        flat, seconds = flat_of_result(e, prepared, model, params, batch.cluster_path_off, N)
        sizes = flat.sizes()
        alg_bytes = 8 * (sizes["num_abundance_samples"] + sizes["num_noise_samples"] + P * N) + P
        lines = [f"gibbs samples table, configs[2] shape x {scale}, -i {model}, -n {N} (--gibbs-thin-its 1): {K} clusters, {P} paths, "
                 f"{sizes['num_blocks']} blocks, {sizes['num_abundance_samples']} abundance samples (estimate {1e3 * seconds:.0f} ms); "
                 f"algorithmic bytes {alg_bytes / 1e6:.1f} MB; times in ms, {R} runs each after one that is not listed",
                 "device: " + e.info()[0],
                 f"limits: resident {lim.resident_paths} paths / {lim.resident_columns} columns ({lim.resident_lds_bytes} B of LDS), sample tile "
                 f"{lim.sample_tile}, global {lim.global_paths} paths per workgroup"]
        made = []
        times, harness = ms(lambda: made.append(HarnessGibbsTable(e, prepared, N)) or made[-1], R + 1)
        lines.append(f"GibbsSamplesTable from the containers (flatten + build)  {fmt(times[1:])}")
        c_flat = flat.as_c()
        tables = []
        ms(lambda: tables.append(GibbsTable.build_flat(e, c_flat)), 1)
        e.reset_stats()
        times, _ = ms(lambda: tables.append(GibbsTable.build_flat(e, c_flat)), R)
        stats = e.stats()
        kernel_ms = stats["build_ms"] / R
        lines.append(f"rpvg_hip_gibbs_table_build, host arrays                  {fmt(times)}")
        lines.append(f"  of which kernels (HIP events, mean of the runs)        {kernel_ms:9.3f}   copies {stats['h2d_ms'] / R:9.3f}   "
                     f"({stats['h2d_bytes'] / R / 1e6:.1f} MB)")
        for t in tables[:-1]:
            t.free()
        tables = tables[-1:]
        ctx = hip.Context(0)
        try:
            pointers, d_flat = device_flat(ctx, flat)
            ctx.reset_stats()
            times, dev_table = ms(lambda: tables.append(GibbsTable.build_flat(ctx, d_flat)) or tables[-1], R + 1)
            dev_kernel_ms = ctx.stats()["build_ms"] / (R + 1)
            lines.append(f"rpvg_hip_gibbs_table_build, device arrays                {fmt(times[1:])}")
            lines.append(f"  of which kernels (HIP events, mean of the runs)        {dev_kernel_ms:9.3f}   = {alg_bytes / (dev_kernel_ms * 1e-3) / 1e9:.0f} GB/s, "
                         f"{alg_bytes / (dev_kernel_ms * 1e-3) / HBM_PEAK:.2f} of the HBM peak")
            times, dev_view = ms(dev_table.view, 1)
            lines.append(f"rpvg_hip_gibbs_table_view (the download, {8 * P * N / 1e6:.0f} MB)          {fmt(times)}")
            lines.append(f"clusters by route (resident, global)                     {dev_view['clusters_by_route']}")
            host = from_containers(prepared, N, P)
            host_times = [1e3 * from_containers(prepared, N, P)["seconds"] for _ in range(R)]
            same = same_table(dev_view, host) and same_table(harness.view(), host) and same_table(tables[0].view(), host)
            ok = ok and same
            lines.append(f"table equals the writer's loops byte for byte (containers, host and device arrays): {same}")
            if same:
                lines.append(f"host: the writer's loops into a dense table (one thread)  {fmt(host_times)}")
            for t in tables:
                t.free()
            for p in pointers.values():
                ctx.free(p)
            if shape == "transcripts":
                ks = list(range(K))
                cols = [list(range(int(batch.cluster_path_off[k + 1] - batch.cluster_path_off[k]))) for k in ks]
                dev = ctx.upload(batch)
                abund, noise, total, _ = ctx.em_solve(dev, ks, cols)
                n, seeds = [N] * K, list(range(1, K + 1))
                t_down, got = ms(lambda: ctx.gibbs_read_counts(dev, ks, cols, abund, noise, n, seeds, 1), R + 1)
                handles = []
                t_res, handle = ms(lambda: handles.append(GibbsSamples.draw(ctx, dev, ks, cols, abund, noise, n, seeds, 1)) or handles[-1], R + 1)
                lines.append(f"rpvg_hip_gibbs_read_counts (with its downloads)          {fmt(t_down[1:])}")
                lines.append(f"rpvg_hip_gibbs_read_counts_resident                      {fmt(t_res[1:])}")
                for h in handles[:-1]:
                    h.free()
                resident = []
                t_build, table = ms(lambda: resident.append(GibbsTable.build_resident(ctx, handle, batch.cluster_path_off, total, N)) or resident[-1], R + 1)
                lines.append(f"rpvg_hip_gibbs_table_build_resident                      {fmt(t_build[1:])}")
                from rpvg_amd.gibbs_table import FlatGibbs
                widths = np.array([len(c) for c in cols], dtype=np.uint64)
                arrays = FlatGibbs(np.arange(K + 1, dtype=np.uint64), np.concatenate([[0], np.cumsum(widths)]), np.concatenate([np.arange(w, dtype=np.uint32) for w in widths]),
                                   np.arange(K + 1, dtype=np.uint64) * N, np.concatenate([g[0] for g in got]), np.concatenate([[0], np.cumsum(widths * N)]),
                                   np.concatenate([g[1].reshape(-1) for g in got]), batch.cluster_path_off, total, N)
                t_arrays, from_arrays = ms(lambda: resident.append(GibbsTable.build(ctx, arrays)) or resident[-1], R + 1)
                lines.append(f"rpvg_hip_gibbs_table_build from the downloaded arrays    {fmt(t_arrays[1:])}")
                same = same_table(table.view(), from_arrays.view())
                ok = ok and same
                lines.append(f"the table of the handle equals the table of the arrays byte for byte: {same}")
                for t in resident:
                    t.free()
                handle.free()
                dev.free()
        finally:
            ctx.close()
        for h in made:
            h.free()
        prepared.free()
    finally:
        e.close()
    return lines, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="x0.05,x1,transcripts", help="comma separated: x<scale>, transcripts")
    ap.add_argument("--n", default="100,1000", help="comma separated numbers of Gibbs samples")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gibbs_table", "ab.txt"))
    ap.add_argument("--resources", nargs="?", const=os.path.join(ROOT, "profiles", "gibbs_table", "resource_usage.txt"), default=None)
    args = ap.parse_args()
    if args.resources:
        resource_usage("gibbs_table.hip", args.resources, width=44)
        return 0
    blocks, ok = [], True
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for N in (int(x) for x in args.n.split(",")):
        for shape in args.shapes.split(","):
            lines, good = run_shape(shape, N, args.repeats)
            print("\n".join(lines) + "\n", flush=True)
            blocks.append("\n".join(lines) + "\n")
            ok = ok and good
            with open(args.out, "w") as f:
                f.write("\n".join(blocks))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
