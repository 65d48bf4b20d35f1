#!/usr/bin/env python3
"""The estimates table (rpvg_amd/csrc/estimates_table.hip) on the estimates of a `haplotype-transcripts` run, next to the host loops
it takes over.

The shapes (all of them in one invocation; the file is written anew): x<scale>, synth.generate at the configs[2] shape (5 000
clusters, 200 000 paths) times the scale; fragments, the batch a run from fragments prepares (tools/path_table_ab.py's stream and
table: tens of thousands of clusters); limits, synthetic clusters at each route's limit and just beyond it.  Measured, wall
time around calls that wait for the device:
  device   rpvg_hip_estimates_table_build from host arrays (upload, kernels) and from device arrays (kernels only),
           rpvg_hip_estimates_table_tpm, rpvg_hip_estimates_table_view (the one packed download); the kernels' own time is the
           context's build span (HIP events around them);
  host     totalTranscriptCount alone; a writer's addEstimates() from the containers against addTable() from the table, both to
           a file (rpvg_amd_estimates_write_from_containers, rpvg_amd_estimates_table_write);
  verdicts the table against the plain-Python model byte for byte, the files against each other, the total against the single chain.

    python tools/estimates_table_ab.py [--shapes x1,x0.05,fragments,limits] [--repeats R] [--out profiles/estimates_table/ab.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/estimates_table_ab.py --shapes fragments --out /dev/null
    python tools/estimates_table_ab.py --kernel-stats "label=DIR/.../..._kernel_stats.csv" ...   (profiles/estimates_table/kernel_trace.txt)
    python tools/estimates_table_ab.py --resources [profiles/estimates_table/resource_usage.txt]    (cross-compiles; needs no GPU)
"""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _resources import resource_usage  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))


def ms(f, repeats):
    out, result = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        result = f()
        out.append(1e3 * (time.perf_counter() - t0))
    return out, result


def fmt(values):
    return " ".join(f"{v:9.3f}" for v in values)


class BatchArrays:
    """What FlatEstimates.from_estimates and the model read of a batch."""
    def __init__(self, cluster_path_off, path_effective_length):
        self.cluster_path_off = np.ascontiguousarray(cluster_path_off, dtype=np.uint64)
        self.path_effective_length = np.ascontiguousarray(path_effective_length, dtype=np.float64)


def device_flat(ctx, flat):
    pointers = {}
    for name in ("set_off", "member_off", "members", "posteriors", "abund_off", "abundances", "noise_count", "cluster_path_off",
                 "path_effective_length"):
        a = getattr(flat, name)
        pointers[name] = ctx.malloc(max(a.nbytes, 8))
        if a.nbytes:
            ctx.h2d(pointers[name], a)
    return pointers, flat.as_c(device_pointers=pointers)


def run_estimates_shape(e, kind, scale, R, chunk):
    """One block of lines for the estimates of a haplotype-transcripts run; kind: "synth" or "fragments"."""
    from rpvg_amd import hip, synth
    from rpvg_amd.batch import make_params
    from rpvg_amd.estimates_table import EstimatesTable, FlatEstimates, HarnessTable, limits, write_from_containers
    from tests import estimates_table_model as M

    K = max(8, int(round(5000 * scale)))
    P = max(K, int(round(200000 * scale)))
    reads = int(round(10000000 * scale))
    params = make_params()
    ok = True
    if kind == "fragments":
        from align_index_ab import stream_chunks
        from rpvg_amd.index import IndexParams, PathTable
        batch, al = synth.generate_with_alignments(seed=3, num_clusters=K, total_paths=P, total_reads=reads)
        chunks = stream_chunks(batch, al, 17, chunk)
        lengths = np.maximum(1, np.round(batch.path_effective_length)).astype(np.uint32) + 300
        table = PathTable(batch.path_group_id, np.maximum(batch.path_source_count, 1), lengths, batch.path_effective_length,
                          batch.path_source_off, batch.source_id, None)
        max_frag = max(int(c.align_frag_length[c.list_align_off[:-1].astype(np.int64)].max()) for c in chunks)
        prepared = e.prepare_from_fragments(chunks, IndexParams(num_paths=P, max_frag_length=max_frag, pre_frag_loc=300), path_table=table)
        what = f"from-fragments index of the configs[2] shape x {scale}"
        arrays = BatchArrays(prepared.cluster_path_off, np.asarray(batch.path_effective_length)[prepared.cluster_paths])
    else:
        batch = synth.generate(seed=3, num_clusters=K, total_paths=P, total_reads=reads)
        prepared = e.prepare(batch)
        what = f"configs[2] shape x {scale}"
        arrays = BatchArrays(batch.cluster_path_off, batch.path_effective_length)
    estimates, seconds = e.run("haplotype-transcripts", params, prepared)
    sets = sum(len(x.path_group_sets) for x in estimates)
    members = sum(len(s) for x in estimates for s in x.path_group_sets)
    lines = [f"estimates table, {what}: {len(estimates)} clusters, {P} paths, {sets} sets, {members} members (haplotype-transcripts, "
             f"estimate {1e3 * seconds:.1f} ms); times in ms, {R} runs each", "device: " + e.info()[0]]
    lim = limits()
    lines.append(f"limits: wavefront {lim.wave_paths} paths / {lim.wave_members} members ({lim.wave_lds_bytes} B of LDS), workgroup {lim.lds_paths} / "
                 f"{lim.lds_members} ({lim.lds_bytes} B)")

    # through the host class: flattening of the containers + the ABI
    made = []
    times, harness = ms(lambda: made.append(HarnessTable(e, prepared, params.ploidy)) or made[-1], R)
    lines.append(f"EstimatesTable from the containers (flatten + build)  {fmt(times)}")
    view = harness.view()
    lines.append(f"clusters by route (wavefront, workgroup, global)      {view['clusters_by_route']}")
    total = view["total_transcript_count"]
    times, _ = ms(lambda: harness.tpm(total), R)
    lines.append(f"tpm step (kernel + wait)                              {fmt(times)}")
    times, view = ms(lambda: harness.tpm(total) or harness.view(), R)
    lines.append(f"tpm step + view (one packed download)                 {fmt(times)}")

    flat = FlatEstimates.from_estimates(arrays, estimates)
    c_flat = flat.as_c()
    e.reset_stats()
    tables = []
    times, _ = ms(lambda: tables.append(EstimatesTable.build_flat(e, c_flat, params.ploidy)), R)
    stats = e.stats()
    lines.append(f"rpvg_hip_estimates_table_build, host arrays           {fmt(times)}")
    lines.append(f"  of which kernels (HIP events, mean of the runs)     {stats['build_ms'] / R:9.3f}   copies {stats['h2d_ms'] / R:9.3f}   "
                 f"({stats['h2d_bytes'] / R / 1e6:.1f} MB)")
    ctx = hip.Context(0)
    try:
        pointers, d_flat = device_flat(ctx, flat)
        times, dev_table = ms(lambda: tables.append(EstimatesTable.build_flat(ctx, d_flat, params.ploidy)) or tables[-1], R + 1)
        lines.append(f"rpvg_hip_estimates_table_build, device arrays         {fmt(times[1:])}")
        times, dev_view = ms(dev_table.view, 1)
        lines.append(f"rpvg_hip_estimates_table_view (first: the download)   {fmt(times)}")
        t0 = time.perf_counter()
        clusters = M.from_estimates(arrays, estimates)
        want = M.table(clusters, params.ploidy)
        model_ms = 1e3 * (time.perf_counter() - t0)
        names = ("haplotype_prob", "read_count", "transcript_count", "member_transcript_count", "cluster_transcript_count")
        same = all(dev_view[n].tobytes() == want[n].tobytes() and view[n].tobytes() == want[n].tobytes() for n in names)
        same = same and all(dev_view[n] == want[n] == view[n] for n in ("total_transcript_count", "noise_count_total", "noise_count_share_total"))
        with_tpm = M.with_tpm(want, total)
        same_tpm = all(view[n].tobytes() == with_tpm[n].tobytes() for n in ("tpm", "member_tpm"))
        lines.append(f"table equals the plain-Python model byte for byte (host and device arrays): {same}   TPMs: {same_tpm}   (model: {model_ms:.0f} ms)")
        ok = ok and same and same_tpm
        for t in tables:
            t.free()
        for p in pointers.values():
            ctx.free(p)
    finally:
        ctx.close()

    # the host loops of the parent commit
    singles = [write_from_containers(prepared, "", params.ploidy, "") for _ in range(R)]
    single = singles[0][0]
    n = sum(1 for x in view["member_transcript_count"] if x > 0)
    lines.append(f"host: totalTranscriptCount (one thread)               {fmt([1e3 * s[1] for s in singles])}")
    bound = 2 * max(n - 1, 0) * 2.0 ** -53 * single
    within = abs(total - single) <= bound
    lines.append(f"total_transcript_count {total!r} against the single chain {single!r}: difference {abs(total - single):.3e} within "
                 f"2 (n - 1) 2^-53 = {bound:.3e} (n = {n}): {within}")
    ok = ok and within
    with tempfile.TemporaryDirectory() as tmp:
        for writer in ("haplotype", "joint"):
            a, b = os.path.join(tmp, "containers_" + writer), os.path.join(tmp, "table_" + writer)
            t_est = [1e3 * write_from_containers(prepared, writer, params.ploidy, a, denominator=total, min_posterior=params.prob_precision)[2]
                     for _ in range(R)]
            t_tab, _ = ms(lambda: harness.write(writer, b, params.prob_precision), R)
            suffix = "_joint.txt" if writer == "joint" else ".txt"
            same = open(a + suffix, "rb").read() == open(b + suffix, "rb").read()
            size = os.path.getsize(a + suffix)
            lines.append(f"host: {writer:<9} addEstimates -> file                 {fmt(t_est)}")
            lines.append(f"      {writer:<9} addTable -> file                     {fmt(t_tab)}   files equal: {same} ({size} bytes)")
            ok = ok and same
    for h in made:
        h.free()
    prepared.free()
    return lines, ok


def synthetic_flat(rng, clusters, paths, members):
    """`clusters` clusters of `paths` paths and `members` members each: sorted sets of two (the last of one when members is odd),
    one abundance per member, random doubles."""
    from rpvg_amd.estimates_table import FlatEstimates
    sizes = np.full((members + 1) // 2, 2, dtype=np.uint64)
    if members % 2:
        sizes[-1] = 1
    sets = len(sizes)
    pairs = np.sort(rng.integers(0, paths, size=(clusters, sets, 2), dtype=np.uint32), axis=2).reshape(clusters, -1)[:, :members]
    member_off = np.concatenate([[0], np.cumsum(np.tile(sizes, clusters))]).astype(np.uint64)
    return FlatEstimates(np.arange(clusters + 1, dtype=np.uint64) * sets, member_off, pairs.reshape(-1), rng.uniform(0.0, 1.0, size=clusters * sets),
                         np.arange(clusters + 1, dtype=np.uint64) * members, rng.uniform(0.0, 500.0, size=clusters * members),
                         rng.uniform(0.0, 40.0, size=clusters), np.arange(clusters + 1, dtype=np.uint64) * paths,
                         rng.uniform(50.0, 8000.0, size=clusters * paths))


def run_limits_shape(R):
    """The routes either side of each limit: the same number of clusters at the limit of a route and one path and one member beyond it
    (device arrays: kernels and the waits of the call, no copy in)."""
    from rpvg_amd import hip
    from rpvg_amd.estimates_table import EstimatesTable, limits
    lim = limits()
    lines = [f"routes either side of the limits: build from device arrays, times in ms, {R} runs each (after one that is not listed)"]
    rng = np.random.default_rng(41)
    ctx = hip.Context(0)
    try:
        lines.append("device: " + ctx.info()[0])
        for label, clusters, paths, members in (("at the wavefront limit", 2048, lim.wave_paths, lim.wave_members),
                                                ("beyond it (workgroup route)", 2048, lim.wave_paths + 1, lim.wave_members + 1),
                                                ("a quarter of the workgroup limit", 256, lim.lds_paths // 4, lim.lds_members // 4),
                                                ("at the workgroup limit", 64, lim.lds_paths, lim.lds_members),
                                                ("beyond it (global route)", 64, lim.lds_paths + 1, lim.lds_members + 1)):
            flat = synthetic_flat(rng, clusters, paths, members)
            pointers, d_flat = device_flat(ctx, flat)
            tables = []
            times, table = ms(lambda: tables.append(EstimatesTable.build_flat(ctx, d_flat, 2)) or tables[-1], R + 1)
            routes = table.view()["clusters_by_route"]
            lines.append(f"{clusters:5d} clusters of {paths:5d} paths, {members:5d} members, {label:<33} {fmt(times[1:])}   routes {routes}")
            for t in tables:
                t.free()
            for p in pointers.values():
                ctx.free(p)
    finally:
        ctx.close()
    return lines, True


def kernel_stats(out, labelled):
    """rocprofv3 --kernel-trace --stats runs of this tool (one shape each: label=kernel_stats.csv) as the kernels' own lines."""
    import csv
    lines = ["estimates_table.hip: the kernels' own time, rocprofv3 --kernel-trace --stats around one shape of tools/estimates_table_ab.py each",
             "(every call of the shape: builds from the containers, from host and from device arrays; hipcub's kernels of the global route listed too)"]
    for item in labelled:
        label, path = item.split("=", 1)
        lines.append("")
        lines.append(label)
        lines.append(f"{'kernel':<46}{'calls':>7}{'avg us':>10}{'min us':>10}{'max us':>10}{'total ms':>10}")
        rows = []
        for r in csv.DictReader(open(path)):
            name = r["Name"].replace("(anonymous namespace)::", "")
            ours = any(k in name for k in ("describeKernel", "residentKernel", "globalPathsKernel", "globalClustersKernel", "totalsKernel", "tpmKernel"))
            if not ours and "radix_sort" not in name and "onesweep" not in name:
                continue
            short = re.sub(r"^void ", "", name).split("(")[0] if ours else "hipcub radix sort: " + re.sub(r"^.*?(\w*(radix_sort|onesweep)\w*).*$", r"\1", name)[:26]
            rows.append((short, r))
        for short, r in sorted(rows, key=lambda x: -float(x[1]["TotalDurationNs"])):
            lines.append(f"{short[:45]:<46}{r['Calls']:>7}{float(r['AverageNs']) / 1e3:10.1f}{float(r['MinNs']) / 1e3:10.1f}{float(r['MaxNs']) / 1e3:10.1f}"
                         f"{float(r['TotalDurationNs']) / 1e6:10.3f}")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="x1,x0.05,fragments,limits", help="comma separated: x<scale>, fragments, limits")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimates_table", "ab.txt"))
    ap.add_argument("--resources", nargs="?", const=os.path.join(ROOT, "profiles", "estimates_table", "resource_usage.txt"), default=None)
    ap.add_argument("--kernel-stats", nargs="+", default=None, metavar="LABEL=CSV")
    ap.add_argument("--kernel-stats-out", default=os.path.join(ROOT, "profiles", "estimates_table", "kernel_trace.txt"))
    args = ap.parse_args()
    if args.resources:
        resource_usage("estimates_table.hip", args.resources, width=44, header_note=" (hipcub's own kernels left out)")
        return 0
    if args.kernel_stats:
        kernel_stats(args.kernel_stats_out, args.kernel_stats)
        return 0

    from rpvg_amd import engine as eng_mod
    blocks, ok = [], True
    for shape in args.shapes.split(","):
        if shape == "limits":
            lines, good = run_limits_shape(args.repeats)
        else:
            e = eng_mod.Engine(0)
            try:
                if shape == "fragments":
                    lines, good = run_estimates_shape(e, "fragments", 1.0, args.repeats, args.chunk)
                else:
                    lines, good = run_estimates_shape(e, "synth", float(shape.lstrip("x")), args.repeats, args.chunk)
            finally:
                e.close()
        print("\n".join(lines) + "\n", flush=True)
        blocks.append("\n".join(lines) + "\n")
        ok = ok and good
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(blocks))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
