#!/usr/bin/env python3
"""The path table (rpvg_amd/csrc/path_table.hip) on the configs[2] shape, next to a one-thread host line.

The paths of synth.generate_with_alignments (200 000 paths, their haplotype ids) become the table by global path id; names are
drawn so that the paths per name follow the quantiles of tests/golden/info_example_pantranscriptome.json (hsts_per_transcript) and
are shuffled inside every cluster, so that first appearances interleave.  The reads, expanded into a stream of per-fragment lists
(tools/align_index_ab.py), give the index.  Measured, wall time around calls that wait for the device:
  device   rpvg_hip_path_table_upload; rpvg_hip_read_rows_to_batch_with_paths against rpvg_hip_read_rows_to_batch;
           rpvg_hip_align_index_name_groups;
  host     rpvg_amd_path_table_host_line: one thread, std::unordered_map<std::string, uint32_t> — group_name_index and the collapsed
           paths (src/main.cpp:853-887,909-951); its result is compared with the device's at full size;
  run      `haplotype-transcripts` from fragments with the table and without it (the route before the table: host-built groups).

    python tools/path_table_ab.py [--scale F] [--repeats R] [--out profiles/path_table/ab.txt]
    python tools/path_table_ab.py --resources [profiles/path_table/resource_usage.txt]    (cross-compiles; needs no GPU)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _resources import resource_usage  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))


def draw_names(rng, cluster_path_off, quantiles):
    """name ids by global path: runs of paths share a name, run lengths follow the fixture's quantiles (p50, p90, p99, max), a
    run ends with its cluster, and the paths of a cluster are shuffled; the ids are sparse and unordered."""
    P = int(cluster_path_off[-1])
    edges = [1, int(quantiles["p50"]), int(quantiles["p90"]), int(quantiles["p99"]), int(quantiles["max"])]
    names = np.zeros(P, dtype=np.uint32)
    next_name = 0
    for k in range(len(cluster_path_off) - 1):
        p0, p1 = int(cluster_path_off[k]), int(cluster_path_off[k + 1])
        run_names, p = [], p0
        while p < p1:
            u = rng.random()
            band = 0 if u < 0.5 else 1 if u < 0.9 else 2 if u < 0.99 else 3
            n = min(int(rng.integers(edges[band], edges[band + 1] + 1)), p1 - p)
            run_names += [next_name] * n
            next_name += 1
            p += n
        names[p0:p1] = rng.permutation(np.asarray(run_names, dtype=np.uint32))
    sparse = rng.choice(np.arange(1, 2 ** 32 - 1, 4099, dtype=np.uint64), size=next_name, replace=False).astype(np.uint32)
    return sparse[names], next_name


def ms(f, repeats):
    out, result = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        result = f()
        out.append(1e3 * (time.perf_counter() - t0))
    return out, result


def fmt(values):
    return " ".join(f"{v:9.3f}" for v in values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_table", "ab.txt"))
    ap.add_argument("--resources", nargs="?", const=os.path.join(ROOT, "profiles", "path_table", "resource_usage.txt"), default=None)
    args = ap.parse_args()
    if args.resources:
        resource_usage("path_table.hip", args.resources, header_note=" (hipcub's own kernels left out)")
        return 0

    from align_index_ab import stream_chunks
    from rpvg_amd import engine as eng_mod, hip, synth
    from rpvg_amd.batch import make_params
    from rpvg_amd.index import AlignmentIndex, DevicePathTable, IndexParams, PathTable, CPathTable
    from rpvg_amd.rows import RowParams

    K = max(8, int(round(5000 * args.scale)))
    P = max(K, int(round(200000 * args.scale)))
    batch, al = synth.generate_with_alignments(seed=3, num_clusters=K, total_paths=P, total_reads=int(round(10000000 * args.scale)))
    chunks = stream_chunks(batch, al, 17, args.chunk)
    with open(os.path.join(ROOT, "tests", "golden", "info_example_pantranscriptome.json")) as f:
        quantiles = json.load(f)["hsts_per_transcript"]
    rng = np.random.default_rng(23)
    name_id, num_names = draw_names(rng, batch.cluster_path_off, quantiles)
    lengths = np.maximum(1, np.round(batch.path_effective_length)).astype(np.uint32) + 300
    table = PathTable(batch.path_group_id, np.maximum(batch.path_source_count, 1), lengths, batch.path_effective_length, batch.path_source_off,
                      batch.source_id, name_id)
    max_frag = max(int(c.align_frag_length[c.list_align_off[:-1].astype(np.int64)].max()) for c in chunks)
    params = IndexParams(num_paths=P, max_frag_length=max_frag, pre_frag_loc=300)
    lines = [f"path table, configs[2] shape x {args.scale}: {P} paths, {len(batch.source_id)} source incidences, {num_names} names, "
             f"{sum(c.num_lists for c in chunks)} lists; times in ms, {args.repeats} runs each"]
    v = np.arange(65536, dtype=np.float64)
    row_params = RowParams(frag_length_log_prob=-0.5 * ((v - 300.0) / 50.0) ** 2 - np.log(50.0 * np.sqrt(2 * np.pi)))

    ctx = hip.Context(0)
    same = False
    try:
        lines.append("device: " + ctx.info()[0])
        index = AlignmentIndex(ctx, params)
        for c in chunks:
            index.add(c)
        info = index.finish()
        lines.append(f"index: {info.num_distinct} distinct lists, {info.num_clusters} clusters")
        uploads = []
        times, dev = ms(lambda: uploads.append(DevicePathTable(ctx, table)) or uploads[-1], args.repeats)
        lines.append(f"table upload                          {fmt(times)}")
        alignments = index.alignments(batch.path_effective_length)
        rows = alignments.build_rows(row_params)
        made = []
        times, _ = ms(lambda: made.append(rows.to_batch()), args.repeats)
        lines.append(f"rows to batch, no path side           {fmt(times)}")
        times, with_paths = ms(lambda: made.append(rows.to_batch(index, dev)) or made[-1], args.repeats)
        lines.append(f"rows to batch with paths              {fmt(times)}   has_source_columns {with_paths.has_source_columns()}")
        for b in made:
            b.free()
        formed = []
        times, groups = ms(lambda: formed.append(index.name_groups(dev)) or formed[-1], args.repeats)
        lines.append(f"name groups + collapsed paths         {fmt(times)}")
        got = groups.view()
        view = index.view()

        L = eng_mod.lib()
        L.rpvg_amd_path_table_host_line.argtypes = [C.POINTER(CPathTable), C.c_uint32] + [C.c_void_p] * 8
        ct = table.as_c()
        Kc = info.num_clusters
        cpo = np.ascontiguousarray(view.batch.cluster_path_off, dtype=np.uint64)
        cpaths = np.ascontiguousarray(view.cluster_paths, dtype=np.uint32)
        pg, cgo = np.zeros(P, dtype=np.uint32), np.zeros(Kc + 1, dtype=np.uint64)
        gsc, glen, geff = np.zeros(P, dtype=np.uint32), np.zeros(P, dtype=np.uint32), np.zeros(P, dtype=np.float64)
        secs = C.c_double(0)
        host_ms = []
        for _ in range(args.repeats):
            rc = L.rpvg_amd_path_table_host_line(C.byref(ct), Kc, cpo.ctypes.data, cpaths.ctypes.data, pg.ctypes.data, cgo.ctypes.data,
                                                 gsc.ctypes.data, glen.ctypes.data, geff.ctypes.data, C.addressof(secs))
            assert rc == 0
            host_ms.append(1e3 * secs.value)
        lines.append(f"host line (one thread, unordered_map) {fmt(host_ms)}")
        G = int(cgo[-1])
        same = (np.array_equal(pg, got["path_group"]) and np.array_equal(cgo, got["cluster_group_off"]) and
                np.array_equal(gsc[:G], got["group_source_count"]) and np.array_equal(glen[:G], got["group_length"]) and
                geff[:G].tobytes() == got["group_effective_length"].tobytes())
        lines.append(f"device groups equal the host line (groups, offsets, counts, lengths; effective lengths byte for byte): {same}   {G} groups")
        for g in formed:
            g.free()
        for d in uploads:
            d.free()
        rows.free()
        alignments.free()
        index.free()
    finally:
        ctx.close()

    e = eng_mod.Engine(0)
    try:
        for label, kw in (("without the table (host-built groups)", dict(path_info=batch)), ("with the table", dict(path_table=table))):
            prep = e.prepare_from_fragments(chunks, params, **kw)
            runs = [1e3 * e.run_raw("haplotype-transcripts", make_params(), prep) for _ in range(args.repeats + 1)][1:]
            lines.append(f"haplotype-transcripts from fragments, {label}: prepare {1e3 * prep.row_construction_seconds:9.2f}   estimate {fmt(runs)}"
                         f"   has_source_columns {prep.has_source_columns}")
            prep.free()
    finally:
        e.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
