#!/usr/bin/env python3
"""The resident estimates route (rpvg_amd/csrc/estimates_gather.hip) next to the container route it takes over, on the estimates of a
`haplotype-transcripts` run at the configs[2] shape (5 000 clusters, 200 000 paths) and at a twentieth of it.  Wall time around
calls that wait for the device, one warm-up and R runs each:

  (a) container route   estimateBatch into the C++ containers (Engine.run_raw: device call, download of the packed block,
                        unpackMerged*), then EstimatesTable from the
                        containers (flatten + build: the figure docs/design/kernels-rows-clusters.md records for the table);
  (b) resident route    run_resident (device call with the block kept, gather), then the table from the resident estimates;
  gather alone          rpvg_hip_flat_estimates_gather on one hand-made device part that holds the run's own sets (width 2), with
                        the context's build span around its launches (HIP events from the describe launch to the scatter launch: it
                        includes the wait for the offender word and S, M in between) and the bytes the call uploads;
  kept blocks           the device memory the kept block of every lane's nested call holds (the calls' capacities);
  bytes over PCIe       the flat arrays the container route uploads for its table against what the gather uploads.

    python tools/resident_estimates_ab.py [--shapes x1,x0.05] [--repeats 3] [--out profiles/resident_estimates/ab.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ms(f, repeats, warm=1):
    out, result = [], None
    for i in range(repeats + warm):
        t0 = time.perf_counter()
        result = f()
        if i >= warm:
            out.append(1e3 * (time.perf_counter() - t0))
    return out, result


def fmt(values):
    return " ".join(f"{v:9.3f}" for v in values)


def part_of_flat(flat):
    """One part of width 2 whose unit k is cluster k with one subset and its sets as slots (the sets of a diploid run have one or two
    members)."""
    K, S = len(flat.noise_count), len(flat.posteriors)
    sizes = np.diff(flat.member_off).astype(np.uint32)
    assert S == 0 or int(sizes.max()) <= 2
    member = np.full((S, 2), 0xFFFFFFFF, dtype=np.uint32)
    abundance = np.zeros((S, 2), dtype=np.float64)
    first = flat.member_off[:-1].astype(np.int64)
    member[:, 0], abundance[:, 0] = flat.members[first], flat.abundances[first]
    two = sizes == 2
    member[two, 1], abundance[two, 1] = flat.members[first[two] + 1], flat.abundances[first[two] + 1]
    return dict(width=2, unit_cluster=np.arange(K, dtype=np.uint32), subset_off=np.arange(K + 1, dtype=np.uint64),
                path_off=flat.set_off.astype(np.uint64), set_count=np.diff(flat.set_off).astype(np.uint32),
                cluster_noise_count=flat.noise_count, set_posterior=flat.posteriors, set_size=sizes, set_member=member, set_abundance=abundance)


def run_shape(e, scale, R):
    from rpvg_amd import hip, synth
    from rpvg_amd import resident_estimates as res
    from rpvg_amd.batch import make_params
    from rpvg_amd.estimates_table import FlatEstimates, HarnessTable

    K = max(8, int(round(5000 * scale)))
    P = max(K, int(round(200000 * scale)))
    batch = synth.generate(seed=3, num_clusters=K, total_paths=P, total_reads=int(round(10000000 * scale)))
    params = make_params()
    prepared = e.prepare(batch)
    lines = []
    try:
        estimates, _ = e.run("haplotype-transcripts", params, prepared)
        # (run_raw: the estimates stay in the C++ containers — no packing of a result, no decoding in Python inside the clock)
        times_run, _ = ms(lambda: e.run_raw("haplotype-transcripts", params, prepared), R)
        want = FlatEstimates.from_estimates(batch, estimates)
        lines.append(f"configs[2] shape x {scale}: {K} clusters, {P} paths, {len(want.posteriors)} sets, {len(want.members)} members; times in ms, "
                     f"one warm-up and {R} runs each;  device: {e.info()[0]}")
        made = []
        times_table, table = ms(lambda: made.append(HarnessTable(e, prepared, params.ploidy)) or made[-1], R)
        lines.append(f"(a) estimateBatch (device call + download + unpack)     {fmt(times_run)}")
        lines.append(f"(a) EstimatesTable from the containers (flatten + build) {fmt(times_table)}")
        kept = []
        times_res, resident = ms(lambda: kept.append(res.run_resident(e, "haplotype-transcripts", params, prepared)) or kept[-1], R)
        if resident is None:
            lines.append("(b) run_resident: NOT TAKEN")
            return lines
        made_res = []
        times_rtable, rtable = ms(lambda: made_res.append(resident.table(e, prepared, params.ploidy)) or made_res[-1], R)
        lines.append(f"(b) run_resident (device call, block kept + gather)     {fmt(times_res)}")
        lines.append(f"(b) EstimatesTable from the resident estimates (build)  {fmt(times_rtable)}")
        lines.append(f"    (a) - (b), medians: estimator call {np.median(times_run) - np.median(times_res):9.3f}   table "
                     f"{np.median(times_table) - np.median(times_rtable):9.3f}")
        kept_bytes = resident.kept_block_bytes()
        lines.append(f"kept device blocks, one per lane (bytes; the calls' capacities, not their results): {kept_bytes}")
        got = resident.get()
        same = all(getattr(got, n).tobytes() == getattr(want, n).tobytes() for n, _ in want._FIELDS)
        va, vb = table.view(), rtable.view()
        same_table = all(va[n].tobytes() == vb[n].tobytes() for n in ("haplotype_prob", "read_count", "transcript_count", "cluster_transcript_count"))
        lines.append(f"verdicts: flat arrays byte for byte {same}; tables byte for byte {same_table and va['total_transcript_count'] == vb['total_transcript_count']}")
        flat_bytes = sum(getattr(want, n).nbytes for n, _ in want._FIELDS)
        # the gather alone, on a device part that holds the run's own sets
        ctx = hip.Context(0)
        try:
            dev = ctx.upload(batch)
            part = part_of_flat(want)
            pointers = {}
            for name, dtype in res._PART_ARRAYS:
                if name in part:
                    a = np.ascontiguousarray(part[name], dtype=dtype)
                    pointers[name] = ctx.malloc(max(a.nbytes, 8))
                    if a.nbytes:
                        ctx.h2d(pointers[name], a)
            d_eff = ctx.malloc(max(want.path_effective_length.nbytes, 8))
            ctx.h2d(d_eff, want.path_effective_length)
            c_part = res.EstimatesPart.from_device(2, part["unit_cluster"], K, len(want.posteriors), **pointers)
            handles = []
            res.gather(ctx, dev, [c_part], d_eff, eff_on_device=True).free()  # warm-up
            ctx.reset_stats()
            times_g, est = ms(lambda: handles.append(res.gather(ctx, dev, [c_part], d_eff, eff_on_device=True)) or handles[-1], R, warm=0)
            stats = ctx.stats()
            again = est.get()
            same_g = all(getattr(again, n).tobytes() == getattr(want, n).tobytes() for n, _ in want._FIELDS)
            lines.append(f"rpvg_hip_flat_estimates_gather alone (device part)      {fmt(times_g)}")
            lines.append(f"  of which describe launch .. scatter launch (HIP events around the launches, the wait for the offender word and S, M "
                         f"included; mean of the runs) {stats['build_ms'] / R:9.3f}   byte for byte {same_g}")
            lines.append(f"bytes over PCIe for the table's input: container route uploads {flat_bytes / 1e6:.2f} MB of flat arrays (behind the download of "
                         f"the packed block); the gather uploads {stats['h2d_bytes'] / R / 1e6:.3f} MB (descriptors, unit_cluster, totals)")
            for h in handles:
                h.free()
            for pointer in list(pointers.values()) + [d_eff]:
                ctx.free(pointer)
            dev.free()
        finally:
            ctx.close()
        for t in made + made_res:
            t.free()
        for r in kept:
            if r is not None:
                r.free()
    finally:
        prepared.free()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="x1,x0.05")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_estimates", "ab.txt"))
    args = ap.parse_args()
    from rpvg_amd import engine as eng_mod
    e = eng_mod.Engine(0)
    lines = ["resident estimates against the container route (tools/resident_estimates_ab.py)", ""]
    try:
        for shape in args.shapes.split(","):
            lines += run_shape(e, float(shape[1:]), args.repeats) + [""]
    finally:
        e.close()
    text = "\n".join(lines)
    print(text)
    if args.out != "/dev/null":
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
