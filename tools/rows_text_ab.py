#!/usr/bin/env python3
"""The rows text (rpvg_amd/csrc/rows_text.hip): the --write-probs dump of a batch's rows on the GPU, next to the route it replaces.

Shapes (all of them in one invocation; the file is written after every block): x<scale>, the rows of synth.generate at the
configs[2] shape (5 000 clusters, 200 000 paths, 10 M reads: 3.28 M rows) times the scale; names c<k>_p<j>, bare markers,
prob_precision 1e-8.  Measured, wall time around calls that wait for the device, R runs each after one that is not listed — and only
behind the verdict that the text and its row_off equal the host line's, byte for byte:
  the build from resident rows: the row arrays lie on the device before the call (rpvg_hip_rows_text with device pointers, which
  is what rpvg_hip_read_rows_text forwards to: there is no alignment set of this size to build a rpvg_hip_read_rows from); labels,
  effective lengths and cluster_path_off are host arrays, as they are for resident rows;
  the build from host arrays (every array copied by the call); the kernels' own time is the context's build span (HIP events);
  the page-locked download of the text (the first view);
  the parent's route for the same rows: one ReadPathProbabilities per row and writeProbabilityClusters into its stream, from host
  arrays (the download of rpvg_hip_read_rows_view in front of it is not in this figure);
  the host line: the plan's rowBytes and rowWrite on one host thread, both passes.

    python tools/rows_text_ab.py [--shapes x0.05,x1] [--repeats R] [--out profiles/rows_text/ab.txt]
    python tools/rows_text_ab.py --resources [profiles/rows_text/resource_usage.txt]    (cross-compiles; needs no GPU)
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _resources import resource_usage  # noqa: E402

ROW_ARRAYS = ("cluster_row_off", "row_count", "row_noise", "row_grp_off", "grp_prob", "grp_idx_off", "path_idx")


def fmt(values):
    return " ".join(f"{v:10.3f}" for v in values)


def run_shape(shape, R, write):
    import numpy as np
    from rpvg_amd import engine as eng_mod, hip, synth
    from rpvg_amd.table_text import ROWS, HarnessTableText, Labels, RowsInput, TableText

    scale = float(shape[1:])
    K = max(8, int(round(5000 * scale)))
    P = max(K, int(round(200000 * scale)))
    batch = synth.generate(seed=3, num_clusters=K, total_paths=P, total_reads=int(round(10000000 * scale)))
    eff = np.ascontiguousarray(batch.path_effective_length, dtype=np.float64)
    cpo = [int(x) for x in batch.cluster_path_off]
    names = [f"c{k}_p{j}" for k in range(K) for j in range(cpo[k + 1] - cpo[k])]
    labels = Labels.of(names, list(range(K)), [int(x) + 50 for x in eff])
    rows = RowsInput.of(batch, eff)
    sizes = rows.sizes()
    e = eng_mod.Engine(0)
    ok = True
    try:
        lines = [f"rows text, configs[2] shape x {scale}: {K} clusters, {sizes['num_paths']} paths, {sizes['num_rows']} rows, {sizes['num_groups']} groups, "
                 f"{sizes['num_entries']} entries, prob_precision 1e-08; times in ms, {R} runs each after one that is not listed", "device: " + e.info()[0]]
        ctx = e._ctx()
        pointers = {}
        for name in ROW_ARRAYS:
            a = getattr(rows, name)
            p = C.c_void_p()
            hip._check(hip.lib().rpvg_hip_malloc(ctx, C.c_uint64(max(a.nbytes, 8)), C.byref(p)), "rpvg_hip_malloc")
            hip._check(hip.lib().rpvg_hip_memcpy_h2d(ctx, p, C.c_void_p(a.ctypes.data), C.c_uint64(a.nbytes)), "rpvg_hip_memcpy_h2d")
            pointers[name] = p.value
        try:
            # rpvg_hip_rows_text takes one on_device flag: the two host arrays of resident rows go to the device inside the timed call
            resident_ms, stats_resident = [], None
            for run in range(R + 1):
                if run == 1:
                    e.reset_stats()
                t0 = time.perf_counter()
                staged = {}
                for name in ("cluster_path_off", "path_effective_length"):
                    a = getattr(rows, name)
                    p = C.c_void_p()
                    hip._check(hip.lib().rpvg_hip_malloc(ctx, C.c_uint64(max(a.nbytes, 8)), C.byref(p)), "rpvg_hip_malloc")
                    hip._check(hip.lib().rpvg_hip_memcpy_h2d(ctx, p, C.c_void_p(a.ctypes.data), C.c_uint64(a.nbytes)), "rpvg_hip_memcpy_h2d")
                    staged[name] = p.value
                flat = rows.as_c(device_pointers={**pointers, **staged, "num_align_lists": None, "cluster_index": None})
                text = TableText.rows(e, flat, labels, 1e-8)
                resident_ms.append(1e3 * (time.perf_counter() - t0))
                text.free()
                for p in staged.values():
                    hip._check(hip.lib().rpvg_hip_free(ctx, C.c_void_p(p)), "rpvg_hip_free")
            stats_resident = e.stats()
            resident_ms = resident_ms[1:]

            texts = []

            def build():
                for t in texts:
                    t.free()
                texts[:] = [HarnessTableText(e, rows, kind=ROWS, labels=labels, prob_precision=1e-8)]
                return 1e3 * texts[0].build_seconds

            build()
            e.reset_stats()
            host_build_ms = [build() for _ in range(R)]
            stats = e.stats()
            text = texts[0]
            t0 = time.perf_counter()
            v = text.view(copy=False)
            view_ms = [1e3 * (time.perf_counter() - t0)]
            L = len(v["row_off"]) - 1
            text.host_line(L, want_bytes=False)
            host_ms = []
            for _ in range(R):
                line = text.host_line(L, want_bytes=False, recompute=True)
                host_ms.append(1e3 * line["seconds"])
            if not line["equal"]:
                lines.append(f"the text is NOT the host line's ({v['num_bytes']} bytes against {line['num_bytes']}); no time is written")
                ok = False
            else:
                try:
                    parent_ms = [1e3 * text.parent_route()[1] for _ in range(R + 1)][1:]
                except hip.EngineError as error:   # (the writer's text has another length)
                    lines.append(f"  parent route: {error}")
                    parent_ms = []
                kernel_ms, kernel_resident_ms = stats["build_ms"] / R, stats_resident["build_ms"] / R
                lines.append(f"{L} lines, {v['num_rows']} printed, {v['num_bytes']} bytes of text; {stats['text_exact_cells'] // R} cells by the exact comparison; "
                             f"equal to the host line: True")
                lines.append(f"  text build, row arrays on the device                {fmt(resident_ms)}")
                lines.append(f"    of which kernels (HIP events, mean of the runs)    {kernel_resident_ms:10.3f}   = {v['num_bytes'] / max(kernel_resident_ms, 1e-9) / 1e6:.2f} GB/s of text")
                lines.append(f"  text build from host arrays                         {fmt(host_build_ms)}")
                lines.append(f"    of which kernels (HIP events, mean of the runs)    {kernel_ms:10.3f}   = {v['num_bytes'] / max(kernel_ms, 1e-9) / 1e6:.2f} GB/s of text; "
                             f"copies {stats['h2d_ms'] / R:.3f} ({stats['h2d_bytes'] / R / 1e6:.1f} MB)")
                lines.append(f"  page-locked download of the text (first view)       {fmt(view_ms)}")
                lines.append(f"  parent: ReadPathProbabilities + writeProbabilityClusters into a stream  {fmt(parent_ms)}")
                lines.append(f"  host line: one thread, measure + write passes       {fmt(host_ms)}")
            text.free()
        finally:
            for p in pointers.values():
                hip._check(hip.lib().rpvg_hip_free(ctx, C.c_void_p(p)), "rpvg_hip_free")
        write(lines + [""])
    finally:
        e.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="x0.05,x1")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_text", "ab.txt"))
    ap.add_argument("--resources", nargs="?", const=os.path.join(ROOT, "profiles", "rows_text", "resource_usage.txt"))
    args = ap.parse_args()
    if args.resources:
        resource_usage("rows_text.hip", args.resources, spills=True, footer=(
            "no kernel has scratch: as in the other two text files the 2 x 28 words of the exact comparison (number_text.hpp) stay in registers.",
            "measureRowsKernel and writeRowsKernel are workgroups of one wavefront (64 consecutive cells of the file); LDS of writeRowsKernel: the",
            "staging block of that wavefront.  guardKernel is this file's copy of table_text_device.hpp's."))
        return 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").close()

    def write(lines):
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)

    ok = True
    for shape in args.shapes.split(","):
        ok = run_shape(shape, args.repeats, write) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
