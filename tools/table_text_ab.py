#!/usr/bin/env python3
"""The table text (rpvg_amd/csrc/table_text.hip) on the tables of a run, next to the route it replaces.

Shapes (all of them in one invocation; the file is written after every block): x<scale>, synth.generate at the configs[2] shape
(5 000 clusters, 200 000 paths) times the scale, estimated with `-i haplotype-transcripts` and with `-i transcripts`, at every N of
--n (--gibbs-thin-its 1: the text does not care how far apart the recorded states are).  Per shape the Gibbs file, and at the
first N the estimates file of the model (haplotype rows; per-path abundance rows for transcripts).  Measured, wall time around
calls that wait for the device, R runs each after one that is not listed — and only behind the verdict that the text and its
row_off equal the host line's, byte for byte:
  the text build from the resident table (labels flattened and uploaded, describe, measure, scan, write); the kernels' own time is
  the context's build span (HIP events) and gives the bytes per second; the page-locked download of the text;
  the parent's route for the same rows: the writer's addTable() into its stream, from the table's host view (whose download is
  measured in profiles/gibbs_table/ab.txt and profiles/estimates_table/ab.txt); the host line: the same row descriptors on one
  host thread, both passes.  Texts of 3 * 10^7 cells and more take the two host figures once, without a warm-up: a run is seconds.
Also: the text's size against the 8 bytes per cell it replaces, and the cells that took the exact comparison.

    python tools/table_text_ab.py [--shapes x0.05,x1] [--n 100,1000] [--repeats R] [--out profiles/table_text/ab.txt]
    python tools/table_text_ab.py --resources [profiles/table_text/resource_usage.txt]    (cross-compiles; needs no GPU)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _resources import resource_usage  # noqa: E402


def ms(f, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def fmt(values):
    return " ".join(f"{v:10.3f}" for v in values)


def measure(e, lines, what, table, kind, P, cells_per_row, N, R):
    """One file: table is the harness table the text is made from; cells_per_row: the numbers of a printed row."""
    from rpvg_amd.table_text import HarnessTableText
    texts = []

    def build():
        for t in texts:
            t.free()
        texts[:] = [HarnessTableText(e, table, kind=kind)]

    build()
    e.reset_stats()
    build_ms = ms(build, R)
    stats = e.stats()
    text = texts[0]
    view_ms = ms(lambda: text.view(copy=False), 1)
    v = text.view(copy=False)
    cells = v["num_rows"] * cells_per_row
    host_runs = R if cells < 3e7 else 1
    host_ms = []
    if host_runs > 1:
        text.host_line(P, want_bytes=False)
    for i in range(host_runs):
        line = text.host_line(P, want_bytes=False, recompute=host_runs > 1 or i > 0)
        host_ms.append(1e3 * line["seconds"])
    if not line["equal"]:
        lines.append(f"{what}: the text is NOT the host line's ({v['num_bytes']} bytes against {line['num_bytes']}); no time is written")
        text.free()
        return False
    parent_ms = [1e3 * text.parent_route(N)[1] for _ in range(host_runs + (1 if host_runs > 1 else 0))][-host_runs:]
    kernel_ms = stats["build_ms"] / R
    lines.append(f"{what}: {v['num_rows']} rows, {cells} cells, {v['num_bytes']} bytes of text = {v['num_bytes'] / max(cells, 1):.2f} per cell against the 8 of a double "
                 f"({8 * cells} bytes); {stats['text_exact_cells'] // R} cells by the exact comparison; equal to the host line: True")
    lines.append(f"  text build from the resident table                  {fmt(build_ms)}")
    lines.append(f"    of which kernels (HIP events, mean of the runs)    {kernel_ms:10.3f}   = {v['num_bytes'] / max(kernel_ms, 1e-9) / 1e6:.2f} GB/s of text, "
                 f"{cells / max(kernel_ms, 1e-9) / 1e3:.1f} M cells/s; copies {stats['h2d_ms'] / R:.3f} ({stats['h2d_bytes'] / R / 1e6:.1f} MB)")
    lines.append(f"  page-locked download of the text (first view)       {fmt(view_ms)}   = {v['num_bytes'] / max(view_ms[0], 1e-9) / 1e6:.2f} GB/s")
    lines.append(f"  parent: addTable() into the writer's stream         {fmt(parent_ms)}")
    lines.append(f"  host line: one thread, measure + write passes       {fmt(host_ms)}")
    text.free()
    return True


def run_shape(shape, model, Ns, R, write):
    from rpvg_amd import engine as eng_mod, synth
    from rpvg_amd.batch import make_params
    from rpvg_amd.estimates_table import HarnessTable, write_from_containers
    from rpvg_amd.gibbs_table import HarnessGibbsTable
    from rpvg_amd.table_text import HAPLOTYPE, PER_PATH

    scale = float(shape.lstrip("x"))
    K = max(8, int(round(5000 * scale)))
    P = max(K, int(round(200000 * scale)))
    batch = synth.generate(seed=3, num_clusters=K, total_paths=P, total_reads=int(round(10000000 * scale)))
    ok = True
    e = eng_mod.Engine(0)
    try:
        prepared = e.prepare(batch)
        for i, N in enumerate(Ns):
            params = make_params(num_gibbs_samples=N, gibbs_thin_its=1)
            t0 = time.perf_counter()
            e.run(model, params, prepared)
            lines = [f"table text, configs[2] shape x {scale}, -i {model}, -n {N} (--gibbs-thin-its 1): {K} clusters, {P} paths (estimate "
                     f"{1e3 * (time.perf_counter() - t0):.0f} ms with its Python containers); times in ms, {R} runs each after one that is not listed",
                     "device: " + e.info()[0]]
            gibbs = HarnessGibbsTable(e, prepared, N)
            try:
                ok = measure(e, lines, "gibbs file", gibbs, None, P, N + 1, N, R) and ok
            finally:
                gibbs.free()
            if i == 0:
                total = write_from_containers(prepared, "", params.ploidy, "")[0]
                table = HarnessTable(e, prepared, params.ploidy)
                try:
                    table.tpm(total)
                    kind, name = (PER_PATH, "abundance file (per-path rows)") if model == "transcripts" else (HAPLOTYPE, "haplotype file (per-path rows)")
                    ok = measure(e, lines, name, table, kind, P, 4 if kind == PER_PATH else 5, 0, R) and ok
                finally:
                    table.free()
            write(lines + [""])
        prepared.free()
    finally:
        e.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="x0.05,x1")
    ap.add_argument("--models", default="haplotype-transcripts,transcripts")
    ap.add_argument("--n", default="100,1000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_text", "ab.txt"))
    ap.add_argument("--resources", nargs="?", const=os.path.join(ROOT, "profiles", "table_text", "resource_usage.txt"))
    args = ap.parse_args()
    if args.resources:
        resource_usage("table_text.hip", args.resources, footer=(
            "no kernel has scratch: the 2 x 28 words of the exact comparison (number_text.hpp) are walked by loops of constant length and stay in registers,",
            "which is what the measure and the write kernel pay their 140-160 VGPRs (3 waves/SIMD) for; LDS of writeKernel: the staging block of one wavefront."))
        return 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").close()

    def write(lines):
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)

    ok = True
    for shape in args.shapes.split(","):
        for model in args.models.split(","):
            ok = run_shape(shape, model, [int(n) for n in args.n.split(",")], args.repeats, write) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
