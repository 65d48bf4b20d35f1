#!/usr/bin/env python3
"""The set text (rpvg_amd/csrc/set_text.hip) on the estimates of a run, next to the route it replaces.

Shapes (all of them in one invocation; the file is written after every block): x<scale>, synth.generate at the configs[2] shape
(5 000 clusters, 200 000 paths) times the scale, estimated with `-i haplotype-transcripts` at its defaults: the joint file; and
h<scale>, the configs[4] shape (5 000 clusters, 500 000 paths, at most 5 000 per cluster) times the scale, estimated with
`-i haplotypes -y 2 --use-hap-gibbs`: the posterior file.  Measured, wall time around calls that wait for the device, R runs each
after one that is not listed — and only behind the verdict that the text and its row_off equal the host line's, byte for byte:
  the text build from the resident table (labels flattened and uploaded, describe, measure, scan, write); the kernels' own time is
  the context's build span (HIP events); the page-locked download of the text (the first view);
  the parent's route for the same rows: the writer's addTable() into its stream, from the table's host view;
  the host line: the same row descriptor on one host thread, both passes.

    python tools/set_text_ab.py [--shapes x0.05,x1,h1] [--repeats R] [--out profiles/set_text/ab.txt]
    python tools/set_text_ab.py --resources [profiles/set_text/resource_usage.txt]    (cross-compiles; needs no GPU)
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


def measure(e, lines, what, table, kind, ploidy, min_posterior, R):
    from rpvg_amd.table_text import HarnessTableText
    texts = []

    def build():
        for t in texts:
            t.free()
        texts[:] = [HarnessTableText(e, table, kind=kind, ploidy=ploidy, min_posterior=min_posterior)]

    build()
    e.reset_stats()
    build_ms = ms(build, R)
    stats = e.stats()
    text = texts[0]
    view_ms = ms(lambda: text.view(copy=False), 1)
    v = text.view(copy=False)
    S = len(v["row_off"]) - 1
    text.host_line(S, want_bytes=False)
    host_ms = []
    for _ in range(R):
        line = text.host_line(S, want_bytes=False, recompute=True)
        host_ms.append(1e3 * line["seconds"])
    if not line["equal"]:
        lines.append(f"{what}: the text is NOT the host line's ({v['num_bytes']} bytes against {line['num_bytes']}); no time is written")
        text.free()
        return False
    parent_ms = [1e3 * text.parent_route()[1] for _ in range(R + 1)][1:]
    kernel_ms = stats["build_ms"] / R
    lines.append(f"{what}: {S} sets, {v['num_rows']} rows printed, {v['num_bytes']} bytes of text; {stats['text_exact_cells'] // R} cells by the exact comparison; "
                 f"equal to the host line: True")
    lines.append(f"  text build from the resident table                  {fmt(build_ms)}")
    lines.append(f"    of which kernels (HIP events, mean of the runs)    {kernel_ms:10.3f}   = {v['num_bytes'] / max(kernel_ms, 1e-9) / 1e6:.2f} GB/s of text; "
                 f"copies {stats['h2d_ms'] / R:.3f} ({stats['h2d_bytes'] / R / 1e6:.1f} MB)")
    lines.append(f"  page-locked download of the text (first view)       {fmt(view_ms)}")
    lines.append(f"  parent: addTable() into the writer's stream         {fmt(parent_ms)}")
    lines.append(f"  host line: one thread, measure + write passes       {fmt(host_ms)}")
    text.free()
    return True


def run_shape(shape, R, write):
    from rpvg_amd import engine as eng_mod, synth
    from rpvg_amd.batch import make_params
    from rpvg_amd.estimates_table import HarnessTable, write_from_containers
    from rpvg_amd.table_text import JOINT, POSTERIOR

    haplotypes = shape[0] == "h"
    scale = float(shape[1:])
    K = max(8, int(round(5000 * scale)))
    P = max(K, int(round((500000 if haplotypes else 200000) * scale)))
    if haplotypes:
        model, params, config = "haplotypes", make_params(use_hap_gibbs=1), "configs[4]"
        batch = synth.generate(seed=5, num_clusters=K, total_paths=P, total_reads=int(round(10000000 * scale)), max_cluster_paths=5000)
    else:
        model, params, config = "haplotype-transcripts", make_params(), "configs[2]"
        batch = synth.generate(seed=3, num_clusters=K, total_paths=P, total_reads=int(round(10000000 * scale)))
    e = eng_mod.Engine(0)
    try:
        prepared = e.prepare(batch)
        t0 = time.perf_counter()
        e.run(model, params, prepared)
        lines = [f"set text, {config} shape x {scale}, -i {model}{' -y 2 --use-hap-gibbs' if haplotypes else ''}: {K} clusters, {P} paths, ploidy {params.ploidy}, "
                 f"min posterior {params.prob_precision:g} (estimate {1e3 * (time.perf_counter() - t0):.0f} ms with its Python containers); times in ms, {R} runs each "
                 f"after one that is not listed", "device: " + e.info()[0]]
        table = HarnessTable(e, prepared, params.ploidy)
        try:
            if not haplotypes:
                table.tpm(write_from_containers(prepared, "", params.ploidy, "")[0])
            ok = measure(e, lines, "posterior file" if haplotypes else "joint file", table, POSTERIOR if haplotypes else JOINT, params.ploidy, params.prob_precision, R)
        finally:
            table.free()
        write(lines + [""])
        prepared.free()
    finally:
        e.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="x0.05,x1,h1")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_text", "ab.txt"))
    ap.add_argument("--resources", nargs="?", const=os.path.join(ROOT, "profiles", "set_text", "resource_usage.txt"))
    args = ap.parse_args()
    if args.resources:
        resource_usage("set_text.hip", args.resources, spills=True, footer=(
            "no kernel has scratch: as in table_text.hip the 2 x 28 words of the exact comparison (number_text.hpp) stay in registers, which the measure",
            "and the write kernel pay 198 VGPRs (2 waves/SIMD) for; the SGPR spills of writeSetsKernel go to VGPR lanes, not to memory.",
            "LDS of writeSetsKernel: the staging block of one wavefront.  guardKernel is this file's copy of table_text_device.hpp's."))
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
