#!/usr/bin/env python3
"""A text as BGZF on the GPU (rpvg_amd/csrc/text_deflate.hip) next to the route it replaces, for the two .gz files of a run.

Texts, at the configs[2] shape (5 000 clusters, 200 000 paths, 10 M reads) times --scale: the Gibbs text of -i transcripts -n N
(a row per path) and the --write-probs text of the batch's rows.  Measured, wall time around calls that wait for the device, R
runs each on a fresh text (the spread is the runs themselves) — and only behind the verdict that the members inflate to the text:
  the device compression (rpvg_hip_table_text_bgzf: zeroing the slots, the chunk kernel, the sum, the gather);
  the page-locked download of the compressed bytes (the first view);
  the file from them (the writer's framing of its own rows, the end-of-file block, one fwrite);
  the parent's route: the page-locked download of the plain text (the first view) and the writer's file through zlib's gzwrite.
Sizes: the members, and zlib at levels 1 and 6 over the same chunks with the same 26 bytes of frame around each.

    python tools/text_bgzf_ab.py [--scale 1] [--n 100] [--repeats 3] [--tree NAME] [--out profiles/text_bgzf/ab.txt]
    python tools/text_bgzf_ab.py --resources [profiles/text_bgzf/resource_usage.txt]    (cross-compiles; needs no GPU)
"""
import argparse
import gzip
import os
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _resources import resource_usage  # noqa: E402

CHUNK = 65280


def fmt(values):
    return " ".join(f"{v:10.3f}" for v in values)


def zlib_size(text, level):
    total = 0
    for at in range(0, len(text), CHUNK):
        deflater = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(deflater.compress(text[at:at + CHUNK])) + len(deflater.flush()) + 26
    return total


def measure(lines, what, make_text, R, tmp, **write_args):
    """make_text() -> a fresh HarnessTableText; the file names are the writers' (a prefix, or the file itself for the dump)."""
    compress_ms, download_ms, file_ms, plain_ms, gz_ms = [], [], [], [], []
    target = os.path.join(tmp, "ab_" + what.split()[0])
    for run in range(R + 1):
        text = make_text()
        try:
            members = text.bgzf(copy=False)
            t0 = time.perf_counter()
            text.write(target + "_bgzf" + (".txt.gz" if write_args == {} else ""), compressed=True, **write_args)
            t1 = time.perf_counter()
            plain = text.view(copy=False)
            t2 = time.perf_counter()
            text.write(target + "_gz" + (".txt.gz" if write_args == {} else ""), **write_args)
            t3 = time.perf_counter()
            if run:
                compress_ms.append(1e3 * members["compress_seconds"])
                download_ms.append(1e3 * members["download_seconds"])
                file_ms.append(1e3 * (t1 - t0))
                plain_ms.append(1e3 * (t2 - t1))
                gz_ms.append(1e3 * (t3 - t2))
            if run == R:
                plain_bytes = text.view()["bytes"]
                members = text.bgzf()
        finally:
            text.free()
    names = [target + kind + ".txt.gz" for kind in ("_bgzf", "_gz")]
    from tests import bgzf_model as B
    file_bytes = open(names[0], "rb").read()
    if B.text_of(members["bytes"]) != plain_bytes or gzip.open(names[0], "rb").read() != gzip.open(names[1], "rb").read() or not file_bytes.endswith(B.EOF_BLOCK):
        lines.append(f"{what}: the members do NOT give the text back; no time is written")
        return False
    n, m = len(plain_bytes), members["num_bytes"]
    level1, level6 = zlib_size(plain_bytes, 1), zlib_size(plain_bytes, 6)
    device, parent = [c + d + f for c, d, f in zip(compress_ms, download_ms, file_ms)], [p + g for p, g in zip(plain_ms, gz_ms)]
    lines.append(f"{what}: {n} bytes of text in {members['num_members']} chunks -> {m} bytes of members = {m / n:.4f} of the text, {members['num_stored_members']} stored; "
                 f"zlib over the same chunks: level 1 {level1} = {level1 / n:.4f}, level 6 {level6} = {level6 / n:.4f}; members / level 1 = {m / level1:.3f}; "
                 f"the file of the parent's gzwrite (one stream, level 6): {os.path.getsize(names[1])}")
    lines.append(f"  device compression                                   {fmt(compress_ms)}   = {n / max(min(compress_ms), 1e-9) / 1e6:.2f} GB/s of text at best")
    lines.append(f"  page-locked download of the members (first view)     {fmt(download_ms)}")
    lines.append(f"  the file from the members (framing, fwrite)          {fmt(file_ms)}")
    lines.append(f"  device route, sum                                    {fmt(device)}")
    lines.append(f"  parent: page-locked download of the text (first view){fmt(plain_ms)}")
    lines.append(f"  parent: the writer's file through gzwrite            {fmt(gz_ms)}")
    lines.append(f"  parent's route, sum                                  {fmt(parent)}")
    if max(device) < min(parent):
        lines.append(f"  the device route beats the parent's on this box: {min(parent) / max(device):.1f} times at the least")
    else:
        lines.append("  the device route does NOT beat the parent's on this box in every run")
    return True


def run(scale, N, R, write, tree):
    import numpy as np
    from rpvg_amd import engine as eng_mod, synth
    from rpvg_amd.batch import make_params
    from rpvg_amd.gibbs_table import HarnessGibbsTable
    from rpvg_amd.table_text import ROWS, HarnessTableText, Labels, RowsInput

    K = max(8, int(round(5000 * scale)))
    P = max(K, int(round(200000 * scale)))
    batch = synth.generate(seed=3, num_clusters=K, total_paths=P, total_reads=int(round(10000000 * scale)))
    commit = tree or subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True).stdout.strip() or "unknown"
    ok = True
    e = eng_mod.Engine(0)
    try:
        with tempfile.TemporaryDirectory() as tmp:
            lines = [f"text as BGZF, configs[2] shape x {scale}: {K} clusters, {P} paths; tree {commit}; times in ms, {R} runs each on a fresh text after one that is not listed",
                     "device: " + e.info()[0]]
            prepared = e.prepare(batch)
            try:
                e.run("transcripts", make_params(num_gibbs_samples=N, gibbs_thin_its=1), prepared)
                gibbs = HarnessGibbsTable(e, prepared, N)
                try:
                    ok = measure(lines, f"gibbs file (-i transcripts -n {N})", lambda: HarnessTableText(e, gibbs), R, tmp, num_gibbs_samples=N) and ok
                finally:
                    gibbs.free()
            finally:
                prepared.free()
            write(lines)
            eff = np.ascontiguousarray(batch.path_effective_length, dtype=np.float64)
            cpo = [int(x) for x in batch.cluster_path_off]
            names = [f"c{k}_p{j}" for k in range(K) for j in range(cpo[k + 1] - cpo[k])]
            labels = Labels.of(names, list(range(K)), [int(x) + 50 for x in eff])
            rows = RowsInput.of(batch, eff)
            lines = []
            ok = measure(lines, "probs file (--write-probs, one batch)", lambda: HarnessTableText(e, rows, kind=ROWS, labels=labels, prob_precision=1e-8), R, tmp) and ok
            write(lines + [""])
    finally:
        e.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tree", default="", help="what to call the tree in the file where git cannot say (default: git describe --always --dirty)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_bgzf", "ab.txt"))
    ap.add_argument("--resources", nargs="?", const=os.path.join(ROOT, "profiles", "text_bgzf", "resource_usage.txt"))
    args = ap.parse_args()
    if args.resources:
        resource_usage("text_deflate.hip", args.resources, spills=True, footer=(
            "no kernel has scratch: every table of deflateChunkKernel — the work space of the plan's code-length routine included — is in LDS.",
            "deflateChunkKernel: a workgroup of 1024 lanes per chunk; its LDS is dynamic (159 528 bytes: the chunk, its shadow, two token masks,",
            "the match table, histograms and codes), which is what holds it to one workgroup = 16 wavefronts per CU, not its registers.",
            "guardKernel is this file's copy of table_text_device.hpp's."))
        return 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").close()

    def write(lines):
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)

    return 0 if run(args.scale, args.n, args.repeats, write, args.tree) else 1


if __name__ == "__main__":
    sys.exit(main())
