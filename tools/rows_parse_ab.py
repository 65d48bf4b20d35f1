#!/usr/bin/env python3
"""The rows parse (rpvg_amd/csrc/rows_parse.hip): the --write-probs dump read on the GPU, next to the reader it replaces.

Shapes (all of them in one invocation; the file is written after every block): x<scale>, the dump of the rows of synth.generate at
the configs[2] shape (5 000 clusters, 200 000 paths, 10 M reads: 3.28 M rows) times the scale, printed by rpvg_hip_rows_text with
names c<k>_p<j>, bare markers, prob_precision 1e-8.  Measured, wall ms around calls that wait, R runs each after one that is not
listed — and only behind the verdict that every array of the device parse equals the host line's, byte for byte:
  the device parse of the text where it lies on the device (rpvg_hip_table_text_rows);
  the device parse of the text in host memory (rpvg_hip_text_rows: the copy of the text is inside);
  of which kernels: the context's build span (HIP events), which holds the scans and the waits between the stages;
  readTextFile alone, on the plain file of the text;
  readProbabilityClusters on the same text in memory, one host thread: the parent's route, the thing measured against;
  the flat host line: that reader and the flattening of its containers into the arrays the device parse makes.

    python tools/rows_parse_ab.py [--shapes x0.05,x1] [--repeats R] [--out profiles/rows_parse/ab.txt]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fmt(values):
    return " ".join(f"{v:10.3f}" for v in values)


def run_shape(shape, R, write):
    import numpy as np
    from rpvg_amd import engine as eng_mod, synth
    from rpvg_amd import table_text as T

    scale = float(shape[1:])
    K = max(8, int(round(5000 * scale)))
    P = max(K, int(round(200000 * scale)))
    batch = synth.generate(seed=3, num_clusters=K, total_paths=P, total_reads=int(round(10000000 * scale)))
    eff = np.ascontiguousarray(batch.path_effective_length, dtype=np.float64)
    cpo = [int(x) for x in batch.cluster_path_off]
    names = [f"c{k}_p{j}" for k in range(K) for j in range(cpo[k + 1] - cpo[k])]
    labels = T.Labels.of(names, list(range(K)), [int(x) + 50 for x in eff])
    e = eng_mod.Engine(0)
    ok = True
    try:
        resident = T.TableText.rows(e, T.RowsInput.of(batch, eff), labels, 1e-8)
        try:
            text = resident.view()["bytes"]
            lines = [f"rows parse, configs[2] shape x {scale}: {len(text)} bytes of text in {text.count(10)} lines; times in ms, {R} runs each after one that is not listed",
                     "device: " + e.info()[0]]
            # the verdict first
            dump = resident.parse(1e-8)
            got = {**dump.rows_view(e), **dump.view()}
            dump.free()
            host = T.host_line_parse(text, 1e-8)
            differ = [n for n in T.PARSED_ARRAYS if (bytes(got[n]) != host[n] if isinstance(host[n], bytes) else np.asarray(got[n]).tobytes() != np.asarray(host[n]).tobytes())]
            sizes = {n: len(host[n]) for n in ("has_rank_key", "path_length", "row_count", "grp_prob", "path_idx")}
            del got
            if differ:
                lines.append(f"the arrays are NOT the host line's ({', '.join(differ)}); no time is written")
                ok = False
            else:
                lines.append(f"{sizes['has_rank_key']} clusters, {sizes['path_length']} paths, {sizes['row_count']} rows, {sizes['grp_prob']} groups, {sizes['path_idx']} indices; "
                             f"equal to the host line: True")
                resident.parse(1e-8).free()  # the run that is not listed
                device_ms = []
                e.reset_stats()
                for _ in range(R):
                    t0 = time.perf_counter()
                    d = resident.parse(1e-8)
                    device_ms.append(1e3 * (time.perf_counter() - t0))
                    d.free()
                stats = e.stats()
                kernel_ms = stats["build_ms"] / R
                host_text_ms = []
                for run in range(R + 1):
                    t0 = time.perf_counter()
                    d = T.parse_rows(e, text, prob_precision=1e-8)
                    host_text_ms.append(1e3 * (time.perf_counter() - t0))
                    d.free()
                host_text_ms = host_text_ms[1:]
                reader_ms, flat_ms = [], []
                for run in range(R + 1):
                    t0 = time.perf_counter()
                    h = T.host_line_parse(text, 1e-8)
                    flat_ms.append(1e3 * (time.perf_counter() - t0))
                    reader_ms.append(1e3 * h["seconds"])
                    del h
                reader_ms, flat_ms = reader_ms[1:], flat_ms[1:]
                with tempfile.TemporaryDirectory() as tmp:
                    name = os.path.join(tmp, "probs.txt")
                    with open(name, "wb") as f:
                        f.write(text)
                    file_ms = [1e3 * T.read_text_file_seconds(name) for _ in range(R + 1)][1:]
                best = min(device_ms)
                lines.append(f"  device parse, text on the device                     {fmt(device_ms)}   = {len(text) / best / 1e6:.2f} GB/s of text")
                lines.append(f"    of which kernels and the waits between them (HIP events, mean)  {kernel_ms:10.3f}")
                lines.append(f"  device parse, text in host memory                    {fmt(host_text_ms)}")
                lines.append(f"  readTextFile alone (plain file)                      {fmt(file_ms)}")
                lines.append(f"  parent: readProbabilityClusters, one host thread     {fmt(reader_ms)}   = {min(reader_ms) / best:.1f} x the device parse of device text, "
                             f"{min(reader_ms) / min(host_text_ms):.1f} x that of host text")
                lines.append(f"  flat host line (reader + flattening + copies out)    {fmt(flat_ms)}")
        finally:
            resident.free()
        write(lines + [""])
    finally:
        e.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="x0.05,x1")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_parse", "ab.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    blocks = []

    def write(lines):
        blocks.extend(lines)
        with open(args.out, "w") as f:
            f.write("\n".join(blocks) + "\n")
        print("\n".join(lines), flush=True)

    ok = all([run_shape(shape, args.repeats, write) for shape in args.shapes.split(",")])
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
