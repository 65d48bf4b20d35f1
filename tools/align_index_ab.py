#!/usr/bin/env python3
"""The alignment-path index (rpvg_amd/csrc/align_index.hip) on the configs[2] reads, next to a one-thread host line.

The alignment-path lists of synth.generate_with_alignments (distinct lists with multiplicities, cluster-local indices) are
expanded by their multiplicities into a shuffled stream of per-fragment lists with global path ids — what the alignment parser
would hand over — and put through
  device   rpvg_hip_align_index_add per chunk + rpvg_hip_align_index_finish: wall time end to end, and the context's spans
           (copies: h2d_ms; kernels of add and finish: build_ms);
  host     rpvg_amd_align_index_host_line: one thread, std::unordered_map keyed by the list's contents — the structure of
           addAlignmentPathsBufferToIndexes (src/main.cpp:200-237).
The two results are compared at full size: histogram, number of distinct lists, first occurrence and multiplicity of each.

    python tools/align_index_ab.py [--scale F] [--chunk N] [--repeats R] [--out profiles/align_index/ab.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rpvg_amd import engine as eng_mod, hip, synth  # noqa: E402
from rpvg_amd.index import AlignmentIndex, CFragmentLists, FragmentLists, IndexParams  # noqa: E402


def ranges(starts, counts):
    """Concatenation of arange(starts[i], starts[i] + counts[i])."""
    total = int(counts.sum())
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    return np.repeat(starts - off[:-1], counts) + np.arange(total, dtype=np.int64), off


def stream_chunks(batch, al, seed, chunk):
    """The reads of `al` repeated by their multiplicities, shuffled, as FragmentLists chunks with global path ids."""
    N = al.num_reads
    read_cluster = np.repeat(np.arange(al.num_clusters, dtype=np.int64), np.diff(al.cluster_read_off.astype(np.int64)))
    rao, apo = al.read_align_off.astype(np.int64), al.align_path_off.astype(np.int64)
    order = np.repeat(np.arange(N, dtype=np.int64), al.read_count.astype(np.int64))
    np.random.default_rng(seed).shuffle(order)
    cpo = batch.cluster_path_off.astype(np.int64)
    out = []
    for begin in range(0, len(order), chunk):
        reads = order[begin:begin + chunk]
        aligns, list_off = ranges(rao[reads], rao[reads + 1] - rao[reads])
        entries, align_off = ranges(apo[aligns], apo[aligns + 1] - apo[aligns])
        entry_cluster = np.repeat(np.repeat(read_cluster[reads], np.diff(list_off)), np.diff(align_off))
        frag = al.align_frag_length[aligns]
        out.append(FragmentLists((frag[list_off[:-1]] > 0).astype(np.uint8), al.read_min_mapq[reads], al.read_noise_score[reads], list_off,
                                 al.align_score_sum[aligns], al.align_length[aligns], frag, align_off,
                                 al.align_path_idx[entries].astype(np.int64) + cpo[entry_cluster]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--chunk", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_index", "ab.txt"))
    args = ap.parse_args()
    K = max(8, int(round(5000 * args.scale)))
    P = max(K, int(round(200000 * args.scale)))
    batch, al = synth.generate_with_alignments(seed=3, num_clusters=K, total_paths=P, total_reads=int(round(10000000 * args.scale)))
    chunks = stream_chunks(batch, al, 17, args.chunk)
    F = sum(c.num_lists for c in chunks)
    A = sum(len(c.align_score_sum) for c in chunks)
    E = sum(len(c.align_path_id) for c in chunks)
    # maxLength() of the prior: here the largest fragment length that is counted (the histogram then lives in LDS, as in a real run)
    max_frag = max(int(c.align_frag_length[c.list_align_off[:-1].astype(np.int64)].max()) for c in chunks)
    params = IndexParams(num_paths=P, max_frag_length=max_frag, pre_frag_loc=300)
    lines = [f"alignment-path index, configs[2] reads x {args.scale}: {F} lists, {A} alignments, {E} entries, {P} paths, chunks of {args.chunk}, {max_frag + 1} histogram bins"]

    ctx = hip.Context(0)
    try:
        lines.append("device: " + ctx.info()[0])
        view = counts = info = None
        for rep in range(args.repeats):
            ctx.reset_stats()
            t0 = time.perf_counter()
            index = AlignmentIndex(ctx, params)
            for c in chunks:
                index.add(c)
            t1 = time.perf_counter()
            info = index.finish()
            t2 = time.perf_counter()
            st = ctx.stats()
            lines.append(f"device run {rep}: add {1e3 * (t1 - t0):9.2f} ms  finish {1e3 * (t2 - t1):9.2f} ms  total {1e3 * (t2 - t0):9.2f} ms   "
                         f"spans: h2d {st['h2d_ms']:.2f} ms, kernels (add + finish) {st['build_ms']:.2f} ms")
            if rep == args.repeats - 1:
                view, counts = index.view(), index.frag_counts()
            index.free()
        lines.append(f"device result: {info.num_distinct} distinct lists, {info.num_clusters} clusters, {info.num_collision_lists} lists through the collision path")
    finally:
        ctx.close()

    L = eng_mod.lib()
    cchunks = (CFragmentLists * len(chunks))(*[c.as_c() for c in chunks])
    cparams = params.as_c()
    host_counts = np.zeros(params.max_frag_length + 1, dtype=np.uint32)
    first, mult = np.zeros(F, dtype=np.uint64), np.zeros(F, dtype=np.uint32)
    D, secs = C.c_uint64(0), C.c_double(0)
    L.rpvg_amd_align_index_host_line.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for rep in range(min(args.repeats, 2)):
        rc = L.rpvg_amd_align_index_host_line(C.addressof(cchunks), len(chunks), C.addressof(cparams), host_counts.ctypes.data, C.addressof(D),
                                              first.ctypes.data, mult.ctypes.data, C.addressof(secs))
        assert rc == 0
        lines.append(f"host line run {rep} (one thread, std::unordered_map): {1e3 * secs.value:9.2f} ms, {D.value} distinct lists")
    by_first = np.argsort(view.first_occurrence, kind="stable")
    same = (D.value == info.num_distinct and np.array_equal(host_counts, counts) and np.array_equal(view.first_occurrence[by_first], first[:D.value])
            and np.array_equal(view.batch.read_count[by_first], mult[:D.value]))
    lines.append(f"device result equals the host line (histogram, distinct lists, first occurrence and multiplicity of each): {same}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
