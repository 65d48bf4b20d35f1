#!/usr/bin/env python3
"""The two routes of the minimum path cover (`-i strains`) next to each other on synthetic clusters of 3 entries per row.

  workgroup   rpvg_hip_min_path_cover: one workgroup per cluster (rpvg_amd/csrc/path_cover.hip) — the yardstick
  grid        rpvg_hip_min_path_cover_any(..., grid_min_work = 1): the whole GPU, a cluster at a time (path_cover_grid.hip)

Shapes: 2^14, 2^16, 2^18 and 2^20 rows, and 2^8, 2^10 and 2^12 below them to find where the grid stops winning; 600 and 9 600
paths; covers of about 8, 100 and 1 000 paths (500 at 600 paths, which cannot hold 1 000; no more than the rows), planted in the manner of wide_cluster / long_cover_cluster of tests/path_cover_cases.py: row r belongs to
planted path r mod C (probability 0.3 .. 0.6) next to two decoys (below 0.01); and one cluster of 65 537 paths, which only the
grid takes.  One cluster per call, wall time around calls that wait for the device, three runs each; the first call of the
process is reported on its own.  The two covers must be equal before a time is written down.  The last lines state what the
table says about a default work threshold (rpvg_amd/csrc/cover_plan.hpp): the smallest power of two of work (rows + entries)
from which the grid is at least twice as fast for every measured cover length.

    python tools/path_cover_grid_ab.py [--repeats R] [--commit ID] [--out profiles/path_cover_grid/ab.txt]
    python tools/path_cover_grid_ab.py --resources [profiles/path_cover_grid/resource_usage.txt]    (cross-compiles; needs no GPU)
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _resources import resource_usage  # noqa: E402


def planted_cluster(seed, n_rows, n_paths, n_cover):
    """One cluster as a ClusterBatch, arrays made by numpy: three probability groups of one path per row."""
    from rpvg_amd.batch import ClusterBatch
    rng = np.random.default_rng(seed)
    planted = rng.permutation(n_paths)[:n_cover].astype(np.uint32)
    pool = np.setdiff1d(np.arange(n_paths, dtype=np.uint32), planted)
    r = np.arange(n_rows)
    noise = 1e-4 + (0.2 - 1e-4) * (rng.permutation(n_rows) + 0.5) / n_rows
    scale = 1.0 - noise
    d1 = rng.integers(0, len(pool), size=n_rows)
    d2 = (d1 + 1 + rng.integers(0, len(pool) - 1, size=n_rows)) % len(pool)
    low = np.sort(rng.uniform(1e-3, 1e-2, size=(n_rows, 2)), axis=1)
    low[:, 1] += 1e-6   # (strictly ascending within the row)
    prob = np.empty((n_rows, 3))
    prob[:, :2] = low * scale[:, None]
    prob[:, 2] = rng.uniform(0.3, 0.6, size=n_rows) * scale
    path = np.empty((n_rows, 3), dtype=np.uint32)
    path[:, 0], path[:, 1], path[:, 2] = pool[d1], pool[d2], planted[r % n_cover]
    return ClusterBatch(cluster_row_off=np.array([0, n_rows]), cluster_path_off=np.array([0, n_paths]),
                        row_count=rng.integers(1, 21, size=n_rows), row_noise=noise, row_grp_off=3 * np.arange(n_rows + 1),
                        grp_prob=prob.reshape(-1), grp_idx_off=np.arange(3 * n_rows + 1), path_idx=path.reshape(-1),
                        path_group_id=np.zeros(n_paths), path_source_count=np.ones(n_paths), path_source_off=np.arange(n_paths + 1),
                        source_id=np.arange(n_paths), path_effective_length=np.full(n_paths, 100.0))


def ms(f, repeats):
    out, result = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        result = f()
        out.append(1e3 * (time.perf_counter() - t0))
    return out, result


def fmt(values):
    return " ".join(f"{v:10.3f}" for v in values)


def commit_id():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--rows", type=int, nargs="*", default=[1 << 8, 1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_cover_grid", "ab.txt"))
    ap.add_argument("--resources", nargs="?", const=os.path.join(ROOT, "profiles", "path_cover_grid", "resource_usage.txt"), default=None)
    args = ap.parse_args()
    if args.resources:
        resource_usage("path_cover_grid.hip", args.resources,
                       header_note=" (hipcub's own kernels left out;\nLDS is the static part: coverStrikeKernel<true> adds 8 bytes per path of the cluster, at most 16 384)")
        return 0

    from rpvg_amd import hip

    lim = hip.cover_limits()
    lines = [f"minimum path cover, workgroup route against grid route: one cluster per call, 3 entries per row; wall ms around calls that wait for "
             f"the device, {args.repeats} runs each", f"commit: {args.commit or commit_id()}"]
    ctx = hip.Context(0)
    ok = True
    table = {}   # work -> [ratio of every cover length and width]
    try:
        lines.append("device: " + str(ctx.info()[0]))
        warm = ctx.upload(planted_cluster(1, 256, 16, 4))
        first_w, _ = ms(lambda: ctx.min_path_cover(warm, [0]), 1)
        first_g, _ = ms(lambda: ctx.min_path_cover_any(warm, [0], grid_min_work=1), 1)
        lines.append(f"first call of the process (256 rows, 16 paths): workgroup {first_w[0]:.3f}   grid {first_g[0]:.3f}")
        warm.free()
        lines.append(f"{'paths':>7}{'rows':>9}{'work':>9}{'cover':>7}   {'workgroup':^32}   {'grid':^32}   workgroup / grid (medians)")
        for n_paths in (600, 9600):
            for n_rows in args.rows:
                for n_cover in (8, 100, 1000 if n_paths > 1000 else 500):
                    dev = ctx.upload(planted_cluster(100 + n_cover, n_rows, n_paths, n_cover))
                    ctx.min_path_cover_any(dev, [0], grid_min_work=1)   # (the pool holds the scratch from here on)
                    tw, cw = ms(lambda: ctx.min_path_cover(dev, [0]), args.repeats)
                    tg, cg = ms(lambda: ctx.min_path_cover_any(dev, [0], grid_min_work=1), args.repeats)
                    dev.free()
                    if cw != cg:
                        ok = False
                        lines.append(f"{n_paths:>7}{n_rows:>9}{4 * n_rows:>9}{n_cover:>7}   THE COVERS DIFFER: no times")
                        continue
                    ratio = float(np.median(tw) / np.median(tg))
                    table.setdefault(4 * n_rows, []).append(ratio)
                    lines.append(f"{n_paths:>7}{n_rows:>9}{4 * n_rows:>9}{len(cw[0]):>7}   {fmt(tw)}   {fmt(tg)}   {ratio:8.2f}")
        dev = ctx.upload(planted_cluster(7, 1 << 16, 65537, 100))
        ctx.min_path_cover_any(dev, [0])
        tg, cg = ms(lambda: ctx.min_path_cover_any(dev, [0]), args.repeats)
        dev.free()
        lines.append(f"{65537:>7}{1 << 16:>9}{4 << 16:>9}{len(cg[0]):>7}   {'(too wide)':^32}   {fmt(tg)}")
    finally:
        ctx.close()
    works = sorted(table)
    verdict = None
    for w in works:   # the smallest measured work from which every larger size, every width and cover length gives the factor of two
        if all(min(table[x]) >= 2.0 for x in works if x >= w):
            verdict = w
            break
    lines.append("smallest ratio per work: " + "   ".join(f"{w}: {min(table[w]):.2f}" for w in works))
    lines.append(f"default threshold by the rule (grid at least twice as fast for every cover length from there on): "
                 f"{'width only — no measured size gives the factor' if verdict is None else verdict}"
                 f"   (the library as built: {'width only' if lim.default_grid_min_work == hip.GRID_NEVER else lim.default_grid_min_work})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
