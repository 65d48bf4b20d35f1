"""The cases of the all-pairs diploid search (tests/pair_search_cases.py) checked without a GPU: the conditions under which
the device test (tests/test_hip_pair_search.py) can neither pass nor fail by accident, asserted on the model and the oracle
alone — every pair is kept, the order of the marginals is decided, a wrong cell or a dropped row moves some sum far above the
tolerance — and that the cases put the row classes, the blocks and the folds where their names say."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import np_oracle
from tests import pair_search_cases as psc


@pytest.mark.parametrize("case", psc.CASES, ids=lambda c: c.name)
def test_conditions_of_the_case(case):
    ref = case.reference()
    model = ref.model
    G, pairs = case.G, case.G * (case.G + 1) // 2
    M, noise, counts, mult = case.matrix()
    assert M.shape == (case.R, G) and len(model.sequence) == pairs
    spread, marginal_spread = psc.spreads(model)
    gap = psc.smallest_marginal_gap(model)
    rows, columns = psc.row_bites(case), psc.column_bites(model)
    # (a row of noise 1 without entries adds log 1 = 0 to every sum, by design: removing it changes nothing.  Those few rows lie
    # inside the count-1 class, never on an edge: the rows at the edges are asserted to count, below)
    counted = noise < 1.0
    print(f"{case.name:45s} {case.R:5d} x {G:4d}: spread {spread:6.1f} / {marginal_spread:6.1f}, oracle {ref.oracle_deviation:.1e} (normaliser {ref.oracle_best:.1e}), "
          f"tol {ref.tol:.1e}, marginal gap {gap:.1e}, row bite {rows[counted].min():.1e}, column bite {columns.min():.1e}")

    # 1. every pair is kept: 650 of the 690.8 log units of the threshold, for the pairs and for the marginals (whose exp must not
    #    underflow into ties); the smallest posterior is then above exp(-(650 + log(pairs))), a normal number (9.7e-289 for the
    #    525 825 pairs of the widest case), and those of the cases as drawn are far above that
    assert spread <= psc.MAX_SPREAD and marginal_spread <= psc.MAX_SPREAD
    assert math.exp(-(psc.MAX_SPREAD + math.log(pairs))) > 9e-289 > 1e10 * np.finfo(np.float64).tiny
    assert len(ref.oracle_sets) == pairs
    assert ref.oracle_sets == model.sequence    # the oracle visits the pairs in the model's order
    assert np.all(ref.oracle_posteriors > 1e-288) and abs(float(ref.oracle_posteriors.sum()) - 1) < 1e-9

    # the model agrees with the oracle: R additions in FP64 of terms of one sign are within R 2^-53 of the sum relative, a
    # logarithm adds an ulp per term — (R + 8) 2^-52 max |ll| bounds a pair's sum; the oracle's normaliser folds add_log over the
    # pairs one by one (src/path_estimator.cpp:453-463), an ulp of the running value per pair on top
    bar = (case.R + 8) * 2.0 ** -52 * ref.max_abs_ll
    assert ref.oracle_deviation <= bar and ref.oracle_best <= bar + pairs * 2.0 ** -52 * ref.max_abs_ll
    assert ref.tol == max(8 * ref.oracle_deviation, 2.0 ** -50 * ref.max_abs_ll)

    # 2. the order is decided
    assert gap >= psc.BITE * ref.tol

    # 3. the inputs bite: removing any row, or reading any column's neighbour in its place, moves some pair's sum
    assert np.all(rows[counted] >= psc.BITE * ref.tol)
    assert np.all(columns >= psc.BITE * ref.tol)
    assert np.all(counts[~counted] == 1) and not np.any(M[~counted]) and int(np.sum(~counted)) == case.empty
    # ... and the first and last row of the matrix, of every class, of every chunk and of every staged block of every work item is a
    # row that counts: a kernel that drops or doubles a row at an edge, or has a class end off by one, is seen
    perm, fast_end, mid_end = psc.device_rows(counts, noise)
    edges = sorted(psc.edge_rows(G, case.R, fast_end, mid_end, case.routes))
    assert {0, case.R - 1} <= set(edges) and all(r in edges for r in (fast_end - 1, fast_end, mid_end - 1, mid_end) if 0 <= r < case.R)
    assert np.all(counted[perm[edges]]) and np.all(rows[perm[edges]] >= psc.BITE * ref.tol)


def test_tiles_of_the_triangle_as_restated():
    """(the block heights and the tile ranges themselves: test_search_plan_header_gives_the_same_figures, against the header)"""
    for T in (1, 2, 16, 23, 256):
        assert [psc.tile_row_of_tile(psc.tile_row_start(ta, T), T) for ta in range(T)] == list(range(T))
        assert psc.tile_row_of_tile(psc.tile_row_start(T - 1, T), T) == T - 1 and psc.tile_row_start(T - 1, T) == T * (T + 1) // 2 - 1
    assert psc.item_sub_rows(64, 128) == 126     # the item of the last 8 tiles of 64 columns stages 16 columns


def test_search_plan_header_gives_the_same_figures(tmp_path):
    """tileSubRows and planTileRanges of search_plan.hpp itself, compiled for the host, against the restatement the cases are built
    on: every number of staged columns, every number of tiles up to 700 (tests/cpp/search_plan_check.cpp spells out the figures of
    the cases' column counts)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = tmp_path / "figures.cpp"
    lines = ['#include "search_plan.hpp"', "#include <cstdio>", "using namespace rpvg_search;", "int main() {",
             "  for (uint32_t n = 4; n <= 1024; n += 4) std::printf(\"s %u %u\\n\", n, tileSubRows(n));",
             "  for (uint32_t t = 1; t <= 700; ++t) { std::vector<std::pair<uint32_t, uint32_t> > r; planTileRanges(t, &r);",
             "    std::printf(\"r %u\", t); for (auto & x : r) std::printf(\" %u %u\", x.first, x.second); std::printf(\"\\n\"); }",
             "  return 0; }"]
    source.write_text("\n".join(lines))
    binary = tmp_path / "figures"
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(root, "rpvg_amd", "csrc"), str(source), "-o", str(binary)])
    seen = 0
    for line in subprocess.check_output([str(binary)], text=True).splitlines():
        words = line.split()
        if words[0] == "s":
            assert psc.tile_sub_rows(int(words[1])) == int(words[2]), line
        else:
            flat = [int(w) for w in words[2:]]
            assert psc.plan_tile_ranges(int(words[1])) == list(zip(flat[0::2], flat[1::2])), line
        seen += 1
    assert seen == 256 + 700


def _ends(name):
    M, noise, counts, _ = psc.BY_NAME[name].matrix()
    perm, fast_end, mid_end = psc.device_rows(counts, noise)
    return perm, fast_end, mid_end, counts[perm], noise[perm]


def test_row_class_cases_put_the_ends_where_their_names_say():
    for G, block in ((12, 126), (64, 46)):
        assert psc.first_sub_rows(G) == block
        R = psc.BY_NAME[f"classes_{G}_only_count_1"].R
        assert _ends(f"classes_{G}_no_count_1")[1] == 0
        assert _ends(f"classes_{G}_only_count_1")[1:3] == (R, R) and R > 2 * block and R % 2 == 1
        _, fast_end, mid_end, counts, _ = _ends(f"classes_{G}_no_logarithm_rows")
        assert 0 < fast_end < mid_end == len(counts)
        _, fast_end, mid_end, _, _ = _ends(f"classes_{G}_ends_inside_a_block")
        assert fast_end // block == mid_end // block == 1 and 0 < fast_end % block < mid_end % block
        _, fast_end, mid_end, counts, _ = _ends(f"classes_{G}_ends_on_block_edges")
        assert fast_end == block and mid_end == 3 * block and len(counts) > mid_end
        _, fast_end, mid_end, counts, _ = _ends(f"classes_{G}_ends_on_chunk_edges")
        assert (fast_end, mid_end) == (256, 512) and len(counts) > 512 and "chunk256" in psc.BY_NAME[f"classes_{G}_ends_on_chunk_edges"].routes
        _, fast_end, mid_end, counts, _ = _ends(f"classes_{G}_ends_in_different_chunks")
        assert fast_end // 256 == 0 and mid_end // 256 == 1 and len(counts) // 256 == 2
        _, fast_end, mid_end, counts, _ = _ends(f"classes_{G}_counts_8_and_9")
        assert set(counts[fast_end:mid_end]) == {8.0} and set(counts[mid_end:]) == {9.0} and counts[mid_end - 1] == 8 and counts[mid_end] == 9
        # noise exactly 2^-30: the product classes; one unit in the last place below: the logarithm class, count 1 included
        perm, fast_end, mid_end, counts, noise = _ends(f"classes_{G}_noise_at_the_floor")
        assert psc.SUB_FLOOR < psc.FLOOR == 2.0 ** -30 and np.nextafter(psc.SUB_FLOOR, 1.0) == psc.FLOOR
        assert np.sum(noise[:fast_end] == psc.FLOOR) == 24 and np.sum(noise[fast_end:mid_end] == psc.FLOOR) == 24
        assert np.sum(noise[mid_end:] == psc.SUB_FLOOR) == 48 and np.sum(noise[:mid_end] == psc.SUB_FLOOR) == 0
        assert sorted(counts[mid_end:][noise[mid_end:] == psc.SUB_FLOOR]) == [1.0] * 24 + [8.0] * 24
    assert psc.item_sub_rows(64, 128) == 126 and _ends("classes_64_ends_on_block_edges_of_126")[1:3] == (126, 252)
    assert _ends("classes_64_ends_on_chunk_edges_of_1024")[1:3] == (1024, 2048)
    _, fast_end, mid_end, counts, _ = _ends("classes_64_ends_in_different_chunks_of_1024")
    assert fast_end // 1024 == 0 and mid_end // 1024 == 1 and len(counts) // 1024 == 1


def test_fold_cases_run_the_products_through_the_folds():
    for G in (64, 65, 88):
        slices = psc.TILE_BLOCK // psc.plan_tile_ranges(psc.tile_count(G))[0][1]
        _, fast_end, _, counts, noise = _ends(f"folds_{G}_floor_run")
        run = 0
        while run < fast_end and noise[run] == psc.FLOOR:
            run += 1
        assert run >= 128 and run // slices > 2 * psc.FOLD_FACTORS, (G, run, slices)   # factors of ~2^-30 in a row, per lane
    assert psc.plan_tile_ranges(psc.tile_count(88)) == [(0, 253)]   # one slice: a lane of the item multiplies every row
    for k in range(22, 30):
        _, fast_end, mid_end, counts, noise = _ends(f"folds_88_count_8_arrives_at_{k}")
        assert fast_end % psc.FOLD_FACTORS == k and fast_end >= 128 and np.all(noise[:mid_end] == psc.FLOOR)
        assert list(counts[fast_end:mid_end]) == [8.0] * 6
        # (since_fold as pairTile2Item keeps it: k after the count-1 rows; a row of count 8 folds first when k + 8 > 30)
        since, arrivals = k, []
        for c in counts[fast_end:mid_end]:
            arrivals.append(since)
            since = (0 if since + c > psc.FOLD_FACTORS else since) + int(c)
        assert arrivals[0] == k and (k != 22 or arrivals[1] == 30)


def test_shapes_the_issue_lists_are_all_there():
    names = set(psc.BY_NAME)
    for G in (1, 2, 3, 4, 5, 8, 9, 20, 21, 28, 29, 61, 64, 65, 85, 88, 89, 92, 96, 97, 208, 209, 468, 469, 1024, 1025):
        case = psc.BY_NAME[f"cols_{G}"]
        assert case.G == G and (case.R == 2 * psc.first_sub_rows(G) + 1 if G < 1024 else case.R == 24)
    for G in (12, 64, 88):
        sr = psc.first_sub_rows(G)
        for R in (1, 2, sr - 1, sr, sr + 1, 255, 256, 257, 513, 1023, 1024, 1025, 2049):
            case = psc.BY_NAME[f"rows_{G}x{R}"]
            assert (case.G, case.R) == (G, R)
            assert ("chunk256" in case.routes) == (R in (255, 256, 257, 513))
    assert [psc.TILE_BLOCK // psc.plan_tile_ranges(psc.tile_count(G))[0][1] for G in (12, 64, 88)] == [42, 2, 1]
    # the sequential kernels: columns on both sides of 128, rows on both sides of 512 and of 2 048, on both routes
    for route in ("table", "walk"):
        shapes = [(c.G, c.R) for c in psc.cases_of(route)]
        assert any(G < 128 and R < 512 for G, R in shapes) and any(G > 128 and R < 512 for G, R in shapes)
        assert any(G < 128 and 512 < R < 2048 for G, R in shapes) and any(G > 128 and 512 < R < 2048 for G, R in shapes)
        assert any(G < 128 and R > 2048 for G, R in shapes) and any(G > 128 and R > 2048 for G, R in shapes)
    assert all("tiles" in c.routes for c in psc.CASES) and len(names) == len(psc.CASES)


def test_the_batch_holds_the_matrices_of_the_cases():
    picked = [psc.BY_NAME[n] for n in ("cols_5", "rows_12x127", "classes_12_noise_at_the_floor", "rows_64x2")]
    batch = psc.batch_of(picked)
    for k, case in enumerate(picked):
        cl = batch.cluster(k)
        M, noise, counts, mult = case.matrix()
        got, got_noise, got_counts = np_oracle.grouped_matrix(cl["rows"], [[p] for p in range(case.G)])
        assert np.array_equal(got, M) and np.array_equal(got_noise, noise) and np.array_equal(got_counts, counts)
        assert [p["source_count"] for p in cl["paths"]] == list(mult)
