"""The conditions the cases of tests/collapse_edge_cases.py have to meet before the device is asked anything
(tests/test_hip_collapse_edges.py), asserted on the model and the numpy restatement of the reference alone:

(a) outside the rounding-equal class any two values of one column are bit-identical or at least 1e-11 relative apart: the
    tolerant comparator (100 epsilon = 2.2e-14) is then an exact lexicographic order, and std::sort, sorted() and a rank from
    pairs cannot differ;
(b) every pair of rows has its largest column distance at most 0.9e-8 or at least 1.1e-8;
(c) collapse_heads reproduces oracle/np_oracle.read_collapse, merged rows and counts, on every case (oracle/pyoracle.py exposes
    no collapse of its own: the C++ oracle's runs inside its estimators, which the end-to-end tests of test_hip_collapse.py use);
(d) every case reaches its target, restated from the kernel's constants: list size and route, crowd size, deciding column,
    sorted positions, matrix rows;
(d') the cases of the held-back stage and of the EM problems reach theirs: rewritten rows per matrix, cells against slices, the
    log1p branch, two chunks of the tile kernel, no pair of columns dropped by the search; an uncollapsed EM solve differs from
    the collapsed one by more than the bar the device is held to;
(e) the cases bite: each of three deliberately wrong models changes a head on every case that names it, every model is named,
    and the cases that name none are the pure route cases.
"""
import numpy as np
import pytest

from oracle import np_oracle, pyoracle
from tests import collapse_edge_cases as cc

ALL = cc.CASES + cc.HELD_CASES + cc.EM_CASES
EXACT = [c for c in ALL if c.kind == "exact" and c.R]
IDS = lambda c: c.name  # noqa: E731


@pytest.mark.parametrize("case", EXACT, ids=IDS)
def test_a_values_of_a_column_are_identical_or_well_apart(case):
    P, _ = case.matrix()
    assert cc.column_gaps(P) >= cc.APART_RELATIVE, case.name


@pytest.mark.parametrize("case", EXACT, ids=IDS)
def test_b_no_pair_of_rows_near_the_precision(case):
    P, _ = case.matrix()
    below, above = cc.pair_distance_gap(P)
    assert below <= cc.CLOSE_BELOW and above >= cc.APART_ABOVE, (case.name, below, above)


@pytest.mark.parametrize("case", [c for c in ALL if c.R], ids=IDS)
def test_c_the_model_is_the_numpy_restatement(case):
    cluster = case.cluster()
    M, noise, counts = np_oracle.dense_matrix(cluster["rows"], case.G)
    Pn = np_oracle.add_noise_and_normalize(M, noise)
    P, cnt = case.matrix()
    assert Pn.tobytes() == P.tobytes() and np.array_equal(counts, cnt)   # the case's matrix is the restatement's, bit for bit
    want_rows, want_counts = np_oracle.read_collapse(Pn, counts, cc.PRECISION)
    got_rows, got_counts = cc.merged(P, cnt, cc.heads_of(case.name))
    assert got_rows.shape == want_rows.shape and got_rows.tobytes() == want_rows.tobytes(), case.name
    assert np.array_equal(got_counts, want_counts), case.name


def test_c_the_cpp_oracle_exposes_no_collapse_of_its_own():
    assert not [name for name in dir(pyoracle) if "collapse" in name.lower()]   # (one that appears belongs into condition (c))


@pytest.mark.parametrize("case", [c for c in ALL if c.R and "cells" not in c.name], ids=IDS)
def test_d_list_size_and_route(case):
    P, _ = case.matrix()
    if case.kind == "rounding":
        # every close pair is equal up to rounding: nothing is listed
        assert int(cc.close_partners(P).sum()) == 2 * len(case.raw)
        for (row, _), _ in case.raw.items():
            d = np.abs(P[row] - P[row - 1])
            assert np.any(d != 0) and np.all(d <= 0.5 * cc.EQUIVALENT_RELATIVE * np.minimum(P[row], P[row - 1])), (row, d)
        return
    listed = int(cc.close_partners(P).sum())
    assert listed == case.listed, (case.name, listed)
    most, _, most_maybe, _ = cc.window_candidates(P)
    assert (1 if most > cc.MAX_WINDOW_COMPARES else 0) == case.whole == (1 if most_maybe > cc.MAX_WINDOW_COMPARES else 0), (case.name, most, most_maybe)
    if case.whole:
        assert case.route == "whole"
    elif listed >= 2:
        assert case.route == cc.list_route(listed), (case.name, listed)
    else:
        assert case.route == "none"


def test_d_every_route_and_both_sides_of_every_threshold_are_reached():
    sizes = {c.listed for c in cc.CASES if not c.whole and c.route != "none"}
    for edge in (cc.LDS_TABLE_ROWS, cc.PAIRWISE_ROWS, cc.LIST_LDS_ROWS):
        assert {edge - 1, edge, edge + 1} <= sizes
    assert {c.route for c in cc.CASES} == set(cc.ROUTES) | {"whole", "none"}
    assert {cc.list_route(n) for n in (128, 129, 1024, 1025, 2048, 2049)} == set(cc.ROUTES)
    assert {c.R for c in cc.CASES} >= {0, 1, 2, 512, 513, 1024, 1025, 2048, 2049, 4097}
    assert {c.G for c in cc.CASES} >= {1, 2, 8, 9, 63, 64, 65, 70}
    assert max(c.R for c in cc.CASES) == 4097
    # forEachColumnPair: a batch of kBatch columns exactly, one more, and deciding columns on both sides of both of its edges
    assert {cc.BATCH, cc.BATCH + 1, cc.PATTERN_COLUMNS - 1, cc.PATTERN_COLUMNS, cc.PATTERN_COLUMNS + 1} <= set(cc.COLUMN_COUNTS)
    decided = {c for case in cc.CASES for c in case.columns.values()}
    assert {0, cc.BATCH - 1, cc.BATCH, cc.PATTERN_COLUMNS - 1, cc.PATTERN_COLUMNS, max(cc.COLUMN_COUNTS) - 1} <= decided


def test_d_the_crowds_stand_on_either_side_of_the_window_limit():
    got = {}
    for size in cc.CROWD_SIZES:
        case = cc.BY_NAME[f"crowd_{size}"]
        P, _ = case.matrix()
        most, pairs, most_maybe, pairs_maybe = cc.window_candidates(P)
        # the lowest row of the crowd lists the rest of it and nothing else, whichever way the keys are cut to quanta
        assert most == most_maybe == size - 1, (size, most, most_maybe)
        assert pairs == pairs_maybe == size * (size - 1) // 2
        got[size] = case.whole
        head = cc.heads_of(case.name)
        assert cc.replaced_rows(P, head) == size - 1
    assert sorted(got.values()) == [0, 1] and cc.CROWD_SIZES[0] - 1 == cc.MAX_WINDOW_COMPARES
    # in the joint call the candidate pairs of all matrices fit the pair buffer (a full buffer sends a matrix to the whole sort, too);
    # a crowd alone does not fit its call's: alone, both crowds are sorted whole
    joint = [cc.CASES[k] for k in cc.joint_listing()]
    total = sum(cc.window_candidates(c.matrix()[0])[3] for c in joint if c.R)
    assert total <= cc.pair_capacity(sum(c.R for c in joint)), total
    for size in cc.CROWD_SIZES:
        assert size * (size - 1) // 2 > cc.pair_capacity(cc.BY_NAME[f"crowd_{size}"].R)


@pytest.mark.parametrize("case", [c for c in cc.CASES if c.columns or c.order_columns], ids=IDS)
def test_d_deciding_columns(case):
    P, _ = case.matrix()
    for (a, b), c in case.columns.items():
        assert cc.deciding_column(P, a, b) == c, (case.name, a, b, c)
    for (a, b), c in case.order_columns.items():
        assert cc.first_differing_column(P, a, b) == c, (case.name, a, b, c)
    if case.name.startswith("columns_") and case.G > 1:
        want = {c for c in (0, 7, 8, 63, 64, case.G - 1) if c < case.G}
        assert set(case.columns.values()) == (want if case.G > 2 else set()) and {int(n.split("_")[1]) for n in case.marks if n[-1].isdigit()} == want
        head = cc.heads_of(case.name)
        for name, rows in case.marks.items():
            a, b = rows
            joined = head[a] == head[b]
            assert joined == (not name.endswith("apart") and not name.startswith("apart")), (case.name, name)
        a, b = case.marks["count"]
        assert P[a].tobytes() == P[b].tobytes()
        for name in ("noise_close", "noise_apart"):
            a, b = case.marks[name]
            assert case.rows[a][0] == case.rows[b][0] and case.rows[a][1] != case.rows[b][1]
        for name in ("single_close", "single_apart"):
            a, b = case.marks[name]
            assert np.count_nonzero(P[a, :-1]) == 1 and np.count_nonzero(P[b, :-1]) == 1


def test_d_columns_of_one():
    case = cc.BY_NAME["columns_1"]
    P, _ = case.matrix()
    head = cc.heads_of(case.name)
    a, b = case.marks["noise_close"]
    assert head[a] == head[b]
    a, b = case.marks["noise_apart"]
    assert head[a] != head[b]
    a, b = case.marks["count"]
    assert P[a].tobytes() == P[b].tobytes() and head[a] == head[b]


def _positions(case):
    P, counts = case.matrix()
    order = cc.tolerant_order(P, counts)
    where = np.zeros(case.R, dtype=np.int64)
    where[order] = np.arange(case.R)
    return P, where


@pytest.mark.parametrize("stretch", [False, True])
def test_d_runs_across_the_sorted_edges(stretch):
    case = cc.BY_NAME["sorted_edges_stretches" if stretch else "sorted_edges_pairs"]
    P, where = _positions(case)
    head = cc.heads_of(case.name)
    for edge in cc.SORTED_EDGES:
        rows = case.marks[f"edge_{edge}"]
        first = edge - 2 if stretch else edge - 1
        assert sorted(int(where[r]) for r in rows) == list(range(first, first + len(rows))), (edge, where[list(rows)])
        assert len({int(head[r]) for r in rows}) == 1   # one run
        if stretch:
            assert all(P[r].tobytes() == P[rows[0]].tobytes() for r in rows[:-1]) and where[rows[-1]] == edge + 1
    assert case.R > 2048   # its rows are sorted in two chunks


def test_d_the_pair_at_the_ends_of_the_matrix():
    case = cc.BY_NAME["ends"]
    P, counts = case.matrix()
    assert case.marks["pair"] == (0, case.R - 1) and list(cc.matrix_row_order(counts, P[:, -1])) == list(range(case.R))
    head = cc.heads_of(case.name)
    assert head[case.R - 1] == 0


def test_d_ladders_join_their_heads_not_their_predecessors():
    case = cc.BY_NAME["ladders"]
    P, counts = case.matrix()
    head = cc.heads_of(case.name)
    order = cc.tolerant_order(P, counts)
    runs = [sum(1 for r in order if head[r] == h) for h in order if head[h] == h]
    # a ladder of n rungs 0.6e-8 apart: runs of two (rung k + 1 is close to rung k, rung k + 2 is not), a single rung left over
    want = []
    for rungs in range(2, 10):
        want += [2] * (rungs // 2) + [1] * (rungs % 2)
    assert runs == want


def test_d_rows_in_between():
    case = cc.BY_NAME["between"]
    P, where = _positions(case)
    head = cc.heads_of(case.name)
    active = cc.close_partners(P)
    for name, (a, b, x) in case.marks.items():
        assert active[a] and active[b] and not active[x], name
        parted = name in ("between_shared", "zero_behind")
        assert (where[a] < where[x] < where[b]) == parted, name
        assert (head[b] == a) == (not parted) and head[a] == a and head[x] == x, name
        shares = np.array_equal(P[x, :3] != 0, P[a, :3] != 0)   # the zero pattern in front of the deciding column
        assert shares == (name != "other_pattern"), name
    a, b, x = case.marks["outside"]
    assert where[x] == where[b] + 1       # one position outside the pair
    a, b, x = case.marks["below"]
    assert where[x] == where[a] - 1
    a, b, x = case.marks["zero_behind"]
    assert P[a, 4] == 0 and P[b, 4] == 0 and P[x, 4] != 0


def test_d_rows_in_between_at_the_edges_of_the_pass():
    case = cc.BY_NAME["between_rows"]
    P, counts = case.matrix()
    _, where = _positions(case)
    head = cc.heads_of(case.name)
    active = cc.close_partners(P)
    listed = [r for r in cc.tolerant_order(P, counts) if active[r]]
    a, b, c = case.marks["triple"]
    # the triple's neighbour pairs are the last of one chunk of kPairChunk pairs and the first of the next (pairs 1 .. 256, 257 ..)
    assert [listed.index(r) for r in (a, b, c)] == [cc.PAIR_CHUNK - 1, cc.PAIR_CHUNK, cc.PAIR_CHUNK + 1]
    x1, x2, x3 = case.marks["between"]
    rows = list(cc.matrix_row_order(counts, P[:, -1]))
    assert [rows.index(x) for x in (x1, x2, x3)] == [cc.BETWEEN_ROWS - 1, cc.BETWEEN_ROWS, cc.BETWEEN_ROWS + 1]
    assert not active[x1] and not active[x2] and not active[x3]
    assert where[a] < where[x1] < where[b] < where[x2] < where[c]
    p, q = case.marks["pair"]
    assert where[p] < where[x3] < where[q]
    assert all(head[r] == r for r in (a, b, c, p, q))
    assert cc.replaced_rows(P, head) == (600 - 5) // 2 + 1   # every other pair joins, and the triple at the front twice


@pytest.mark.parametrize("R", [r for r in cc.ROW_COUNTS if r >= 16])
def test_d_matrices_of_every_size_hold_a_ladder_and_a_row_in_between(R):
    case = cc.BY_NAME[f"rows_{R}"]
    P, _ = case.matrix()
    assert case.R == R and cc.replaced_rows(P, cc.heads_of(case.name)) == 3


@pytest.mark.parametrize("which", cc.WRONG_MODELS)
def test_e_a_wrong_model_changes_a_head_on_every_case_that_names_it(which):
    named = [c for c in cc.CASES if which in c.bites]
    assert named, which
    for case in named:
        P, counts = case.matrix()
        assert not np.array_equal(cc.wrong_heads(P, counts, which), cc.heads_of(case.name)), (which, case.name)


def test_e_the_cases_without_a_wrong_model_are_the_route_cases():
    unnamed = {c.name for c in cc.CASES if not c.bites}
    route = {c.name for c in cc.CASES if c.name.startswith(("list_", "crowd_", "sorted_edges_", "ends", "no_rows", "rounding_equal"))}
    route |= {f"rows_{r}" for r in (1, 2)} | {f"columns_{g}" for g in cc.COLUMN_COUNTS if g <= cc.PATTERN_COLUMNS}
    assert unnamed == route, unnamed ^ route


# ---- (d') the held-back stage and the EM problems ---------------------------------------------------------------------------------------

def _collapsed(case):
    P, counts = case.matrix()
    head = cc.heads_of(case.name)
    return P, counts, head, P[head]


def test_d_held_back_shapes():
    from tests import pair_search_cases as psc
    assert psc.CHUNK_ROWS == cc.SEARCH_CHUNK_ROWS
    rewritten = {}
    for case in cc.HELD_CASES:
        P, counts, head, Pc = _collapsed(case)
        rewritten[case.name] = cc.replaced_rows(P, head)
        model = psc.pair_model(np.ascontiguousarray(Pc[:, :-1]), np.ascontiguousarray(Pc[:, -1]), counts, case.multiplicities())
        assert max(psc.spreads(model)) <= psc.MAX_SPREAD, case.name   # the search keeps every pair of columns
        assert cc.window_candidates(P)[2] <= cc.MAX_WINDOW_COMPARES
    for G, n in cc.HELD_SHAPES:
        assert rewritten[f"held_{G}x{n}"] == n
    counts_of = sorted(n for _, n in cc.HELD_SHAPES)
    assert {cc.STAGE_ROWS - 1, cc.STAGE_ROWS, cc.STAGE_ROWS + 1} <= set(counts_of)
    cells = sorted(G * G for G, _ in cc.HELD_SHAPES)
    assert cells[0] < cc.ADJUST_SLICES <= cells[-2] and cells[-1] > cc.ADJUST_SLICES and {G for G, _ in cc.HELD_SHAPES} == {1, 3, 4, 5}


def test_d_held_back_log1p_branch_next_to_the_series():
    case = cc.BY_NAME["held_log1p"]
    P, counts, head, Pc = _collapsed(case)

    def x_of(r, a, b):   # the relative change of the search's log argument of cell (a, b): adjustSearchSums
        before = P[r, -1] + (P[r, a] + P[r, b]) / 2
        after = Pc[r, -1] + (Pc[r, a] + Pc[r, b]) / 2
        return abs(after - before) / before

    moved = [r for r in range(case.R) if head[r] != r]
    planted = {r for pair in case.marks["log1p"] for r in pair}
    big = [r for r in moved if r in planted]
    assert len(big) == cc.LOG1P_ROWS and len(moved) > len(big)
    for r in big:
        assert 0.9e-5 < P[r, 1] < 1.2e-5 and 4.9e-9 < abs(P[r, 1] - Pc[r, 1]) < 5.1e-9
        assert x_of(r, 1, 1) > 1e-4 and x_of(r, 0, 1) > 1e-4 and x_of(r, 2, 2) < 1e-4   # both branches on one row
    for r in moved:
        if r not in planted:
            assert max(x_of(r, a, b) for a in range(3) for b in range(a, 3)) < 1e-4


def test_d_held_back_rows_in_two_chunks():
    case = cc.BY_NAME["held_chunks"]
    P, counts, head, _ = _collapsed(case)
    assert list(cc.matrix_row_order(counts, P[:, -1])) == list(range(case.R))   # the matrix keeps the cluster's order
    moved = sorted(r for r in range(case.R) if head[r] != r)
    assert {r // cc.SEARCH_CHUNK_ROWS for r in moved} == {0, 1}
    a, b = case.marks[f"row_{cc.SEARCH_CHUNK_ROWS - 1}"]
    assert (a, b) == (cc.SEARCH_CHUNK_ROWS - 1, cc.SEARCH_CHUNK_ROWS) and (head[b] == a or head[a] == b)


@pytest.mark.parametrize("case", cc.EM_CASES, ids=IDS)
def test_d_an_uncollapsed_em_solve_differs_by_more_than_the_bar(case):
    from tests import small_cases
    P, counts = case.matrix()
    Pc, merged_counts = np_oracle.read_collapse(P, counts, cc.PRECISION)
    assert len(merged_counts) < len(counts)
    collapsed = pyoracle.em_dense(Pc, merged_counts)
    plain = pyoracle.em_dense(P, counts)
    assert np.count_nonzero(collapsed[0]) >= 2   # two paths keep an abundance
    assert not small_cases.rel_close(plain[0], collapsed[0], rel=10 * cc.EM_BAR, floor=0.0), (plain[0], collapsed[0])


def test_d_the_stretch_of_equal_cells_is_not_a_stretch_of_equal_bits():
    case = cc.BY_NAME["em_cells"]
    P, counts = case.matrix()
    stretch = sorted({r for (r, _) in case.raw})
    cells = np.floor(P[stretch] * 2.0 ** 44)
    assert len(stretch) == 40 and np.all(cells == cells[0]) and len({P[r].tobytes() for r in stretch}) >= 4
    head = cc.collapse_heads(P, counts)
    assert len({int(head[r]) for r in stretch}) == 1 and int(np.sum(head == head[stretch[0]])) == 41   # one run, the satellite in it
