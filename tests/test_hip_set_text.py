"""The set text on the GPU (rpvg_amd/csrc/set_text.hip, rpvg_hip_estimates_set_text of include/rpvg_hip.h) against the plain-Python
model of tests/set_text_model.py, which tests/test_set_text_model.py pins to hand-written rows and to the writers' own bytes.  Every
byte and every row_off is compared: there is no tolerance.  The TPMs a row prints are the resident table's (its view), which
tests/test_hip_estimates_table.py holds to its model."""
import math

import numpy as np
import pytest

from rpvg_amd import hip
from rpvg_amd.estimates_table import EstimatesTable, FlatEstimates
from rpvg_amd.table_text import JOINT, POSTERIOR, Labels, TableText
from tests import estimates_table_model as EM
from tests import set_text_model as S
from tests import table_text_model as M

pytestmark = pytest.mark.gpu

KINDS = [JOINT, POSTERIOR]


def assert_text(text, want_bytes, want_off):
    """The view of a device text against the model's bytes and offsets; the guards around the text on the device are intact."""
    got = text.view()
    assert got["row_off"].tolist() == [int(x) for x in want_off]
    assert got["num_bytes"] == len(want_bytes) and got["num_rows"] == int(np.count_nonzero(np.diff(np.asarray(want_off, dtype=np.int64))))
    if got["bytes"] != want_bytes:
        at = next(i for i in range(min(len(want_bytes), len(got["bytes"]))) if got["bytes"][i] != want_bytes[i])
        raise AssertionError(f"byte {at}: {got['bytes'][max(at - 30, 0):at + 30]!r} != {want_bytes[max(at - 30, 0):at + 30]!r}")
    assert text.guards_intact()
    return got


def table_of(ctx, clusters, ploidy, denominator=1.0):
    """(flat, table, member_tpm): the resident table of the clusters, with TPMs when a denominator is given."""
    flat = FlatEstimates(**EM.flatten(clusters))
    table = EstimatesTable.build(ctx, None, flat, ploidy)
    member_tpm = None
    if denominator is not None:
        table.tpm(denominator)
        member_tpm = table.view()["member_tpm"]
    return flat, table, member_tpm


def check_sets(ctx, clusters, names, ids, kind, ploidy, min_posterior, precision=8, denominator=1.0):
    flat, table, member_tpm = table_of(ctx, clusters, ploidy, denominator)
    try:
        want_bytes, want_off = S.set_text(kind, EM.flatten(clusters), member_tpm, names, ids, ploidy, min_posterior, precision)
        text = TableText.sets(ctx, table, flat.as_c(), Labels.of(names, ids), kind, ploidy, min_posterior, precision)
        try:
            return assert_text(text, want_bytes, want_off)
        finally:
            text.free()
    finally:
        table.free()


def names_for(clusters, lengths=None, seed=0):
    P = sum(c["num_paths"] for c in clusters)
    lengths = lengths or S.NAME_LENGTHS
    return M.names_of_lengths([lengths[i % len(lengths)] for i in range(P)], seed=seed)


# ---- both kinds at every ploidy -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ploidy", [1, 2, 3, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_every_set_size_at_every_ploidy(hip_ctx, kind, ploidy):
    """Set sizes 1 .. ploidy all present (every pad count), members unsorted and repeated, in three clusters with an empty one between
    them; names of 0 to 255 bytes, so rows start at every residue modulo 4."""
    rng = np.random.default_rng(100 + ploidy)
    clusters = [S.every_size_cluster(ploidy, 9, rng), S.cluster_of_sets([], [], 0, rng), S.every_size_cluster(ploidy, 8, rng), S.every_size_cluster(ploidy, 2, rng)]
    got = check_sets(hip_ctx, clusters, names_for(clusters), [3, 1, 4000000000, 12], kind, ploidy, 0.0)
    S_total = sum(len(c["sets"]) for c in clusters)
    assert got["num_rows"] == S_total == 9 * ploidy and len(got["row_off"]) == S_total + 1
    assert {int(x) % 4 for x in got["row_off"][:-1]} == {0, 1, 2, 3}
    assert (ploidy == 1) == (b"\t.\t" not in got["bytes"])
    if kind == JOINT and ploidy > 1:
        assert b"\t0\t0" * (ploidy - 1) + b"\n" in got["bytes"]


@pytest.mark.parametrize("kind", KINDS)
def test_a_row_of_eight_names_of_255_bytes(hip_ctx, kind):
    """More than one step of the staging block in one row: 8 x 256 bytes of names, then the numbers."""
    rng = np.random.default_rng(7)
    sets = [[3, 1, 2, 0, 3, 3, 1, 0], [2], [0, 1, 2, 3, 0, 1, 2, 3]]
    clusters = [S.cluster_of_sets(sets, [0.5, 0.25, 0.125], 4, rng)]
    names = M.names_of_lengths([255] * 4, seed=2)
    got = check_sets(hip_ctx, clusters, names, [5], kind, 8, 0.0)
    assert int(got["row_off"][1]) > 8 * 256 and got["num_rows"] == 3


# ---- the filter ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_the_filter_is_the_writers_comparison(hip_ctx, kind):
    """posterior == min_posterior is printed, one ulp below is dropped, +0.0 and -0.0 are printed at min_posterior 0 and dropped above
    it, NaN of either sign is always printed; dropped rows first, last and adjacent; a cluster whose sets are all dropped and a
    cluster without sets."""
    rng = np.random.default_rng(8)
    below = float(np.nextafter(0.25, 0.0))
    first = S.cluster_of_sets([[0], [1, 0], [1, 1], [0, 1], [1], [0], [0, 0]], [below, 0.25, 0.0, -0.0, M.NAN, M.NEG_NAN, 0.5], 2, rng)
    all_dropped = S.cluster_of_sets([[0], [0, 0]], [0.1, below], 1, rng)
    empty = S.cluster_of_sets([], [], 3, rng)
    last = S.cluster_of_sets([[2, 0], [1]], [1.0, 0.2], 3, rng)
    clusters = [first, all_dropped, empty, last]
    names, ids = names_for(clusters, [4, 7, 2]), [1, 2, 3, 4]
    got = check_sets(hip_ctx, clusters, names, ids, kind, 2, 0.25)
    lengths = np.diff(got["row_off"].astype(np.int64))
    assert [bool(n) for n in lengths] == [False, True, False, False, True, True, True, False, False, True, False]
    assert b"\tnan" in got["bytes"] and b"\t-nan" in got["bytes"] and got["num_rows"] == 5
    got = check_sets(hip_ctx, clusters, names, ids, kind, 2, 0.0)
    assert got["num_rows"] == 11 and b"\t1\t-0" in got["bytes"] and b"\t1\t0" in got["bytes"]
    got = check_sets(hip_ctx, clusters, names, ids, kind, 2, 2.0)     # every finite posterior lies below: the two NaN rows are left
    assert got["num_rows"] == 2
    got = check_sets(hip_ctx, [all_dropped, empty], names_for([all_dropped, empty], [3]), [1, 2], kind, 2, 0.25)   # no row at all
    assert got["num_bytes"] == 0 and got["bytes"] == b"" and got["row_off"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("kind", KINDS)
def test_no_set_and_no_cluster(hip_ctx, kind):
    rng = np.random.default_rng(9)
    clusters = [S.cluster_of_sets([], [], 2, rng)]
    got = check_sets(hip_ctx, clusters, ["a", "b"], [1], kind, 2, 0.0)
    assert got["num_bytes"] == 0 and got["row_off"].tolist() == [0]
    got = check_sets(hip_ctx, [], [], [], kind, 2, 0.0)
    assert got["num_bytes"] == 0 and got["row_off"].tolist() == [0]


# ---- hard cells ----------------------------------------------------------------------------------------------------------------------

def abundance_whose_tpm_is(value):
    """x with fl(x * 1e6) == value (the TPM of an abundance x at effective length 1 and denominator 1), or None."""
    x = value / 1e6
    for candidate in (x, float(np.nextafter(x, math.inf)), float(np.nextafter(x, -math.inf))):
        if candidate * 1e6 == value:
            return candidate
    return None


def tpm_ties(precision):
    """Abundances whose TPMs are ties of both parities at `precision` digits: k + 0.5 at 8, (2 k + 1) / 4 .. at 17 digits."""
    found, k = {}, 0
    while len(found) < 2 and k < 10000:
        value = (10000000.5 + k) if precision == 8 else (1125899906842624.25 + 0.5 * k)   # 8 digits: halves; 17 digits at 2^50: quarters
        tie, parity = M.is_tie(value, precision)
        x = abundance_whose_tpm_is(value) if tie else None
        if x is not None and parity not in found:
            found[parity] = x
        k += 1
    assert len(found) == 2
    return [found[0], found[1]]


@pytest.mark.parametrize("precision", [8, 17])
def test_hard_cells_in_every_numeric_column(hip_ctx, precision):
    """Ties of both parities, a carry into the next power of ten (at 8 digits 9.99999995e+99, whose cell grows to 1e+100; at 17 digits
    the double below 10^98, the exponent 100 having no such double), -0.0, a subnormal, inf and the longest cell as posterior, as
    abundance and as TPM (effective length 1 and denominator 1: TPM = abundance * 1e6, with abundances chosen for their TPMs)."""
    rng = np.random.default_rng(10)
    ties = M.TIES_8 if precision == 8 else M.TIES_17
    carry, carry_text = (9.99999995e+99, "1e+100") if precision == 8 else (1e+98, "1e+98")
    assert M.fmt(carry, precision) == carry_text and abundance_whose_tpm_is(carry) is not None
    hard = ties + [carry, 99999999.5, -0.0, 5e-324, math.inf, M.LONGEST[0], M.LONGEST[1], 1e-5]
    for_tpm = tpm_ties(precision) + [abundance_whose_tpm_is(carry), -0.0, 5e-324, math.inf, M.LONGEST[1], -2e-314]
    sets = [[i % 3, (i + 1) % 3] for i in range(len(hard))]
    abundances = []
    for i, v in enumerate(hard):
        abundances += [v, for_tpm[i % len(for_tpm)]]
    cluster = S.cluster_of_sets(sets, hard, 3, rng, abundances=abundances)
    cluster["eff"] = [1.0, 1.0, 1.0]
    names, ids = ["a", "bb", "ccc"], [1]
    flat, table, member_tpm = table_of(hip_ctx, [cluster], 2, 1.0)
    table.free()
    assert all(member_tpm[2 * i + 1] == abundances[2 * i + 1] * 1e6 for i in range(len(hard)))
    cells = {JOINT: list(hard) + list(abundances) + [float(v) for v in member_tpm], POSTERIOR: list(hard)}
    for kind in KINDS:
        hip_ctx.reset_stats()
        got = check_sets(hip_ctx, [cluster], names, ids, kind, 2, -math.inf, precision)
        assert got["num_rows"] == len(hard)
        num_ties = sum(1 for v in cells[kind] if math.isfinite(v) and v != 0 and M.is_tie(v, precision)[0])
        assert num_ties >= (6 if kind == JOINT else 2) and hip_ctx.stats()["text_exact_cells"] >= num_ties
        assert max(len(M.fmt(v, precision)) for v in cells[kind]) == (15 if precision == 8 else 24)
    tpm_cells = [float(v) for v in member_tpm]
    assert {M.is_tie(v, precision)[1] for v in tpm_cells if math.isfinite(v) and v != 0 and M.is_tie(v, precision)[0]} == {0, 1}
    assert any(M.fmt(v, precision) == "-0" for v in tpm_cells) and any(M.fmt(v, precision) == "inf" for v in tpm_cells)
    assert any(M.fmt(v, precision) == carry_text for v in tpm_cells) and any(0 < abs(v) < 2.2e-308 for v in tpm_cells)
    assert max(len(M.fmt(v, precision)) for v in tpm_cells) == (15 if precision == 8 else 24)


def test_exact_cells_are_counted_for_ties_alone(hip_ctx):
    rng = np.random.default_rng(11)
    cluster = S.cluster_of_sets([[0, 1], [1], [1, 1]], [0.5, 0.25, 0.125], 2, rng, abundances=[3.0, 7.0, 11.0, 1.0, 2.0])
    cluster["eff"] = [1.0, 1.0]
    hip_ctx.reset_stats()
    check_sets(hip_ctx, [cluster], ["a", "b"], [1], JOINT, 2, 0.0)
    assert hip_ctx.stats()["text_exact_cells"] == 0
    cluster["abundances"] = [10000000.5, 7.0, 10000001.5, 1.0, 2.0]
    cluster["posteriors"] = [0.5, 0.25, 123456785.0]
    check_sets(hip_ctx, [cluster], ["a", "b"], [1], JOINT, 2, 0.3)     # the middle set is dropped: its cells are not counted
    assert hip_ctx.stats()["text_exact_cells"] == 3
    check_sets(hip_ctx, [cluster], ["a", "b"], [1], POSTERIOR, 2, 0.0)
    assert hip_ctx.stats()["text_exact_cells"] == 4


# ---- inputs the posterior kind does not need ------------------------------------------------------------------------------------------

def test_posterior_rows_without_abundances_and_without_tpms(hip_ctx):
    """A `haplotypes` result: num_abundances = 0 and a table that never had its TPMs."""
    rng = np.random.default_rng(12)
    clusters = [S.every_size_cluster(3, 4, rng, with_abundances=False), S.every_size_cluster(3, 2, rng, with_abundances=False)]
    assert FlatEstimates(**EM.flatten(clusters)).sizes()["num_abundances"] == 0
    got = check_sets(hip_ctx, clusters, names_for(clusters), [8, 9], POSTERIOR, 3, 0.3, denominator=None)
    assert 0 < got["num_rows"] < 18


# ---- equal bytes across routes --------------------------------------------------------------------------------------------------------

def test_device_arrays_two_builds_and_ranges(hip_ctx):
    """Host arrays against device arrays (labels too), two builds, and rpvg_hip_table_text_get on ranges that split a row."""
    rng = np.random.default_rng(13)
    clusters = [S.every_size_cluster(3, 5, rng), S.every_size_cluster(3, 3, rng)]
    names, ids = names_for(clusters), [21, 22]
    flat, table, member_tpm = table_of(hip_ctx, clusters, 3, 2.5)
    labels = Labels.of(names, ids)
    pointers, label_pointers = {}, {}
    try:
        for source, into in ((flat, pointers), (labels, label_pointers)):
            for name, _ in source._FIELDS:
                a = getattr(source, name)
                into[name] = hip_ctx.malloc(max(a.nbytes, 8))
                if a.nbytes:
                    hip_ctx.h2d(into[name], a)
        for kind in KINDS:
            want_bytes, want_off = S.set_text(kind, EM.flatten(clusters), member_tpm, names, ids, 3, 0.2)
            for estimates, source in ((flat.as_c(), labels), (flat.as_c(), labels), (flat.as_c(device_pointers=pointers), labels.as_c(device_pointers=label_pointers)),
                                      (flat.as_c(), labels.as_c(device_pointers=label_pointers))):
                text = TableText.sets(hip_ctx, table, estimates, source, kind, 3, 0.2)
                try:
                    assert_text(text, want_bytes, want_off)
                    n = len(want_bytes)
                    inside = next(int(want_off[r]) + 1 for r in range(len(want_off) - 1) if want_off[r + 1] > want_off[r])   # inside the first printed row
                    for begin, end in ((0, n), (1, n - 1), (7, 7), (n, n), (inside, inside + 1), (inside, n - 2)):
                        assert text.bytes(begin, end) == want_bytes[begin:end]
                    with pytest.raises(hip.EngineError, match=r"\(-3\)"):
                        text.bytes(1, n + 1)
                finally:
                    text.free()
    finally:
        table.free()
        for p in list(pointers.values()) + list(label_pointers.values()):
            hip_ctx.free(p)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_a_usable_context(hip_ctx):
    rng = np.random.default_rng(14)
    good = [S.cluster_of_sets([[0]], [0.5], 2, rng), S.cluster_of_sets([[0, 1], [1]], [0.5, 0.25], 2, rng), S.cluster_of_sets([[1, 1]], [1.0], 3, rng)]
    names, ids = names_for(good, [4, 5, 6]), [7, 8, 9]
    labels = Labels.of(names, ids)

    def refused(table, flat, kind, match, ploidy=2, precision=8, with_labels=None):
        with pytest.raises(hip.EngineError, match=match):
            TableText.sets(hip_ctx, table, flat.as_c() if isinstance(flat, FlatEstimates) else flat, with_labels or labels, kind, ploidy, 0.0, precision)

    flat, table, _ = table_of(hip_ctx, good, 2, 1.0)
    other_ploidy = EstimatesTable.build(hip_ctx, None, flat, 3)
    without_tpm = EstimatesTable.build(hip_ctx, None, flat, 2)
    try:
        other_ploidy.tpm(1.0)
        # the same numbers of clusters, paths and members as the table's: a set of size 0 and a set of size ploidy + 1 in cluster 1
        for sets, posteriors in (([[0, 1, 1], []], [0.5, 0.25]), ([[0, 1, 1]], [0.5]), ([[], [0, 1, 1]], [0.5, 0.25])):
            broken = list(good)
            broken[1] = dict(good[1], sets=[tuple(s) for s in sets], posteriors=posteriors)
            for kind in KINDS:
                refused(table, FlatEstimates(**EM.flatten(broken)), kind, r"\(-3\).*cluster 1: a set whose size is not in 1 \.\. ploidy")
        stray = list(good)
        stray[2] = dict(good[2], sets=[(1, 3)])
        refused(table, FlatEstimates(**EM.flatten(stray)), POSTERIOR, r"\(-3\).*cluster 2: a set member that is not a path of the cluster")
        for kind in KINDS:
            refused(table, flat, kind, r"\(-3\).*ploidy outside 1 \.\. 8", ploidy=0)
            refused(table, flat, kind, r"\(-3\).*ploidy outside 1 \.\. 8", ploidy=9)
            refused(table, flat, kind, r"\(-3\).*precision outside 1 \.\. 17", precision=0)
            refused(table, flat, kind, r"\(-3\).*precision outside 1 \.\. 17", precision=18)
            refused(table, flat, kind, r"\(-3\).*labels of 4 paths", with_labels=Labels.of(names[:4], ids))
            refused(table, flat, kind, r"\(-3\).*in 2 clusters", with_labels=Labels.of(names, ids[:2]))
            descending = Labels.of(names, ids)
            descending.name_off[2] = descending.name_off[1] - 1
            refused(table, flat, kind, r"\(-3\).*path 1: name_off", with_labels=descending)
            short = Labels.of(names, ids)
            refused(table, flat, kind, r"\(-3\).*path 6: name_off", with_labels=short.as_c(num_name_bytes=len(short.name_bytes) - 1))
        refused(table, flat, 1, r"\(-3\).*no such kind")
        refused(without_tpm, flat, JOINT, r"\(-3\).*no TPMs")
        refused(other_ploidy, flat, JOINT, r"\(-3\).*built for ploidy 3")
        fewer = FlatEstimates(**EM.flatten(good[:2]))
        refused(table, fewer, POSTERIOR, r"\(-3\).*not that of the estimates")
        for lenient in (without_tpm, other_ploidy):       # the posterior rows need neither
            text = TableText.sets(hip_ctx, lenient, flat.as_c(), labels, POSTERIOR, 2, 0.0)
            text.free()
    finally:
        table.free()
        other_ploidy.free()
        without_tpm.free()
    # joint from a cluster without abundances: the table takes such a cluster, the joint rows do not
    bare = list(good)
    bare[1] = dict(good[1], abundances=[])
    bare_flat, bare_table, _ = table_of(hip_ctx, bare, 2, 1.0)
    try:
        refused(bare_table, bare_flat, JOINT, r"\(-3\).*cluster 1: not one abundance per set member")
        text = TableText.sets(hip_ctx, bare_table, bare_flat.as_c(), labels, POSTERIOR, 2, 0.0)
        text.free()
    finally:
        bare_table.free()
    for kind in KINDS:                                     # the context is usable afterwards
        check_sets(hip_ctx, good, names, ids, kind, 2, 0.0)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def test_end_to_end(tmp_path):
    """Engine.run on the small_cases batch of the tables' own end-to-end tests, one table per writer.  haplotype-transcripts (ploidy
    2): EstimatesTable, TableText.sets and addText() into a file give the bytes JointHaplotypeAbundanceEstimatesWriter::addEstimates
    writes from the containers, header and `Unknown` row included.  haplotypes: the same for JointHaplotypeEstimatesWriter, whose
    file has a header and no `Unknown` row.  Each text is the host line's."""
    from rpvg_amd import engine as eng_mod
    from rpvg_amd.batch import ClusterBatch, make_params
    from rpvg_amd.estimates_table import HarnessTable, write_from_containers
    from rpvg_amd.table_text import HarnessTableText
    from tests import small_cases

    batch = ClusterBatch.from_clusters(small_cases.make_batch_clusters(4242, n_clusters=8, with_empty=True))
    params = make_params()
    engine = eng_mod.Engine(0)
    try:
        prepared = engine.prepare(batch)
        try:
            for model, kind, writer, suffix in (("haplotype-transcripts", JOINT, "joint", "_joint.txt"), ("haplotypes", POSTERIOR, "posterior", ".txt")):
                engine.run(model, params, prepared)
                total = write_from_containers(prepared, "", params.ploidy, "")[0] if kind == JOINT else 0.0   # a haplotypes result has no abundances to sum
                write_from_containers(prepared, writer, params.ploidy, str(tmp_path / f"containers_{writer}"), denominator=total,
                                      min_posterior=params.prob_precision, unaligned_read_count=9)
                table = HarnessTable(engine, prepared, params.ploidy)
                try:
                    if kind == JOINT:
                        table.tpm(total)
                    text = HarnessTableText(engine, table, kind=kind, ploidy=params.ploidy, min_posterior=params.prob_precision)
                    try:
                        got = text.view()
                        line = text.host_line(len(got["row_off"]) - 1)
                        assert got["num_rows"] >= 2 and line["equal"] and got["bytes"] == line["bytes"] and got["row_off"].tolist() == line["row_off"].tolist()
                        text.write(str(tmp_path / f"text_{writer}"), unaligned_read_count=9)
                    finally:
                        text.free()
                finally:
                    table.free()
                want = open(tmp_path / f"containers_{writer}{suffix}", "rb").read()
                assert want.startswith(S.header(kind, params.ploidy) + got["bytes"]) and open(tmp_path / f"text_{writer}{suffix}", "rb").read() == want
                assert (want.count(b"\n") == got["num_rows"] + 2 and b"\nUnknown\tUnknown\t0\t0\t" in want) if kind == JOINT else want.count(b"\n") == got["num_rows"] + 1
        finally:
            prepared.free()
    finally:
        engine.close()
