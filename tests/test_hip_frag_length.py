"""The fragment-length model on the GPU (rpvg_amd/csrc/frag_length.hip) against the restatement of
tests/frag_length_cases.py, which tests/test_frag_length_model.py pins to the reference's own vectors.

The fit is compared with 1e-3 absolute, the reference's own tolerance for this algorithm
(src/tests/fragment_length_dist_test.cpp:144-146): on near-symmetric samples the alternating search moves by some 1e-4
when the likelihood sums are added in another order.  Everything downstream — the density table, the effective lengths —
is compared at the DEVICE's own parameters.  Effective lengths are compared where the denominator of the truncated mean,
cdf(v) - cdf(u), is at least 1e-6; below that the reference's value is the rounding noise of its Owen's T."""
import copy
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle
from rpvg_amd import engine as eng_mod
from rpvg_amd import hip
from rpvg_amd.batch import ClusterBatch, make_params
from rpvg_amd.rows import INT32_LOWEST, AlignmentBatch, RowParams
from tests import frag_length_cases as cases

pytestmark = pytest.mark.gpu

VECTORS = list(cases.count_vectors())
_device_fits = {}


def device_fit(hip_ctx, name, skew_normal=True):
    """The device's fit of a fixture vector, computed once per session."""
    key = (name, skew_normal)
    if key not in _device_fits:
        _device_fits[key] = hip_ctx.frag_length_fit(cases.count_vectors()[name], skew_normal)
    return _device_fits[key]


def fit_bits(fit):
    return (np.float64(fit.loc).tobytes(), np.float64(fit.scale).tobytes(), np.float64(fit.shape).tobytes(), fit.max_length,
            fit.sample_size, fit.iterations, fit.evaluations, fit.valid)


# ---- fit ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", VECTORS)
def test_fit_equals_the_restatement(hip_ctx, name):
    counts = cases.count_vectors()[name]
    got, want = device_fit(hip_ctx, name), cases.restated_fit(name)
    print(name, "device", got.loc, got.scale, got.shape, got.iterations, got.evaluations,
          "restated", want["loc"], want["scale"], want["shape"], want["iterations"], want["evaluations"])
    assert got.valid == 1 and got.max_length == len(counts) and got.sample_size == int(counts.sum())
    assert abs(got.loc - want["loc"]) < 1e-3
    assert abs(got.scale - want["scale"]) < 1e-3
    assert abs(got.shape - want["shape"]) < 1e-3
    assert 1 <= got.iterations <= 100 and got.evaluations > 0
    again = hip_ctx.frag_length_fit(counts, True)
    assert fit_bits(again) == fit_bits(got)  # one fixed order of every sum: the same bits


def test_fit_finds_the_pinned_maximum_likelihood_estimate(hip_ctx):  # fragment_length_dist_test.cpp:134-147
    got, mle = device_fit(hip_ctx, "reference_mle_92"), cases.fixture()["mle"]
    assert abs(got.loc - mle[0]) < 1e-3 and abs(got.scale - mle[1]) < 1e-3 and abs(got.shape - mle[2]) < 1e-3


@pytest.mark.parametrize("name", VECTORS)
def test_normal_fit_is_sample_mean_and_standard_deviation(hip_ctx, name):
    counts = cases.count_vectors()[name].astype(np.int64)
    idx = np.arange(len(counts), dtype=np.int64)
    n = int(counts.sum())
    mean = float((idx * counts).sum()) / n
    sd = np.sqrt(float(np.sum((idx - mean) ** 2 * counts)) / (n - 1))
    got = device_fit(hip_ctx, name, skew_normal=False)
    assert got.valid == 1 and got.shape == 0.0 and got.max_length == len(counts) and got.iterations == 0
    assert abs(got.loc - mean) <= 1e-12 * mean
    assert abs(got.scale - sd) <= 1e-12 * sd


def test_degenerate_and_invalid_counts(hip_ctx):
    counts = np.zeros(300, dtype=np.uint32)
    fit = hip_ctx.frag_length_fit(counts)
    assert fit.valid == 0 and fit.sample_size == 0
    counts[217] = 1
    for skew_normal in (True, False):
        fit = hip_ctx.frag_length_fit(counts, skew_normal)
        assert fit.valid == 0 and fit.loc == 217.0 and fit.scale == 0.0 and fit.shape == 0.0 and fit.max_length == 300
    counts[0] = 3
    with pytest.raises(hip.EngineError, match="length 0"):
        hip_ctx.frag_length_fit(counts)
    for bad in (np.zeros(65537, dtype=np.uint32), np.zeros(0, dtype=np.uint32)):
        rc = hip.lib().rpvg_hip_frag_length_fit(hip_ctx.handle, C.c_void_p(bad.ctypes.data if bad.size else None), C.c_uint32(bad.size),
                                                C.c_int(1), C.byref(hip.CFragLengthFit()))
        assert rc == RPVG_HIP_ERR_INVALID
    longest = np.zeros(65536, dtype=np.uint32)  # 64 entries per thread, the widest kernel
    longest[1:] = 1 + (np.arange(65535) % 7)
    got = hip_ctx.frag_length_fit(longest, False)
    idx = np.arange(65536, dtype=np.float64)
    mean = float((idx * longest).sum()) / float(longest.sum())
    assert got.valid == 1 and got.max_length == 65536 and abs(got.loc - mean) <= 1e-12 * mean


RPVG_HIP_ERR_INVALID = -3  # include/rpvg_hip.h


# ---- density table --------------------------------------------------------------------------------------------

def table_cases(hip_ctx):
    out = [(name, device_fit(hip_ctx, name).loc, device_fit(hip_ctx, name).scale, device_fit(hip_ctx, name).shape) for name in VECTORS]
    out.append(("normal_10_2", 10.0, 2.0, 0.0))  # fragment_length_dist_test.cpp:10
    out += [("consistency_mu%d_sigma%d" % (mu, sigma), float(mu), float(sigma), -3.0) for mu in range(4) for sigma in (1, 2, 3)]  # :59-85
    return out


def test_density_table_equals_the_oracle_at_the_same_parameters(hip_ctx):
    for name, loc, scale, shape in table_cases(hip_ctx):
        table = hip_ctx.frag_length_table(loc, scale, shape)
        try:
            got = table.download()
        finally:
            table.free()
        want = pyoracle.frag_length_table(loc, scale, shape)
        assert got.shape == (65536,) and np.all(np.isfinite(got)), name
        err = np.abs(got - want) / np.abs(want)
        print(name, "max relative error", err.max())
        assert err.max() <= 1e-9, (name, int(np.argmax(err)))


def test_log_prob_constants_of_the_reference(hip_ctx):  # fragment_length_dist_test.cpp:15-18
    lp = cases.fixture()["log_prob"]
    table = hip_ctx.frag_length_table(float(lp["loc"]), float(lp["scale"]), 0.0)
    try:
        got = table.download()
    finally:
        table.free()
    for value, want in lp["values"]:
        assert cases.double_compare(got[value], want), (value, got[value], want)
    assert cases.double_compare(got[9], got[11])


# ---- skew-normal CDF, truncated mean ----------------------------------------------------------------------------

def test_skew_normal_cdf_and_truncated_mean_tables_of_the_reference(hip_ctx):  # fragment_length_dist_test.cpp:87-132
    rows = np.array(cases.fixture()["skew_normal_cdf"])
    got = hip_ctx.frag_length_eval("cdf", rows[:, :4])
    assert np.all(np.abs(got - rows[:, 4]) < 1e-6), np.abs(got - rows[:, 4])
    rows = np.array(cases.fixture()["truncated_mean"])
    got = hip_ctx.frag_length_eval("truncated_mean", rows[:, :5])
    assert np.all(np.abs(got - rows[:, 5]) < 1e-6), np.abs(got - rows[:, 5])


# ---- effective lengths --------------------------------------------------------------------------------------

def check_effective_lengths(hip_ctx, name, loc, scale, shape, floor):
    got = hip_ctx.effective_lengths(cases.PATH_LENGTHS, loc, scale, shape)
    want, denom = cases.effective_lengths(cases.PATH_LENGTHS, loc, scale, shape)
    assert got.shape == (2053,) and got[0] == 0.0
    assert np.all(np.isfinite(got)) and np.all(got[1:] >= 1.0)
    comparable = denom >= 1e-6
    comparable[0] = False
    assert int(comparable.sum()) >= floor, (name, int(comparable.sum()))
    err = np.abs(got[comparable] - want[comparable]) / want[comparable]
    print(name, "comparable", int(comparable.sum()), "max relative error", err.max())
    assert err.max() <= 1e-6, (name, err.max())


@pytest.mark.parametrize("name", VECTORS)
def test_effective_lengths_at_the_device_fit(hip_ctx, name):
    fit = device_fit(hip_ctx, name)
    check_effective_lengths(hip_ctx, name, fit.loc, fit.scale, fit.shape, cases.min_comparable_lengths(name))


def test_effective_lengths_of_normal_distributions_and_the_reference_values(hip_ctx):  # paths_index_test.cpp:69-77
    for loc, scale, shape in cases.NORMAL_DISTRIBUTIONS:
        check_effective_lengths(hip_ctx, "normal_%g_%g" % (loc, scale), loc, scale, shape, 1000)
    for case in cases.fixture()["effective_length"]:
        got = hip_ctx.effective_lengths(case["lengths"], float(case["loc"]), float(case["scale"]), 0.0)
        for g, want in zip(got, case["values"]):
            assert cases.double_compare(g, want), (g, want)


# ---- through the pipeline -------------------------------------------------------------------------------------

def pipeline_clusters():
    """Three small clusters from the case data of tests/test_row_construction.py: its base case, its multi-alignment case
    and its random cluster (12 paths, 300 reads)."""
    base = dict(paths=[dict(effective_length=3.0), dict(effective_length=3.0)],
                reads=[dict(count=1, min_mapq=10, noise_score=INT32_LOWEST, aligns=[(3, 5, 10, [0, 1])])])
    multi = copy.deepcopy(base)
    multi["paths"] += [dict(effective_length=3.0), dict(effective_length=3.0)]
    multi["reads"][0]["aligns"].append((5, 8, 15, [3]))
    rng = np.random.default_rng(11)
    paths = [dict(effective_length=float(rng.integers(50, 3000))) for _ in range(12)]
    reads = []
    for _ in range(300):
        aligns = []
        for _ in range(int(rng.integers(1, 4))):
            idx = sorted(set(int(x) for x in rng.integers(0, 12, size=int(rng.integers(1, 5)))))
            aligns.append((int(rng.integers(-10, 60)), int(rng.integers(50, 150)), int(rng.integers(1, 40)), idx))
        reads.append(dict(count=int(rng.integers(1, 4)), min_mapq=int(rng.choice([0, 3, 10, 30, 60])),
                          noise_score=int(rng.choice([INT32_LOWEST, -3000000, -500000])), aligns=aligns))
    return [base, multi, dict(paths=paths, reads=reads)]


def path_batch(clusters, effective_lengths):
    it = iter(effective_lengths)
    return ClusterBatch.from_clusters([dict(paths=[dict(group_id=i, source_count=1, source_ids=[i], effective_length=float(next(it)))
                                                   for i, _ in enumerate(cl["paths"])], rows=[]) for cl in clusters])


def test_fit_table_and_effective_lengths_through_the_pipeline(hip_ctx):
    """prepare_from_alignments(frag_counts, path_lengths) — fit, table and effective lengths on the device in one call — against
    the same steps composed by hand: rows and estimates are the same bits, and the paths carry the device's effective lengths."""
    clusters = pipeline_clusters()
    # fragment lengths of the reads (1 .. 39) with a skewed count vector around them, so that their densities matter
    counts = np.zeros(64, dtype=np.uint32)
    counts[1:] = np.round(4000 * np.exp(-0.5 * ((np.arange(1, 64) - 14.0) / np.where(np.arange(1, 64) < 14, 4.0, 9.0)) ** 2)).astype(np.uint32)
    path_lengths = np.array([40, 55, 38, 7, 90, 61] + [int(p["effective_length"]) + 20 for p in clusters[2]["paths"]], dtype=np.uint32)

    e = eng_mod.Engine(0)
    try:
        fit = e.fit_frag_length(counts)
        assert fit.valid and fit.max_length == 64 and abs(fit.shape) > 0.5
        eff = e.effective_lengths(path_lengths, fit)
        assert np.all(eff >= 1.0)

        fused = e.prepare_from_alignments(AlignmentBatch.from_clusters(clusters), path_batch(clusters, np.zeros(len(path_lengths))),
                                          frag_counts=counts, path_lengths=path_lengths, min_noise_prob=1e-4)
        assert fused.frag_fit[:5] == fit[:5] and fused.frag_fit.stats == fit.stats
        assert np.array_equal(fused.path_effective_length, eff)

        by_hand_clusters = copy.deepcopy(clusters)
        it = iter(eff)
        for cl in by_hand_clusters:
            for p in cl["paths"]:
                p["effective_length"] = float(next(it))
        by_hand_aligns = AlignmentBatch.from_clusters(by_hand_clusters)
        by_hand = e.prepare_from_alignments(by_hand_aligns, path_batch(clusters, eff), frag=fit, min_noise_prob=1e-4)

        params = make_params()
        got, _ = e.run("transcripts", params, fused)
        want, _ = e.run("transcripts", params, by_hand)
        assert len(got) == len(want) == 3
        for g, w in zip(got, want):
            assert g.total_count == w.total_count and g.em_iters == w.em_iters
            gk, wk = g.keyed(), w.keyed()
            assert set(gk) == set(wk)
            for key in wk:
                assert gk[key][0] == wk[key][0]
                assert np.array_equal(np.asarray(gk[key][1]), np.asarray(wk[key][1]))

        with pytest.raises(ValueError):
            e.prepare_from_alignments(by_hand_aligns, path_batch(clusters, eff), frag=fit, frag_counts=counts, path_lengths=path_lengths)
    finally:
        e.close()

    # the rows themselves: built from the resident table + effective lengths set in place, against the table's host copy
    table = hip_ctx.frag_length_table(fit.loc, fit.scale, fit.shape)
    dev = hip_ctx.upload_alignments(AlignmentBatch.from_clusters(clusters))
    try:
        assert np.array_equal(dev.set_effective_lengths(path_lengths, fit.loc, fit.scale, fit.shape), eff)
        resident, _, _ = hip_ctx.build_rows(dev, RowParams(min_noise_prob=1e-4, frag_length_table=table))
        uploaded, _, _ = hip_ctx.build_rows(by_hand_aligns, RowParams(min_noise_prob=1e-4, frag_length_log_prob=table.download()))
    finally:
        dev.free()
        table.free()
    assert resident.num_rows == uploaded.num_rows > 0
    for name in ("cluster_row_off", "row_count", "row_noise", "row_grp_off", "grp_prob", "grp_idx_off", "path_idx"):
        assert np.array_equal(getattr(resident, name), getattr(uploaded, name)), name
    want_rows, _ = pyoracle.build_rows(by_hand_aligns, RowParams(min_noise_prob=1e-4, frag_length_log_prob=pyoracle.frag_length_table(fit.loc, fit.scale, fit.shape)))
    assert want_rows.num_rows == resident.num_rows
    assert np.allclose(resident.grp_prob, want_rows.grp_prob, rtol=1e-9, atol=0) and np.array_equal(resident.path_idx, want_rows.path_idx)


def test_row_params_without_any_table_are_refused(hip_ctx):
    dev = hip_ctx.upload_alignments(AlignmentBatch.from_clusters(pipeline_clusters()[:1]))
    try:
        h = C.c_void_p()
        from rpvg_amd.rows import CRowParams
        prm = CRowParams(1e-8, 1e-4, 0, None, None)
        rc = hip.lib().rpvg_hip_read_rows_build(hip_ctx.handle, dev.handle, C.byref(prm), C.c_int32(1), C.byref(h))
        assert rc == RPVG_HIP_ERR_INVALID and b"frag_length_log_prob" in hip.lib().rpvg_hip_last_error()
    finally:
        dev.free()


# ---- the C++ interface ----------------------------------------------------------------------------------------

def build_frag_length_dist_check() -> str:
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "frag_length_dist_check")
    host, csrc = os.path.join(root, "rpvg_amd", "host"), os.path.join(root, "rpvg_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fopenmp", "-I" + host, "-I" + csrc,
                           os.path.join(root, "tests", "cpp", "frag_length_dist_check.cpp"), "-o", binary, "-L" + host, "-lrpvg_amd_host",
                           "-L" + csrc, "-lrpvg_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + csrc])
    return binary


@pytest.mark.parametrize("name", ["reference_mle_92", "reference_real_data_1000"])
def test_host_classes_through_the_cpp_interface(tmp_path, name):
    """tests/cpp/frag_length_dist_check.cpp: FragmentLengthDist(counts, skew_normal) and effectivePathLengths of
    rpvg_amd/host/read_rows.hpp against the sequential host loop."""
    import subprocess
    counts_file = tmp_path / "counts.txt"
    counts_file.write_text("\n".join(str(int(c)) for c in cases.count_vectors()[name]) + "\n")
    out = subprocess.run([build_frag_length_dist_check(), str(counts_file)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "ok"
