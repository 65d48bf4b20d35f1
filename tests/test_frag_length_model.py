"""The restatement of the fragment-length model (tests/frag_length_cases.py) against the reference's OWN vectors —
src/tests/fragment_length_dist_test.cpp:8-155 and src/tests/paths_index_test.cpp:69-77, carried as data in
tests/golden/frag_length_fixture.json.  The GPU tests compare the device with this restatement, so it is pinned here
first, without a GPU."""
import numpy as np
import pytest

from tests import frag_length_cases as cases


def test_fixture_holds_the_reference_vectors_and_the_seeded_samples():
    vectors = cases.count_vectors()
    assert [len(v) for v in vectors.values()] == [92, 1000, 1001, 801, 801, 601, 3001]
    assert all(v[0] == 0 for v in vectors.values())
    assert [int(v.sum()) for v in vectors.values()][2:] == [100000, 100000, 50000, 60, 200000]
    assert len(cases.PATH_LENGTHS) == 2053 and len(cases.PATH_LENGTHS) % 64 != 0


def test_fit_finds_the_pinned_maximum_likelihood_estimate():  # fragment_length_dist_test.cpp:134-147
    fit = cases.restated_fit("reference_mle_92")
    mle = cases.fixture()["mle"]
    assert fit["valid"] and fit["max_length"] == 92
    assert abs(fit["loc"] - mle[0]) < 1e-3
    assert abs(fit["scale"] - mle[1]) < 1e-3
    assert abs(fit["shape"] - mle[2]) < 1e-3
    assert fit["evaluations"] == 522  # likelihood sums one after the other: what one launch per sum would cost


def test_fit_terminates_on_counts_derived_from_real_data():  # fragment_length_dist_test.cpp:149-154
    fit = cases.restated_fit("reference_real_data_1000")
    assert fit["valid"] and 1 <= fit["iterations"] <= 100
    assert np.isfinite([fit["loc"], fit["scale"], fit["shape"]]).all()


def test_normal_fit_is_sample_mean_and_standard_deviation():
    counts = cases.count_vectors()["reference_mle_92"]
    sample = np.repeat(np.arange(len(counts)), counts)
    fit = cases.fit(counts, skew_normal=False)
    assert fit["shape"] == 0.0 and fit["valid"]
    assert abs(fit["loc"] - sample.mean()) <= 1e-12 * sample.mean()
    assert abs(fit["scale"] - sample.std(ddof=1)) <= 1e-12 * sample.std(ddof=1)


def test_fewer_than_two_samples_leave_an_invalid_distribution():  # src/fragment_length_dist.cpp:74-80
    counts = np.zeros(50, dtype=np.uint32)
    assert not cases.fit(counts)["valid"]
    counts[17] = 1
    fit = cases.fit(counts)
    assert not fit["valid"] and fit["loc"] == 17 and fit["scale"] == 0 and fit["shape"] == 0


def test_skew_normal_cdf_table():  # fragment_length_dist_test.cpp:87-108
    for x, m, s, a, want in cases.fixture()["skew_normal_cdf"]:
        assert abs(float(cases.skew_normal_cdf(x, m, s, a)) - want) < 1e-6


def test_truncated_mean_table():  # fragment_length_dist_test.cpp:110-132
    for m, s, a, c, d, want in cases.fixture()["truncated_mean"]:
        assert abs(float(cases.truncated_mean(m, s, a, c, d)[0]) - want) < 1e-6


def test_log_prob_constants_and_log_phi():  # fragment_length_dist_test.cpp:15-18,31-38
    lp = cases.fixture()["log_prob"]
    for value, want in lp["values"]:
        assert cases.double_compare(float(cases.log_prob(value, lp["loc"], lp["scale"], 0.0)), want)
    assert cases.double_compare(float(cases.log_prob(9, 10, 2, 0.0)), float(cases.log_prob(11, 10, 2, 0.0)))
    z = np.arange(-10, 31, dtype=np.float64)
    assert np.all(np.abs(cases.log_phi(z) - np.log(cases.phi_cdf(z))) < 1e-5)
    assert np.all(np.isfinite(cases.log_phi(np.array([-25.0, -100.0, -1e4]))))  # the series below -20


def test_effective_lengths_of_the_reference():  # paths_index_test.cpp:69-77
    for case in cases.fixture()["effective_length"]:
        got, _ = cases.effective_lengths(case["lengths"], float(case["loc"]), float(case["scale"]), 0.0)
        for g, want in zip(got, case["values"]):
            assert cases.double_compare(g, want), (g, want)


@pytest.mark.parametrize("name", list(cases.count_vectors()))
def test_enough_path_lengths_have_a_usable_denominator(name):
    """The GPU test compares effective lengths where the denominator of the truncated mean is >= 1e-6 and asks for at
    least cases.min_comparable_lengths(name) such lengths of the 2 053; elsewhere the reference's own value is rounding
    noise of its Owen's T."""
    fit = cases.restated_fit(name)
    values, denom = cases.effective_lengths(cases.PATH_LENGTHS, fit["loc"], fit["scale"], fit["shape"])
    assert int((denom >= 1e-6).sum()) >= cases.min_comparable_lengths(name)
    assert values[0] == 0.0 and np.all(np.isfinite(values)) and np.all(values[1:] >= 1.0)
