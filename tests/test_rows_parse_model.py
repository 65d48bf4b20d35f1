"""tests/rows_parse_model.py, the yardstick of tests/test_hip_rows_parse.py, pinned without a GPU: to hand-written texts, to
readProbabilityClusters (the harness's host line, byte for byte, on every case the host reader accepts), to tests/rows_text_model.py
as its inverse, and to the functions of rpvg_amd/csrc/rows_parse_plan.hpp run over serial scans on the host (what the kernels
compute, refusals included)."""
import numpy as np
import pytest

from rpvg_amd import hip
from rpvg_amd.table_text import host_line_parse, plan_parse
from tests import rows_parse_cases as cases
from tests import rows_parse_model as P
from tests import rows_text_model as R


def accepted():
    yield from ((f"shapes at {pp}", cases.shapes(pp)) for pp in (1e-8, 1e-12, 1e-17))
    yield from ((f"residue {n}", cases.residue(n)) for n in (1, 2, 3, 63, 64, 65, 127, 128, 129, 130))
    yield "a 4000-byte name", cases.text_of([dict(num_paths=2, rows=[(1, 0.5, [(0.5, [1])])])], names=[b"x" * 4000, b"y"])
    yield "1000 indices in one group", cases.text_of([dict(num_paths=100000, rows=[(1, 0.5, [(0.5, [int(x) for x in np.random.default_rng(3).integers(0, 100000, size=1000)])])])], name_lengths=(1,))
    yield "64 rows of the longest cells", cases.long_cells()
    yield "hard tokens", cases.hard_token_text()
    yield from cases.STRUCTURE.items()
    yield from cases.GROUP_ORDER.items()


ACCEPTED = dict(accepted())
# std::stod throws on a subnormal (glibc's strtod sets ERANGE for it): the host reader cannot read the text of the hard tokens,
# which the device parse must (docs/design/parity.md item 22).  Python's float() and the C++ check's strtod are its yardstick.
HOST_REFUSES = {"hard tokens"}


def test_hand_written_text():
    flat = P.parse(b"# 7 3\nab,10,2.5 c,,d,20,1e2\n\n2 0.25 0.5:1 0.125:0,1\n1 1\n#\n#\nz,1,1\n")
    want = dict(cluster_row_off=[0, 2, 2, 2], cluster_path_off=[0, 2, 2, 3], row_count=[2, 1], row_noise=[0.25, 1.0], row_grp_off=[0, 2, 2], grp_prob=[0.125, 0.5],
                grp_idx_off=[0, 2, 3], path_idx=[0, 1, 1], name_off=[0, 2, 6, 7], path_length=[10, 20, 1], path_effective_length=[2.5, 100.0, 1.0], has_rank_key=[1, 0, 0],
                num_align_lists=[7, 0, 0], cluster_index=[3, 0, 0])
    assert flat["name_bytes"] == b"abc,,dz"
    for name, values in want.items():
        assert flat[name].tolist() == values, name
    assert flat["path_idx"].dtype == np.uint32 and flat["grp_idx_off"].dtype == np.uint64 and flat["has_rank_key"].dtype == np.uint8


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_model_is_the_host_reader_and_the_plan(name):
    text = ACCEPTED[name]
    flat = P.parse(text)
    if name in HOST_REFUSES:
        with pytest.raises(hip.EngineError, match="stod"):
            host_line_parse(text)
    else:
        assert P.same(host_line_parse(text), flat) == []
    assert P.same(plan_parse(text), flat) == []


def test_group_order_cases_differ_from_their_reprint():
    for name, text in cases.GROUP_ORDER.items():
        assert P.print_back(P.parse(text)) != text, name
    flat = P.parse(cases.GROUP_ORDER["equal probabilities, descending lists"])
    assert [flat["path_idx"][int(a):int(b)].tolist() for a, b in zip(flat["grp_idx_off"][:-1], flat["grp_idx_off"][1:])] == [[0], [0, 2, 2], [1], [1, 2], [2], [2, 1]]


@pytest.mark.parametrize("prob_precision", [1e-8, 1e-12, 1e-17])
def test_inverse_of_the_rows_text_model(prob_precision):
    """print -> parse -> print is the identity, and at 17 digits so is parse -> arrays: every double round-trips."""
    clusters = cases.random_clusters(21, 200)
    rng = np.random.default_rng(22)
    n = sum(c["num_paths"] for c in clusters)
    names = [b"t%d" % i for i in range(n)]
    lengths, eff = [int(x) for x in rng.integers(0, 100000, size=n)], [float("%.6g" % x) for x in rng.gamma(2.0, 400.0, size=n)]
    flat = R.flatten(clusters)
    text = R.rows_text(flat, names, lengths, eff, prob_precision)[0]
    parsed = P.parse(text)
    assert P.print_back(parsed, prob_precision) == text
    assert P.names_of(parsed) == names and parsed["path_length"].tolist() == lengths
    if prob_precision == 1e-17:
        for name, array in flat.items():
            assert parsed[name].tobytes() == array.tobytes(), name
        assert parsed["path_effective_length"].tolist() == eff  # (six digits: the path line's 8 hold them)


@pytest.mark.parametrize("text", list(cases.REFUSALS))
def test_refusals(text):
    line, why = cases.REFUSALS[text]
    with pytest.raises(P.Refused) as refused:
        P.parse(text)
    assert (refused.value.line, refused.value.why) == (line, why)
    with pytest.raises(hip.EngineError, match=r"line %d: " % line) as by_plan:
        plan_parse(text)
    assert str(by_plan.value).endswith(f"line {line}: {P.REASONS[why]}")


def test_plan_counts_the_exact_tokens():
    """The ties and the near-tie of the hard tokens go the slow way as an effective length and as a probability; nothing else of the text does."""
    assert plan_parse(cases.hard_token_text())["exact_tokens"] == 2 * len(cases.SLOW)
    assert plan_parse(cases.shapes(1e-17))["exact_tokens"] == 0
