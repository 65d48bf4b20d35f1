"""The texts of the rows parse's tests, CPU and GPU (tests/test_rows_parse_model.py, tests/test_hip_rows_parse.py): name -> bytes,
each the smallest at which a mechanism of rpvg_amd/csrc/rows_parse.hip can go wrong.  Printed by tests/rows_text_model.py, or
written by hand where the writer would not print them (clusters without paths or rows, unsorted groups, refusals)."""
import numpy as np

from tests import rows_parse_model as P
from tests import rows_text_model as R
from tests import table_text_model as M

U32_MAX, U64_MAX = 4294967295, 18446744073709551615

# the hard tokens of tests/cpp/number_parse_check.cpp, as cells; SLOW are decided by the exact comparison: exact ties all four
# (10^23 is the middle of two doubles that lie 2^24 apart)
SLOW = [b"9007199254740993", b"9007199254740995", b"4611686018427388416", b"1e23"]
HARD = SLOW + [b"1.7976931348623158e308", b"2.4703282292062327e-324", b"2.4703282292062328e-324", b"4.9406564584124654e-324", b"2.2250738585072011e-308",
               b"2.2250738585072014e-308", b"-0", b"0.000", b"00012.5", b"5E-1", b"inf", b"-inf", b"1.", b".5"]
# as a noise cell: inside (0, 1], and what rounds to 1 from above
HARD_NOISE = [b"2.4703282292062328e-324", b"4.9406564584124654e-324", b"2.2250738585072011e-308", b"5E-1", b"00000.5", b"1.",
              b"0.9999999999999999999", b"1.000000000000000000", b"9.999999999999999445e-1", b"9.999999999999999444e-1"]


def text_of(clusters, prob_precision=1e-8, ranked=False, name_lengths=(3,), seed=0, names=None):
    """clusters: dicts of num_paths and rows as tests/rows_text_model.py takes them; random lengths and effective lengths."""
    rng = np.random.default_rng(seed)
    n = sum(c["num_paths"] for c in clusters)
    if names is None:
        names = M.names_of_lengths([name_lengths[i % len(name_lengths)] for i in range(n)], seed=seed)
    lengths, eff = [int(x) for x in rng.integers(0, 100000, size=n)], [float(x) for x in rng.gamma(2.0, 400.0, size=n)]
    K = len(clusters)
    lists, index = ([int(x) for x in rng.integers(0, 1000, size=K)], list(range(K))) if ranked else (None, None)
    return R.rows_text(R.flatten(clusters), names, lengths, eff, prob_precision, lists, index)[0]


def random_clusters(seed, num_clusters, max_paths=6, max_rows=5, max_groups=4):
    """Clusters as the writer prints them: every row's groups sorted."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(num_clusters):
        n = int(rng.integers(1, max_paths + 1))
        rows = []
        for _ in range(int(rng.integers(1, max_rows + 1))):
            groups = sorted((float(rng.random()), [int(x) for x in rng.integers(0, n, size=int(rng.integers(1, 4)))]) for _ in range(int(rng.integers(0, max_groups + 1))))
            rows.append((int(rng.integers(1, 50)), float(rng.random()) or 0.5, groups))
        out.append(dict(num_paths=n, rows=rows))
    return out


def shapes(prob_precision):
    """The shapes of tests/test_hip_rows_text.py, bare and ranked markers mixed in one text."""
    rng = np.random.default_rng(1)
    members = lambda n: [int(x) for x in rng.integers(0, 70, size=n)]
    rows = [(0, 0.5, []), (9, 0.25, [(0.5, [])]), (10, 1e-9, [(0.125, [69])]), (U32_MAX, 1.0, [(0.1, members(63)), (0.2, members(64))]),
            (1, 0.3, [(0.3, members(65)), (0.4, [])]), (7, 0.9, [(0.5, []), (0.6, [0, 1])])]
    first = [dict(num_paths=70, rows=rows), dict(num_paths=1, rows=[(3, 0.75, [(0.25, [0])])])]
    second = [dict(num_paths=n, rows=[(n, 0.5, [(0.5, [n - 1])])]) for n in (1, 2, 64, 65, 300)]
    third = random_clusters(3, 20)
    return (text_of(first, prob_precision, ranked=False) + text_of(second, prob_precision, ranked=True, name_lengths=[0, 1, 3, 4, 5, 26, 27, 255], seed=4)
            + text_of(third, prob_precision, ranked=False, seed=5) + b"# 0 " + str(U64_MAX)[:19].encode() + b"\nx,1,2\n1 1\n")


def residue(n):
    """A small text whose first name has n bytes: every later token starts n bytes further."""
    clusters = [dict(num_paths=2, rows=[(3, 0.25, [(0.125, [0]), (0.5, [0, 1])]), (1, 0.5, [])]), dict(num_paths=1, rows=[(2, 1.0, [(1.0, [0])])])]
    return text_of(clusters, ranked=True, names=[b"n" * n, b"second", b"third"])


def long_cells():
    """64 rows of the longest cells back to back: 64 groups of a 24-byte probability at 17 digits each, ten-digit read counts."""
    smallest = 2.2250738585072014e-308
    probs = sorted(smallest * (1 + j * 2.0 ** -40) for j in range(64))
    lines = [b"#", b" ".join(b"p%d,%d,%s" % (j, U32_MAX, b"-1.2345678901234567e-300") for j in range(3))]
    cells = b" ".join(M.fmt(p, 17).encode() + b":2" for p in probs)
    lines += [str(U32_MAX).encode() + b" " + M.fmt(smallest, 17).encode() + b" " + cells] * 64
    return b"\n".join(lines) + b"\n"


STRUCTURE = {
    "empty text": b"",
    "only empty lines": b"\n\n\n",
    "one cluster": b"#\na,1,2.5\n3 0.5 0.5:0\n",
    "one bare marker": b"#",
    "no trailing newline": b"#\na,1,2.5\n3 0.5 0.5:0",
    "no paths: marker then marker": b"#\n#\na,1,2.5\n3 0.5 0.5:0\n# 4 5\n# 6 7\n",
    "paths and no rows": b"# 1 2\na,1,2.5 b,2,3.5\n#\nc,3,4\n1 1\n# 3 4\nd,9,9\n",
    "empty lines": b"\n\n#\n\na,1,2.5\n\n\n3 0.5 0.5:0\n\n#\n\n\nb,0,5\n\n1 0.25\n\n",
    "names with commas and colons": b"#\na,b,c,1,2.5 :,#,,7,1e3 ,0,0\n3 0.5 0.5:0,1,2 0.5:2\n",
    "a row that is only two fields": b"#\na,1,2\n4294967295 1\n0 1e-300\n",
    "groups without indices": b"#\na,1,2\n1 0.5 0.25: 0.5:0 0.75:\n",
}

# each differs from its own re-print: the groups leave sorted
GROUP_ORDER = {
    "descending probabilities": b"#\na,1,2 b,1,2 c,1,2\n1 0.5 0.75:0 0.5:1 0.25:2\n2 0.5 0.125:0\n",
    "equal probabilities, descending lists": b"#\na,1,2 b,1,2 c,1,2\n1 0.5 0.25:2,1 0.25:2 0.25:1,2 0.25:1 0.25:0,2,2 0.25:0\n",
    "equal at 8 digits only": b"#\na,1,2 b,1,2\n1 0.5 0.250000001:1 0.25:1 0.2500000001:0\n",
    "one descent at the end of 70 groups": b"#\na,1,2 b,1,2\n1 0.5 " + b" ".join(b"%s:0" % M.fmt(0.001 * (j + 1), 8).encode() for j in range(69)) + b" 0.0005:1\n",
    "129 groups reversed": b"#\na,1,2 b,1,2\n1 0.5 " + b" ".join(b"%s:%d" % (M.fmt(0.001 * (129 - j), 8).encode(), j % 2) for j in range(129)) + b"\n7 1\n",
    "a prefix list sorts first": b"#\na,1,2 b,1,2\n1 0.5 0.5:0,1,1 0.5:0,1 0.5:0\n",
}

# text -> (line, reason): one refusal each, then pairs of offending lines (the smaller wins) and pairs of reasons on a line
REFUSALS = {
    b"a,1,2\n#\n": (1, P.ORPHAN),
    b"\n\n1 0.5\n#\n": (3, P.ORPHAN),
    b"# 1\n": (1, P.MARKER),
    b"# 1 2 3\n": (1, P.MARKER),
    b"# 1 x\n": (1, P.MARKER),
    b"# 12345678901234567890 1\n": (1, P.MARKER),
    b"#\na,1\n": (2, P.PATH_FIELD),
    b"#\na,1,2 b\n": (2, P.PATH_FIELD),
    b"#\na,1,2\n5\n": (3, P.SHORT_ROW),
    b"#\na,1,2\n5 0.5 0.5\n": (3, P.NO_COLON),
    b"#\na,1,2\n5 0.5 0.5:1\n": (3, P.INDEX),
    b"#\n#\n5 0.5 0.5:0\n": (3, P.PATH_FIELD),
    b"#\na,1,2\n#\n\nb,1,2 c,1,2\n1 0.5 0.5:1\n1 0.5 0.5:2\n": (7, P.INDEX),
    b"#\na,1,2\n4294967296 0.5\n": (3, P.TOO_BIG),
    b"#\na,4294967296,2\n": (2, P.TOO_BIG),
    b"#\na,1,2\n5 0.5 0.5:4294967296\n": (3, P.TOO_BIG),
    b"#\na,1,2\n5 0\n": (3, P.NOISE),
    b"#\na,1,2\n5 -0.5\n": (3, P.NOISE),
    b"#\na,1,2\n5 1.0000000000000002\n": (3, P.NOISE),
    b"#\na,1,2\n5 nan\n": (3, P.NOISE),
    b"#\na,1,2\n5 inf\n": (3, P.NOISE),
    b"#\na,1,1e309\n": (2, P.OVERFLOW),
    b"#\na,1,2\n5 0.5 1.7976931348623159e308:0\n": (3, P.OVERFLOW),
    b"#\na,1,2\n5 0.12345678901234567890\n": (3, P.TOO_LONG),
    b"#\na,1,2\n5 0.5 0.5:00000000000000000000\n": (3, P.TOO_LONG),
    b"#\na,1,1.5abc\n": (2, P.MALFORMED),
    b"#\na,1,0x1p3\n": (2, P.MALFORMED),
    b"#\na,1,2\n5 +1\n": (3, P.MALFORMED),
    b"#\na,1,2\n+5 1\n": (3, P.MALFORMED),
    b"#\na,,2\n": (2, P.MALFORMED),
    b"#\na,1,\n": (2, P.MALFORMED),
    b"#\na,1,2\n5 0.5 :0\n": (3, P.MALFORMED),
    b"#\na,1,2\n5 0.5 0.5:0,\n": (3, P.MALFORMED),
    b"#\na,1,2\n5 0.5 0.5:,0\n": (3, P.MALFORMED),
    b"#\na,1,2\n5 0.5 0.5:0,,0\n": (3, P.MALFORMED),
    b"#\na,1,2\n5 0.5 0.5:0:0\n": (3, P.MALFORMED),
    b"#\na,1,2\n5 0.5\r\n": (3, P.MALFORMED),
    b"#\na,1,2\n5\t0.5\n": (3, P.SHORT_ROW),
    b"#\na,1,2\n5 0.5 \n": (3, P.EMPTY_FIELD),
    b"#\na,1,2\n5  0.5\n": (3, P.EMPTY_FIELD),
    b"#\n a,1,2\n": (2, P.EMPTY_FIELD),
    b"# \n": (1, P.EMPTY_FIELD),
    b"#\na,1,2\n5 \n": (3, P.EMPTY_FIELD),
    # two offending lines: the smaller wins, whatever its reason
    b"#\na,1,2\n5 0.5 \n5\n": (3, P.EMPTY_FIELD),
    b"#\na,1,2\n5 0.5 0.5:0\n\n5 2\n# 1\n": (5, P.NOISE),
    b"# x y\n#\na\n5\n": (1, P.MARKER),
    # two reasons on one line: the smaller reason
    b"#\na,1,2\n5 2 0.5 0.5:x\n": (3, P.NO_COLON),
    b"#\na,1,2\n 5 0.5:7\n": (3, P.NO_COLON),
    b"#\na,1,2\n5 0.5 0.5:7 \n": (3, P.INDEX),
}


def long_row(groups, descending):
    """One row of that many groups of one index, ascending by probability or descending, and a row behind it."""
    probs = [M.fmt((groups - j if descending else j + 1) / (2.0 * groups), 8).encode() for j in range(groups)]
    return b"#\na,1,2 b,1,2\n\n1 0.5 " + b" ".join(b"%s:%d" % (p, j % 2) for j, p in enumerate(probs)) + b"\n2 1\n"


def big_text():
    """About 70 000 lines and 1 MB: every scan runs more than one tile."""
    return text_of(random_clusters(11, 17000, max_rows=5), ranked=True, name_lengths=(4, 9, 17), seed=12)


def hard_token_text():
    """The hard tokens as effective lengths and as probabilities, the noise ones as noise cells."""
    lines = [b"#", b" ".join(b"p%d,%d,%s" % (j, j, t) for j, t in enumerate(HARD + [b"nan", b"-nan"]))]
    lines += [b"1 %s" % t for t in HARD_NOISE]
    lines += [b"2 0.5 %s:%d" % (t, j) for j, t in enumerate(HARD)]
    return b"\n".join(lines) + b"\n"


# the bound of the one-thread sort (kMaxUnsortedGroups = 1024): a row of 1024 groups is sorted whatever its order, a longer one
# must arrive in order, and one that does not is refused by name, behind every other offence of the text
GROUP_ORDER["1024 groups reversed"] = long_row(1024, True)
STRUCTURE["1025 groups in order"] = long_row(1025, False)
REFUSALS[long_row(1025, True)] = (4, P.UNSORTED_ROW)
REFUSALS[long_row(1025, True) + b"5 2\n"] = (6, P.NOISE)
