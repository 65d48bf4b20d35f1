"""Generates tests/golden/frag_length_fixture.json: the vectors the reference holds for its fragment-length model and the
seeded count vectors the tests add to them.

From the reference's unit tests (data only; read from the checkout, which does not travel):
  src/tests/fragment_length_dist_test.cpp   the two fragment-length count vectors (:137 and :150), the ten rows of
                                            skew-normal CDF values (:90-101) and of truncated means (:114-125), the
                                            pinned maximum-likelihood estimate (:144-146), the logProb constants (:15-18)
  src/tests/paths_index_test.cpp:64-77      two path lengths, two normal distributions, four effective lengths
Drawn here: count vectors of samples of scipy.stats.skewnorm, in this order from numpy.random.default_rng(1); each sample
is rounded, clipped to [1, L - 1] and binned to length L.

    python tests/golden/make_frag_length_fixture.py [/root/reference]
"""
import json
import os
import re
import sys

import numpy as np
from scipy.stats import skewnorm

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT = "/root/reference"

# (a, loc, scale, n, L); the last one is longer than the fit kernel's workgroup: several entries per thread, ragged last stride
SEEDED = [(5, 250, 60, 100000, 1001), (-4, 400, 50, 100000, 801), (0, 300, 40, 50000, 801), (3, 200, 30, 60, 601),
          (4, 1500, 300, 200000, 3001)]


def number_lists(text, opener):
    """The brace-enclosed rows of numbers behind every occurrence of `opener`."""
    out = []
    for m in re.finditer(re.escape(opener), text):
        depth, i = 0, m.end() - 1
        start = i
        while True:
            depth += text[i] == "{"
            depth -= text[i] == "}"
            i += 1
            if depth == 0:
                break
        out.append(text[start:i])
    return out


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else DEFAULT
    text = open(os.path.join(root, "src", "tests", "fragment_length_dist_test.cpp")).read()
    counts = [[int(x) for x in re.findall(r"\d+", block)] for block in number_lists(text, "length_counts{")]
    assert [len(c) for c in counts] == [92, 1000], [len(c) for c in counts]
    tables = []
    for block in number_lists(text, "tests {"):
        rows = re.findall(r"\{([^{}]+)\}", block)
        tables.append([[float(x) for x in row.split(",")] for row in rows])
    assert [len(t) for t in tables] == [10, 10] and len(tables[0][0]) == 5 and len(tables[1][0]) == 6

    rng = np.random.default_rng(1)
    seeded = []
    for (a, loc, scale, n, length) in SEEDED:
        x = skewnorm.rvs(a, loc=loc, scale=scale, size=n, random_state=rng)
        x = np.clip(np.rint(x), 1, length - 1).astype(np.int64)
        seeded.append(dict(a=a, loc=loc, scale=scale, n=n, counts=np.bincount(x, minlength=length).tolist()))
        assert len(seeded[-1]["counts"]) == length and seeded[-1]["counts"][0] == 0

    doc = dict(
        source="src/tests/fragment_length_dist_test.cpp and src/tests/paths_index_test.cpp of the reference checkout (their data only)",
        counts_mle=counts[0], counts_real_data=counts[1],
        mle=[50.996133408667475, 10.035973814767827, 4.7885824148015015],
        skew_normal_cdf=tables[0],       # x, m, s, a -> cdf
        truncated_mean=tables[1],        # m, s, a, c, d -> mean
        log_prob=dict(loc=10, scale=2, values=[[9, -1.737085713764618], [15, -4.737085713764618], [10000, -12475014.11208571307361]]),
        effective_length=[dict(loc=5, scale=2, lengths=[38, 7], values=[32.889504274642021, 2.4592743581826583]),
                          dict(loc=20, scale=1, lengths=[38, 7], values=[18, 1])],
        seeded=seeded)
    out = os.path.join(HERE, "frag_length_fixture.json")
    with open(out, "w") as f:
        json.dump(doc, f)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
