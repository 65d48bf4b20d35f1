"""Plain-Python model of the table text (include/rpvg_text.h): the rows the three writers print, every double by Python's
'%.*g' % v — correctly rounded, ties to even, which was checked against glibc on ties, carries, subnormals and the specials — with
`-nan` where the sign bit of a NaN is set (glibc's spelling; Python writes `nan` for both).  The cases of tests/test_hip_table_text.py."""
import struct
from decimal import Decimal, localcontext

import numpy as np

PER_PATH, HAPLOTYPE = 0, 1


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


NAN, NEG_NAN = from_bits(0x7ff8000000000000), from_bits(0xfff8000000000000)


def fmt(v, precision=8):
    v = float(v)
    if v != v:
        return "-nan" if bits(v) >> 63 else "nan"
    return "%.*g" % (precision, v)


def is_tie(v, precision):
    """Whether v lies exactly half way between two decimals of `precision` significant digits; and the parity of the lower one."""
    with localcontext() as exact:
        exact.prec = 1200                                # a double has at most 767 significant decimal digits
        d = abs(Decimal(v))
        exponent = d.adjusted() - (precision - 1)
        scaled = d.scaleb(-exponent)                     # `precision` digits in front of the point
        whole = int(scaled)
        return scaled - whole == Decimal("0.5"), whole % 2


def join(rows):
    """rows: one bytes per path (b"" for a row that is not printed) -> (text, row_off)."""
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return b"".join(rows), off


def _raw(name):
    return name.encode() if isinstance(name, str) else bytes(name)


def gibbs_text(table, cluster_path_off, names, cluster_ids, precision=8):
    """table: samples [P, N] and listed [P] (tests/gibbs_table_model.table or a view of the device table)."""
    rows = []
    for k in range(len(cluster_ids)):
        for g in range(int(cluster_path_off[k]), int(cluster_path_off[k + 1])):
            if not table["listed"][g]:
                rows.append(b"")
                continue
            cells = [str(int(cluster_ids[k]))] + [fmt(v, precision) for v in table["samples"][g]]
            rows.append(_raw(names[g]) + b"\t" + "\t".join(cells).encode() + b"\n")
    return join(rows)


def estimates_text(kind, flat, table, names, lengths, cluster_ids, precision=8):
    """flat: the arrays of rpvg_estimates_flat by name; table: haplotype_prob, read_count, tpm [P] and member_tpm [M].
    PER_PATH has the writer's precondition that set i of a cluster is {i}: ValueError names the first cluster that breaks it."""
    rows = []
    for k in range(len(cluster_ids) if kind == PER_PATH else 0):                 # every cluster is checked before a row is written
        p0, p1 = int(flat["cluster_path_off"][k]), int(flat["cluster_path_off"][k + 1])
        s0, s1 = int(flat["set_off"][k]), int(flat["set_off"][k + 1])
        ok = s1 - s0 == p1 - p0 and int(flat["abund_off"][k + 1]) - int(flat["abund_off"][k]) == p1 - p0
        for i in range(p1 - p0 if ok else 0):
            m0, m1 = int(flat["member_off"][s0 + i]), int(flat["member_off"][s0 + i + 1])
            ok = ok and m1 - m0 == 1 and int(flat["members"][m0]) == i
        if not ok:
            raise ValueError(f"cluster {k}")
    for k in range(len(cluster_ids)):
        p0, p1 = int(flat["cluster_path_off"][k]), int(flat["cluster_path_off"][k + 1])
        s0 = int(flat["set_off"][k])
        for g in range(p0, p1):
            cells = [str(int(cluster_ids[k])), str(int(lengths[g])), fmt(flat["path_effective_length"][g], precision)]
            if kind == PER_PATH:
                i = g - p0
                cells += [fmt(flat["abundances"][int(flat["abund_off"][k]) + i], precision), fmt(table["member_tpm"][int(flat["member_off"][s0]) + i], precision)]
            else:
                cells += [fmt(table["haplotype_prob"][g], precision), fmt(table["read_count"][g], precision), fmt(table["tpm"][g], precision)]
            rows.append(_raw(names[g]) + b"\t" + "\t".join(cells).encode() + b"\n")
    return join(rows)


# ---- cases --------------------------------------------------------------------------------------------------------------------

# ties of both parities at 8 digits, the carries that change the notation, -0.0, a subnormal, inf, both NaNs, the longest cells
TIES_8 = [10000000.5, 10000001.5, 123456785.0, 123456795.0, 99999999.5]             # even, odd, odd, odd, a carry into 1e+08
TIES_17 = [820243765413041.875, 2184215104430048.25, -1421918149280896.25]
CARRIES = [float(np.nextafter(0.0000999999995, 1.0)), 0.0000999999995, 1.99999995, 9.99999995e+99, 0.000999999995, 99999.9995, 999999995.0]
SPECIALS = [-0.0, 0.0, 5e-324, float("inf"), float("-inf"), NAN, NEG_NAN, 1e-5, from_bits(2024)]
LONGEST = [-1.2345678e-308, -1.2345678901234567e-308]
HARD_CELLS = TIES_8 + TIES_17 + CARRIES + SPECIALS + LONGEST

NAME_LENGTHS = [0, 1, 3, 4, 5, 255]


def names_of_lengths(lengths, seed=0):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(97, 123, size=n, dtype=np.uint8)) for n in lengths]


def gibbs_clusters(listed_rows, N):
    """listed_rows: per cluster a list of None (an unlisted path) or N values -> clusters of tests/gibbs_table_model with ONE
    block per cluster that lists the paths with values."""
    clusters = []
    for rows in listed_rows:
        ids = [i for i, r in enumerate(rows) if r is not None]
        abund = [[float(rows[i][s]) for i in ids] for s in range(N)] if ids else []
        blocks = [dict(ids=ids, noise=[0.5 * (s + 1) for s in range(N)], abund=abund)] if ids else []
        clusters.append(dict(num_paths=len(rows), total_count=7.25, blocks=blocks))
    return clusters


def sample_values(rng, n):
    """Values a sampler could have drawn, and rows of them that differ: counts with fractions, zeros, some large."""
    v = rng.gamma(0.7, 40.0, size=n)
    v[rng.random(n) < 0.2] = 0.0
    v[rng.random(n) < 0.05] *= 1e6
    return [float(x) for x in v]


def hand_gibbs():
    """Two clusters (ClusterIDs 7 and 9) of 2 and 1 paths, N = 3; path 1 is not listed."""
    table = dict(samples=np.array([[10.0, 0.5, 1e-5], [0.0, 0.0, 0.0], [123456785.0, -0.0, 1e21]]), listed=np.array([1, 0, 1], dtype=np.uint8))
    text = b"tx_a\t7\t10\t0.5\t1e-05\n" + b"c\t9\t1.2345678e+08\t-0\t1e+21\n"
    return table, [0, 2, 3], ["tx_a", "b", "c"], [7, 9], text, [0, 20, 20, 47]


def hand_estimates():
    """One cluster (ClusterID 4) of two paths, set i = {i}."""
    flat = dict(cluster_path_off=[0, 2], set_off=[0, 2], member_off=[0, 1, 2], members=[0, 1], abund_off=[0, 2], abundances=[1.5, 0.0],
                path_effective_length=[812.25, 1e-7])
    table = dict(member_tpm=[250000.0, 0.0], haplotype_prob=[1.0, 0.3333333333333333], read_count=[12.0, 99999999.5], tpm=[1e6, 0.125])
    per_path = b"a\t4\t1000\t812.25\t1.5\t250000\n" + b"bb\t4\t20\t1e-07\t0\t0\n"
    haplotype = b"a\t4\t1000\t812.25\t1\t12\t1000000\n" + b"bb\t4\t20\t1e-07\t0.33333333\t1e+08\t0.125\n"
    return flat, table, ["a", "bb"], [1000, 20], [4], per_path, haplotype
