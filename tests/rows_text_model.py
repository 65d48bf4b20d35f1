"""Plain-Python model of the --write-probs dump as text (include/rpvg_text.h, rpvg_amd/csrc/rows_text_plan.hpp): the lines
ProbabilityClusterWriter::addCluster prints, every double by Python's '%.*g' with `-nan` spelled out (tests/table_text_model.fmt),
and the offsets of the L = 2 K + R lines.  The cases of tests/test_hip_rows_text.py."""
import math

import numpy as np

from tests import table_text_model as M

PATH_DIGITS = 8


def digits_of(prob_precision):
    """max(8, ceil(-log10(prob_precision))), the reference's choice (src/threaded_output_writer.cpp:40)"""
    return max(PATH_DIGITS, int(math.ceil(-math.log10(prob_precision))))


def flatten(clusters):
    """clusters: dicts of num_paths and rows, a row being (count, noise, [(prob, [idx, ...]), ...]) -> the arrays of
    rpvg_rows_text_input by name, without the path side."""
    cro, cpo, count, noise, rgo, prob, gio, idx = [0], [0], [], [], [0], [], [0], []
    for c in clusters:
        for row_count, row_noise, groups in c["rows"]:
            count.append(row_count)
            noise.append(row_noise)
            for p, members in groups:
                prob.append(p)
                idx += list(members)
                gio.append(len(idx))
            rgo.append(len(prob))
        cro.append(len(count))
        cpo.append(cpo[-1] + c["num_paths"])
    return dict(cluster_row_off=np.array(cro, dtype=np.uint64), cluster_path_off=np.array(cpo, dtype=np.uint64), row_count=np.array(count, dtype=np.uint32),
                row_noise=np.array(noise, dtype=np.float64), row_grp_off=np.array(rgo, dtype=np.uint64), grp_prob=np.array(prob, dtype=np.float64),
                grp_idx_off=np.array(gio, dtype=np.uint64), path_idx=np.array(idx, dtype=np.uint32))


def _raw(name):
    return name.encode() if isinstance(name, str) else bytes(name)


def lines(flat, names, lengths, effective_lengths, prob_precision=1e-8, num_align_lists=None, cluster_index=None):
    """The 2 K + R lines in file order as bytes; b"" for the lines of a cluster without rows or without paths."""
    digits = digits_of(prob_precision)
    cro, cpo = [int(x) for x in flat["cluster_row_off"]], [int(x) for x in flat["cluster_path_off"]]
    rgo, gio = [int(x) for x in flat["row_grp_off"]], [int(x) for x in flat["grp_idx_off"]]
    out = []
    for k in range(len(cro) - 1):
        printed = cro[k + 1] > cro[k] and cpo[k + 1] > cpo[k]
        marker = b"#\n" if num_align_lists is None else b"# %d %d\n" % (int(num_align_lists[k]), int(cluster_index[k]))
        paths = b" ".join(_raw(names[p]) + b"," + str(int(lengths[p])).encode() + b"," + M.fmt(effective_lengths[p], PATH_DIGITS).encode() for p in range(cpo[k], cpo[k + 1])) + b"\n"
        out += [marker if printed else b"", paths if printed else b""]
        for r in range(cro[k], cro[k + 1]):
            cells = [str(int(flat["row_count"][r])), M.fmt(flat["row_noise"][r], digits)]
            for g in range(rgo[r], rgo[r + 1]):
                cells.append(M.fmt(flat["grp_prob"][g], digits) + ":" + ",".join(str(int(i)) for i in flat["path_idx"][gio[g]:gio[g + 1]]))
            out.append((" ".join(cells) + "\n").encode() if printed else b"")
    return out


def rows_text(flat, names, lengths, effective_lengths, prob_precision=1e-8, num_align_lists=None, cluster_index=None):
    """(text, row_off [L + 1])"""
    return M.join(lines(flat, names, lengths, effective_lengths, prob_precision, num_align_lists, cluster_index))


def num_cells(flat):
    """C = 3 K + 3 P + 2 R + G + M"""
    K = len(flat["cluster_row_off"]) - 1
    return 3 * K + 3 * int(flat["cluster_path_off"][K]) + 2 * len(flat["row_count"]) + len(flat["grp_prob"]) + len(flat["path_idx"])


def row_of_cells(n, rng, num_paths, count=1):
    """A row of n >= 2 cells, the two head cells included: groups of random sizes that add up."""
    assert n >= 2
    groups, left = [], n - 2
    while left > 0:
        size = int(rng.integers(0, min(left, 7)))      # cells of the group: 1 + size
        groups.append((float(rng.random()), [int(x) for x in rng.integers(0, num_paths, size=size)]))
        left -= 1 + size
    return (count, float(rng.random()), groups)
