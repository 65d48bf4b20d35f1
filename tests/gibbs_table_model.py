"""Plain-Python restatement of ReadCountGibbsSamplesWriter::addSamples (rpvg_amd/host/io/estimates_writers.cpp; the reference's
src/threaded_output_writer.cpp:114-214) as a dense table: the model of the Gibbs samples table (include/rpvg_samples.h).

A cluster is a dict(num_paths, total_count, blocks); a block a dict(ids, noise, abund): strictly ascending cluster-local path ids,
n noise samples and n rows of len(ids) abundance samples (sample-major, as CountSamples::abundance_samples).  Blocks without samples
are what the estimator drops before the writer sees them; the model drops them where the estimator does.

The noise chains are Python float loops in the writer's order: no sum(), no sorting, no fsum.
"""
import numpy as np


# ---- the writer's loops ------------------------------------------------------------------------------------------------------------

def table(clusters, N):
    """dict(samples [P, N], listed [P], noise_counts [N]) as the writer prints them: a listed row is the writer's row, every other
    cell is +0.0."""
    assert N >= 1
    P = sum(c["num_paths"] for c in clusters)
    rows = [[0.0] * N for _ in range(P)]
    listed = [0] * P
    noise_counts = [0.0] * N
    p0 = 0
    for cluster in clusters:
        seen = [b for b in cluster["blocks"] if len(b["noise"]) > 0]   # src/path_abundance_estimator.cpp:1455
        if not seen:
            for idx in range(N):
                noise_counts[idx] += cluster["total_count"]
            p0 += cluster["num_paths"]
            continue
        no_column = None
        index = [[] for _ in range(cluster["num_paths"])]   # path_gibbs_sampling_index
        idx = 0
        for i, block in enumerate(seen):
            assert len(block["abund"]) == len(block["noise"]) and all(len(r) == len(block["ids"]) for r in block["abund"])
            for noise_sample in block["noise"]:
                noise_counts[idx] += noise_sample
                idx += 1
            for j, path in enumerate(block["ids"]):
                if not index[path]:
                    index[path] = [no_column] * len(seen)
                index[path][i] = j
        assert idx <= N
        while idx < N:
            noise_counts[idx] += cluster["total_count"]
            idx += 1
        for path, columns in enumerate(index):
            if not columns:
                continue
            listed[p0 + path] = 1
            row, at = rows[p0 + path], 0
            for j, column in enumerate(columns):
                block = seen[j]
                for k in range(len(block["noise"])):
                    row[at] = 0.0 if column is no_column else block["abund"][k][column]
                    at += 1
            # (the rest of the row is the writer's "\t0")
        p0 += cluster["num_paths"]
    return dict(samples=np.array(rows, dtype=np.float64).reshape(P, N), listed=np.array(listed, dtype=np.uint8),
                noise_counts=np.array(noise_counts, dtype=np.float64))


def text(clusters, N, names, cluster_ids, unaligned_read_count=0):
    """The file the writer produces (before gzip): the header, the listed rows and the `Unknown` row, numbers as `%.8g`."""
    t = table(clusters, N)

    def number(x):
        return "%.8g" % x

    lines = ["Name\tClusterID" + "".join(f"\tReadCountSample_{i + 1}" for i in range(N))]
    g = 0
    for k, cluster in enumerate(clusters):
        for _ in range(cluster["num_paths"]):
            if t["listed"][g]:
                lines.append(f"{names[g]}\t{cluster_ids[k]}" + "".join("\t" + number(x) for x in t["samples"][g].tolist()))
            g += 1
    lines.append("Unknown\t0" + "".join("\t" + number(x + unaligned_read_count) for x in t["noise_counts"].tolist()))
    return "\n".join(lines) + "\n"


def flatten(clusters, N):
    """The arrays of rpvg_gibbs_flat (keyword arguments of rpvg_amd.gibbs_table.FlatGibbs)."""
    goff, poff, path, noff, noise, aoff, abund, cpo, total = [0], [0], [], [0], [], [0], [], [0], []
    for cluster in clusters:
        for block in cluster["blocks"]:
            path.extend(block["ids"])
            poff.append(len(path))
            noise.extend(block["noise"])
            noff.append(len(noise))
            for row in block["abund"]:
                abund.extend(row)
            aoff.append(len(abund))
        goff.append(len(poff) - 1)
        cpo.append(cpo[-1] + cluster["num_paths"])
        total.append(cluster["total_count"])
    return dict(gibbs_off=goff, gibbs_path_off=poff, gibbs_path=path, gibbs_noise_off=noff, gibbs_noise=noise, gibbs_abund_off=aoff,
                gibbs_abund=abund, cluster_path_off=cpo, total_count=total, num_gibbs_samples=N)


def route_of(lim, cluster):
    widest = max([len(b["ids"]) for b in cluster["blocks"]], default=0)
    return 0 if cluster["num_paths"] <= lim.resident_paths and widest <= lim.resident_columns else 1


def clusters_by_route(lim, clusters):
    out = [0, 0]
    for cluster in clusters:
        out[route_of(lim, cluster)] += 1
    return out


# ---- the hand case -----------------------------------------------------------------------------------------------------------------

def hand_case():
    """Cluster A: three paths, blocks {0,2} with two samples, {1} with none and {1,2} with one; N = 4, so one tail column, and path 1
    is listed only through the third block.  Cluster B: two paths, no blocks; its total_count enters all four columns.
    Returns (clusters, N, expected): the expected table written out from the writer's lines, not computed."""
    a = dict(num_paths=3, total_count=100.0, blocks=[
        dict(ids=[0, 2], noise=[1.5, 2.5], abund=[[10.0, 30.0], [11.0, 31.0]]),
        dict(ids=[1], noise=[], abund=[]),
        dict(ids=[1, 2], noise=[4.25], abund=[[20.5, 32.5]])])
    b = dict(num_paths=2, total_count=7.0, blocks=[])
    expected = dict(
        #        block {0,2}: s0    s1    block {1,2}: s0   tail
        samples=[[10.0, 11.0, 0.0, 0.0],    # path 0: column 0 of the first block, not in the third
                 [0.0, 0.0, 20.5, 0.0],     # path 1: not in the first block, column 0 of the third
                 [30.0, 31.0, 32.5, 0.0],   # path 2: column 1 of both
                 [0.0, 0.0, 0.0, 0.0],      # cluster B: nothing listed
                 [0.0, 0.0, 0.0, 0.0]],
        listed=[1, 1, 1, 0, 0],
        # 0.0 + A's noise samples 1.5, 2.5, 4.25 and then A's total_count in the tail column; + B's total_count in every column
        noise_counts=[1.5 + 7.0, 2.5 + 7.0, 4.25 + 7.0, 100.0 + 7.0])
    return [a, b], 4, expected


# ---- cases -------------------------------------------------------------------------------------------------------------------------

class Values:
    """Source values that are non-zero and pairwise distinct across everything one instance hands out."""

    def __init__(self, start=1):
        self.at = start

    def take(self, n):
        out = [(self.at + i) * 0.12345678901234 + 1.0 for i in range(n)]
        self.at += n
        return out


def make_block(values, ids, n):
    flat = values.take(n * len(ids))
    return dict(ids=list(ids), noise=values.take(n), abund=[flat[s * len(ids):(s + 1) * len(ids)] for s in range(n)])


def spread_ids(rng, num_paths, columns):
    return sorted(int(x) for x in rng.choice(num_paths, size=columns, replace=False))


def make_cluster(values, rng, num_paths, block_shapes):
    """block_shapes: (columns, samples) per block, the ids drawn from the cluster's paths."""
    return dict(num_paths=num_paths, total_count=values.take(1)[0] + 1000.0,
                blocks=[make_block(values, spread_ids(rng, num_paths, c), n) for c, n in block_shapes])


def source_values(clusters):
    out = []
    for cluster in clusters:
        for block in cluster["blocks"]:
            for row in block["abund"]:
                out.extend(row)
    return out


def scatter_cases(lim):
    """name -> (clusters, N): the shapes of tests/test_hip_gibbs_table.py.  In every case all abundance samples are non-zero and
    pairwise distinct (tests/test_gibbs_table_model.py asserts it): a cell read from the wrong place, or left unwritten, cannot
    compare equal."""
    rng = np.random.default_rng(20261019)
    values = Values()
    ts = lim.sample_tile
    cases = {}
    widths = (1, 2, 31, 32, 33, 63, 64, 65)
    counts = sorted({1, 63, 64, 65, ts - 1, ts, ts + 1})
    # every width with every count, a cluster each; a second block of another width shares the rows
    cases["widths_and_counts"] = ([make_cluster(values, rng, c + 3, [(c, n), (min(c, 2), 1)]) for c in widths for n in counts], max(counts) + 1)
    N = 2 * ts + 5
    cases["tails"] = ([make_cluster(values, rng, 9, [(4, ts), (3, ts + 5)]),                   # S_k = N: no tail
                       make_cluster(values, rng, 9, [(4, ts), (3, ts + 4)]),                   # S_k = N - 1
                       make_cluster(values, rng, 9, [(4, 0), (9, 0)]),                         # all blocks empty: nothing listed
                       make_cluster(values, rng, 5, [(2, 0), (3, 7), (1, 0), (5, 2)])], N)     # empty blocks between others
    cases["one_sample"] = ([make_cluster(values, rng, 6, [(3, 1)]), make_cluster(values, rng, 4, []), make_cluster(values, rng, 70, [(65, 1)])], 1)
    cases["many_blocks"] = ([make_cluster(values, rng, 40, [(2, 1)] * 200)], 200)
    cases["odd_clusters"] = ([dict(num_paths=0, total_count=3.5, blocks=[]), make_cluster(values, rng, 300, [(2, 5), (1, 3)]),
                              dict(num_paths=0, total_count=4.5, blocks=[]), make_cluster(values, rng, 2, [(2, 2)])], 9)
    cases["single_cluster"] = ([make_cluster(values, rng, 12, [(5, 3), (7, 4)])], 8)
    cases["empty_batch"] = ([], 3)
    limits_case = []
    for d in (-1, 0, 1):
        limits_case.append(make_cluster(values, rng, lim.resident_paths + d, [(10, 3), (3, 2)]))
        limits_case.append(make_cluster(values, rng, 100, [(lim.resident_columns + d, ts + 1), (5, 2)]))
    limits_case.append(make_cluster(values, rng, lim.resident_paths, [(lim.resident_columns, 2)]))
    limits_case.append(make_cluster(values, rng, lim.resident_paths + 1, [(lim.resident_columns + 1, 2), (lim.resident_paths + 1, 1)]))
    limits_case.append(make_cluster(values, rng, lim.global_paths * 2 + 7, [(lim.global_paths + 70, 3)]))   # several segments, a wide block
    limits_case.append(make_cluster(values, rng, 3, [(2, 2)]))   # a small cluster behind the large ones
    cases["route_limits"] = (limits_case, ts + 9)
    return cases


# ---- the order of the noise chains -------------------------------------------------------------------------------------------------

def sequential_sum(values):
    acc = 0.0
    for v in values:
        acc += v
    return acc


def reversed_sum(values):
    acc = 0.0
    for v in reversed(values):
        acc += v
    return acc


def pairwise_sum(values):
    values = list(values)
    if not values:
        return 0.0
    while len(values) > 1:
        values = [values[i] + values[i + 1] if i + 1 < len(values) else values[i] for i in range(0, len(values), 2)]
    return values[0]


def column_addends(clusters, N, s):
    """What the clusters add to noise column s, in cluster order."""
    out = []
    for cluster in clusters:
        noise = [x for b in cluster["blocks"] for x in b["noise"]]
        out.append(noise[s] if s < len(noise) else cluster["total_count"])
    return out


def noise_case(K, N=70, first_seed=0):
    """K clusters whose noise samples and total counts have magnitudes from 1e-3 to 1e9; some with fewer than N samples, some with
    none.  For K >= 3 the seed is searched until some column's chain differs in its last bits from the reversed chain and from a
    pairwise sum (for K <= 2 every order gives the same double: a + b is b + a)."""
    seed = first_seed
    while True:
        rng = np.random.default_rng(seed)

        def magnitudes(n):
            return [float(x) for x in 10.0 ** rng.uniform(-3.0, 9.0, size=n)]

        clusters = []
        for k in range(K):
            n = [N, N - 1, 0, int(rng.integers(1, N + 1))][k % 4]
            ids = [0, 1]
            blocks = []
            if n:
                first = int(rng.integers(0, n + 1))
                for part in (first, n - first):
                    blocks.append(dict(ids=ids, noise=magnitudes(part), abund=[magnitudes(2) for _ in range(part)]))
            clusters.append(dict(num_paths=2, total_count=magnitudes(1)[0], blocks=blocks))
        if K < 3 or order_matters(clusters, N):
            return clusters, N, seed
        seed += 1


def order_matters(clusters, N):
    for s in range(N):
        addends = column_addends(clusters, N, s)
        forward = sequential_sum(addends)
        if forward != reversed_sum(addends) and forward != pairwise_sum(addends):
            return True
    return False
