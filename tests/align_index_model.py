"""Plain-Python model of the alignment-path index (include/rpvg_index.h) and the streams the tests put through it.

The model restates the reference line by line with Python's own containers:
  - addAlignmentPathsBufferToIndexes (src/main.cpp:200-237): the histogram gate, the normalisation of lists that hold one
    alignment, a dict keyed by the list's contents whose insertion order is the order of first occurrence;
  - PathClusters (src/path_clusters.cpp:12-86,163-207, addNodeClusters :88-262): every id set connects its members to its
    first one; a BFS from every unvisited path in ascending id order numbers the clusters, members ascending;
  - the caller's loop (src/main.cpp:731-754,811-827,846-857): a list's cluster is that of the first path of its first
    alignment, clusters are taken in descending (number of lists, cluster index) order, global ids become positions in the
    cluster's ascending member list.
A list is {"is_simple", "min_mapq", "noise_score", "aligns": [(score_sum, align_length, frag_length, [path id...])...]}.
"""
from collections import deque

import numpy as np


class InvalidList(ValueError):
    def __init__(self, index, why):
        super().__init__(f"list {index}: {why}")
        self.index = index


class IndexModel:
    def __init__(self, num_paths, is_single_end=False, frag_length_min_mapq=30, max_frag_length=1000, pre_frag_loc=300):
        assert max_frag_length < 65536
        self.num_paths = num_paths
        self.is_single_end = is_single_end
        self.frag_length_min_mapq = frag_length_min_mapq
        self.max_frag_length = max_frag_length
        self.pre_frag_loc = pre_frag_loc
        self.counts = [0] * (max_frag_length + 1)
        self.index = {}  # contents -> [multiplicity, first occurrence]; insertion order = order of first occurrence
        self.num_lists = 0

    def _counted(self, ls):
        return (not self.is_single_end) and bool(ls["is_simple"]) and ls["min_mapq"] >= self.frag_length_min_mapq  # :213

    def _check(self, i, ls):
        if len(ls["aligns"]) == 0:
            raise InvalidList(i, "no alignments")
        if ls["noise_score"] > 0:
            raise InvalidList(i, "positive noise score")
        for (_, _, _, ids) in ls["aligns"]:
            if len(ids) == 0:
                raise InvalidList(i, "an alignment without paths")
            if any(p >= self.num_paths for p in ids) or any(a >= b for a, b in zip(ids, ids[1:])):
                raise InvalidList(i, "path ids not ascending or out of range")
        if self._counted(ls) and not (0 < ls["aligns"][0][2] <= self.max_frag_length):
            raise InvalidList(i, "counted fragment length of 0 or above the maximum")

    def add(self, lists):
        """One chunk: all of it or, when a list is invalid, none of it."""
        keys = {}  # by object: the streams of the tests repeat their list objects
        for i, ls in enumerate(lists):
            if id(ls) not in keys:
                self._check(i, ls)
                keys[id(ls)] = None
        for ls in lists:
            if self._counted(ls):
                self.counts[ls["aligns"][0][2]] += 1  # :215, the original first alignment
            key = keys[id(ls)]
            if key is None:
                aligns = tuple((s, a, f, tuple(ids)) for (s, a, f, ids) in ls["aligns"])
                if len(aligns) == 1:  # :218-224 (size 2 with the noise entry)
                    aligns = ((1, 1, self.pre_frag_loc, aligns[0][3]),)
                key = keys[id(ls)] = (bool(ls["is_simple"]), ls["min_mapq"], ls["noise_score"], aligns)
            slot = self.index.setdefault(key, [0, self.num_lists])  # :226-227
            slot[0] += 1
            self.num_lists += 1

    def finish(self, extra_sets=()):
        P = self.num_paths
        # ---- PathClusters: adjacency through the anchor of every set, BFS in ascending id order
        adjacent = [set() for _ in range(P)]
        sets = [[p for al in key[3] for p in al[3]] for key in self.index] + [list(s) for s in extra_sets]
        for s in sets:
            for p in s[1:]:
                adjacent[s[0]].add(p)
                adjacent[p].add(s[0])
        path_to_cluster = [None] * P
        clusters = []
        for start in range(P):
            if path_to_cluster[start] is not None:
                continue
            members, queue = [], deque([start])
            path_to_cluster[start] = len(clusters)
            while queue:
                p = queue.popleft()
                members.append(p)
                for q in adjacent[p]:
                    if path_to_cluster[q] is None:
                        path_to_cluster[q] = len(clusters)
                        queue.append(q)
            clusters.append(sorted(members))
        K = len(clusters)
        # ---- the lists of every cluster, in order of first occurrence
        cluster_lists = [[] for _ in range(K)]
        for key, (count, first) in self.index.items():
            cluster_lists[path_to_cluster[key[3][0][3][0]]].append((key, count, first))  # :746-748
        order = sorted(((len(cluster_lists[c]), c) for c in range(K)), reverse=True)  # :811-827
        out = dict(cluster_read_off=[0], cluster_path_off=[0], read_count=[], read_min_mapq=[], read_noise_score=[], read_align_off=[0],
                   align_score_sum=[], align_length=[], align_frag_length=[], align_path_off=[0], align_path_idx=[], rank_cluster=[],
                   path_to_cluster=path_to_cluster, cluster_paths=[], first_occurrence=[])
        for _, c in order:
            local = {p: i for i, p in enumerate(clusters[c])}  # :855-857
            out["rank_cluster"].append(c)
            out["cluster_paths"].extend(clusters[c])
            out["cluster_path_off"].append(len(out["cluster_paths"]))
            for key, count, first in cluster_lists[c]:
                out["read_count"].append(count)
                out["read_min_mapq"].append(key[1])
                out["read_noise_score"].append(key[2])
                out["first_occurrence"].append(first)
                for (s, a, f, ids) in key[3]:
                    out["align_score_sum"].append(s)
                    out["align_length"].append(a)
                    out["align_frag_length"].append(f)
                    out["align_path_idx"].extend(local[p] for p in ids)
                    out["align_path_off"].append(len(out["align_path_idx"]))
                out["read_align_off"].append(len(out["align_score_sum"]))
            out["cluster_read_off"].append(len(out["read_count"]))
        arrays = {name: np.asarray(out[name], dtype=DTYPES[name]) for name in out}
        return dict(arrays=arrays, frag_counts=np.asarray(self.counts, dtype=np.uint32), num_lists=self.num_lists,
                    num_distinct=len(self.index), num_clusters=K, clusters=clusters)


DTYPES = dict(cluster_read_off=np.uint64, cluster_path_off=np.uint64, read_count=np.uint32, read_min_mapq=np.uint8,
              read_noise_score=np.int32, read_align_off=np.uint64, align_score_sum=np.int32, align_length=np.uint16,
              align_frag_length=np.uint16, align_path_off=np.uint64, align_path_idx=np.uint32, rank_cluster=np.uint32,
              path_to_cluster=np.uint32, cluster_paths=np.uint32, first_occurrence=np.uint64)


def run_model(params, chunks, extra_sets=()):
    """params: the keyword arguments of IndexModel; chunks: a sequence of sequences of lists."""
    model = IndexModel(**params)
    for chunk in chunks:
        model.add(chunk)
    return model.finish(extra_sets)


def model_clusters(result, effective_length=None):
    """The model's output as the cluster dicts of rpvg_amd.rows.AlignmentBatch.from_clusters; effective_length per GLOBAL path."""
    a = result["arrays"]
    out = []
    for r in range(result["num_clusters"]):
        p0, p1 = int(a["cluster_path_off"][r]), int(a["cluster_path_off"][r + 1])
        paths = [{"effective_length": 1.0 if effective_length is None else float(effective_length[int(p)])} for p in a["cluster_paths"][p0:p1]]
        reads = []
        for d in range(int(a["cluster_read_off"][r]), int(a["cluster_read_off"][r + 1])):
            aligns = []
            for j in range(int(a["read_align_off"][d]), int(a["read_align_off"][d + 1])):
                e0, e1 = int(a["align_path_off"][j]), int(a["align_path_off"][j + 1])
                aligns.append((int(a["align_score_sum"][j]), int(a["align_length"][j]), int(a["align_frag_length"][j]),
                               [int(x) for x in a["align_path_idx"][e0:e1]]))
            reads.append({"count": int(a["read_count"][d]), "min_mapq": int(a["read_min_mapq"][d]),
                          "noise_score": int(a["read_noise_score"][d]), "aligns": aligns})
        out.append({"paths": paths, "reads": reads})
    return out


# ---- streams ---------------------------------------------------------------------------------------------------------

def mk(aligns, is_simple=1, min_mapq=40, noise_score=-5):
    return {"is_simple": is_simple, "min_mapq": min_mapq, "noise_score": noise_score, "aligns": [(s, a, f, list(ids)) for (s, a, f, ids) in aligns]}


def chunked(lists, size):
    return [lists[i:i + size] for i in range(0, len(lists), size)] or [[]]


def hand_case():
    """Six lists over six paths, written out from the reference's lines (tests/test_align_index_model.py spells out the result)."""
    params = dict(num_paths=6, is_single_end=False, frag_length_min_mapq=30, max_frag_length=10, pre_frag_loc=5)
    lists = [
        mk([(10, 50, 7, [4, 5])], 1, 40, -3),                    # counted at 7; one alignment: becomes (1, 1, 5)
        mk([(8, 40, 6, [0]), (7, 40, 6, [1])], 1, 29, -3),      # mapq 29: not counted; two alignments stay as they are
        mk([(12, 60, 9, [4, 5])], 1, 40, -3),                    # counted at 9; equal to list 0 after normalisation
        mk([(10, 50, 7, [4, 5])], 0, 40, -3),                    # not simple: not counted, and a list of its own
        mk([(5, 30, 10, [2])], 1, 60, 0),                        # counted in the last bin
        mk([(8, 40, 6, [0]), (7, 40, 6, [1])], 1, 29, -3),      # list 1 again
    ]
    return params, lists


def random_stream(seed, num_paths, num_lists, num_templates, max_block=6, long_lists=0, max_frag_length=600, join_prob=0.05):
    """Lists drawn with replacement from `num_templates` distinct-ish templates.  The paths are cut into blocks of 1 .. max_block
    consecutive ids (a transcript's haplotype paths); a template's alignments take their paths from one block, sometimes from
    two neighbouring ones, which joins them.  `long_lists` templates get more than 16 entries; the first of them more than 64."""
    rng = np.random.default_rng(seed)
    blocks, p = [], 0
    while p < num_paths:
        n = int(rng.integers(1, max_block + 1))
        blocks.append(list(range(p, min(p + n, num_paths))))
        p += n
    templates = []
    for t in range(num_templates):
        b = int(rng.integers(0, len(blocks)))
        pool = list(blocks[b])
        if b + 1 < len(blocks) and rng.random() < join_prob:
            pool += blocks[b + 1]
        n_al = int(rng.integers(1, 4))
        if t < long_lists:
            pool = list(range(0, min(num_paths, 40)))
            n_al = 5 if t == 0 else 2
        aligns = []
        for _ in range(n_al):
            k = int(rng.integers(1, len(pool) + 1))
            if t < long_lists:
                k = min(len(pool), 14 if t == 0 else 9 + int(rng.integers(0, 6)))
            ids = sorted(int(x) for x in rng.choice(pool, size=k, replace=False))
            aligns.append((int(rng.integers(20, 300)), int(rng.integers(50, 300)), int(rng.integers(1, max_frag_length + 1)), ids))
        templates.append(mk(aligns, int(rng.random() < 0.8), int(rng.choice([0, 10, 29, 30, 60])), -int(rng.integers(0, 40))))
    picks = rng.integers(0, num_templates, size=num_lists)
    return [templates[int(i)] for i in picks]


def default_params(num_paths, **kw):
    p = dict(num_paths=num_paths, is_single_end=False, frag_length_min_mapq=30, max_frag_length=600, pre_frag_loc=277)
    p.update(kw)
    return p
