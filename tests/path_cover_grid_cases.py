"""Clusters at the edges of the minimum path cover's whole-GPU route (rpvg_amd/csrc/path_cover_grid.hip; test-only, plain
Python and numpy, no GPU).  The model, the margin and the generators are those of tests/path_cover_cases.py; the numbers of the
route — the widest cluster of the workgroup route, the rounds between two looks at the control record, the geometry of the
pick kernel — are read from the library's plan (rpvg_hip_cover_limits: rpvg_amd/csrc/cover_plan.hpp), so a case sits at an edge
of the code as it is built.

Every case has a decision margin of at least MIN_MARGIN = 1e-9 in the model (tests/test_path_cover_grid_cases.py asserts it).
The device adds a weight's R terms, all of one sign, one after the other: within R * 2^-53 relative of the exact sum.  The
tallest column here has 129 rows but for the threshold case, whose planted columns have THRESHOLD_ROWS / 8 rows (4 096 with the
plan as it is): 4 096 * 2^-53 ~ 4.5e-13, three orders of magnitude below the margin (the bound still lies two orders below
1e-9 at 10^5 rows).
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from rpvg_amd import hip
from tests import path_cover_cases as pcc
from tests.path_cover_cases import Cluster, CoverCase

LIMITS = hip.cover_limits()
CHUNK = int(LIMITS.chunk_rounds)
MAX_WORKGROUP_PATHS = int(LIMITS.workgroup_max_paths)
PICK_BLOCK = int(LIMITS.pick_block)
PICK_TILE = PICK_BLOCK * int(LIMITS.pick_per_thread)   # consecutive paths of one workgroup of the pick kernel
WIDTH_ONLY = 2 ** 64 - 1

WIDE_PATHS = (MAX_WORKGROUP_PATHS + 1, 16384, 65537)
TWIN_PATHS = 3000
TWIN_SEED = 9500   # the first seed from 9500 that passes twin_ok for every pair below (the same cluster up to the twins' places)
TALL_PATHS = 300
TALL_CHAINS = (63, 64, 65, 129)   # terms of a planted column: either side of the 64 terms the lanes of the weight kernel hold


def twin_pairs() -> Dict[str, Tuple[int, int]]:
    """The twins at the edges of the pick kernel's geometry: a workgroup takes PICK_TILE consecutive paths, thread t the paths
    t, t + PICK_BLOCK, ... of them."""
    pairs = {"last_thread_and_first_of_the_next_workgroup": (PICK_TILE - 1, PICK_TILE),
             "end_of_a_stride_and_the_next_workgroup": (PICK_BLOCK - 1, PICK_TILE),
             "second_and_third_workgroup": (2 * PICK_TILE - 1, 2 * PICK_TILE),
             "first_and_last_workgroup": (0, TWIN_PATHS - 1)}
    if PICK_TILE > PICK_BLOCK:
        pairs["both_on_one_thread"] = (0, PICK_BLOCK)
    assert all(a < b < TWIN_PATHS for a, b in pairs.values()) and (TWIN_PATHS - 1) // PICK_TILE >= 2
    return pairs


def wide_twin_cluster(seed: int, pair: Tuple[int, int]) -> Cluster:
    """pcc.reduction_cluster at N = 3 000: the twins at `pair`, a third path between them in their group, twenty decoys."""
    rng = np.random.default_rng(seed)
    rest = [j for j in range(TWIN_PATHS) if j not in pair]
    picked = [int(x) for x in rng.choice(rest, size=21, replace=False)]
    return pcc.twin_cluster(seed, 48, TWIN_PATHS, first=pair[0], second=pair[1], middle=picked[0], decoys=sorted(picked[1:]))


def twin_ok(cluster: Cluster, first: int, second: int) -> bool:
    """What a twin case needs here: the margin, the first twin in the model's cover and the second not."""
    m = pcc.cover_model(cluster)
    return m.margin >= pcc.MIN_MARGIN and first in m.cover and second not in m.cover


def find_twin_seed(start: int = 9500) -> int:
    """How TWIN_SEED was chosen (not run by any test)."""
    seed = start
    while not all(twin_ok(wide_twin_cluster(seed, p), *p) for p in twin_pairs().values()):
        seed += 1
    return seed


def tall_cluster(seed: int, n_paths: int, n_rows: int) -> Cluster:
    """pcc.wide_cluster with n_rows rows: row r belongs to planted path r mod 8 (probability 0.3 .. 0.6), next to up to two of
    40 decoys (probability below 0.01): the cover is the planted paths, and a planted column has n_rows / 8 terms."""
    rng = np.random.default_rng(seed)
    planted = pcc.wide_planted(n_paths)
    pool = [int(x) for x in rng.choice([j for j in range(n_paths) if j not in planted], size=min(40, n_paths - len(planted)), replace=False)]
    noise = pcc._noise(rng, n_rows)
    rows = []
    for r in range(n_rows):
        scale = 1.0 - noise[r]
        groups = [(float(rng.uniform(0.3, 0.6) * scale), [planted[r % len(planted)]])]
        for j in rng.choice(pool, size=int(rng.integers(0, 3)), replace=False):
            groups.append((float(rng.uniform(1e-3, 1e-2) * scale), [int(j)]))
        rows.append(pcc._row(rng.integers(1, 21), noise[r], groups))
    return Cluster(n_paths, rows)


def work_of(cluster: Cluster) -> int:
    """rows + entries, as the plan counts a cluster's work."""
    return len(cluster.rows) + sum(len(members) for _, _, groups in cluster.rows for _, members in groups)


# The cluster of the work threshold: narrower than the workgroup route's limit, so only its work can send it over the whole GPU.
# The library's default is read from the plan; where that is "width only" the tests pass this cluster's own work as the threshold.
THRESHOLD_ROWS = 8192 if int(LIMITS.default_grid_min_work) == WIDTH_ONLY else int(LIMITS.default_grid_min_work) // 2   # (work ~ 3 per row)
THRESHOLD_PATHS = 600


def threshold_cluster() -> Cluster:
    return tall_cluster(7300, THRESHOLD_PATHS, THRESHOLD_ROWS)


def _cases() -> List[CoverCase]:
    cases: List[CoverCase] = []
    for n in WIDE_PATHS:
        cases.append(CoverCase(f"grid_wide_{n}", "grid_wide", lambda n=n: pcc.wide_cluster(5000 + n, n)))
    for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        cases.append(CoverCase(f"grid_long_cover_{n}", "grid_long_cover", lambda n=n: pcc.long_cover_cluster(6100, n)))
    for name, pair in twin_pairs().items():
        cases.append(CoverCase(f"grid_twins_{name}", "grid_twins", lambda pair=pair: wide_twin_cluster(TWIN_SEED, pair), pair))
    for chain in TALL_CHAINS:
        cases.append(CoverCase(f"grid_tall_{chain}", "grid_tall", lambda chain=chain: tall_cluster(7400 + chain, TALL_PATHS, 8 * chain)))
    cases.append(CoverCase("grid_noise_one", "noise_one", lambda: pcc.noise_one_cluster(7001)))
    cases.append(CoverCase("grid_nothing_to_cover", "nothing_to_cover", lambda: pcc.nothing_to_cover_cluster(7101)))
    cases.append(CoverCase("grid_single_path", "single_path", lambda: pcc.single_path_cluster(7201, False)))
    cases.append(CoverCase("grid_single_path_noise_one", "single_path", lambda: pcc.single_path_cluster(7202, True)))
    return cases


CASES: List[CoverCase] = _cases()
BY_NAME: Dict[str, CoverCase] = {c.name: c for c in CASES}
TWIN_CASES = [c for c in CASES if c.twins is not None]
THRESHOLD_CASE = CoverCase("grid_threshold", "grid_threshold", threshold_cluster)

# Both routes on one input: 200 small clusters with no margin requirement (the weights have the same bits on both routes, so
# whatever a round decides it decides on both).
RANDOM_SEEDS = tuple(range(8200, 8400))


def random_small_cluster(seed: int) -> Cluster:
    """2 to 40 paths, 1 to 300 rows; a row holds 1 to 4 probability groups of 1 to 3 paths, counts 1 .. 20, now and then a row
    whose noise is 1."""
    rng = np.random.default_rng(seed)
    n_paths = int(rng.integers(2, 41))
    n_rows = int(rng.integers(1, 301))
    noise = pcc._noise(rng, n_rows)
    rows = []
    for r in range(n_rows):
        nz = 1.0 if rng.random() < 0.03 else float(noise[r])
        members = [int(x) for x in rng.permutation(n_paths)[:int(rng.integers(1, min(n_paths, 8) + 1))]]
        probs = sorted(float(x) for x in rng.uniform(1e-3, 0.9, size=4) * (1.0 - min(nz, 0.5)))
        groups, at = [], 0
        for prob in probs:
            take = int(rng.integers(1, 4))
            if at < len(members):
                groups.append((prob, members[at:at + take]))
            at += take
        rows.append(pcc._row(rng.integers(1, 21), nz, groups))
    return Cluster(n_paths, rows)
