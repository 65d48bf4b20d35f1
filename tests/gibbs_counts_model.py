"""The read-count Gibbs sampler (-n) restated draw for draw in plain Python (test-only).

A reading of rpvg_amd/csrc/gibbs_random.hpp (Philox, sampleBinomial, sampleGamma), gibbsReadCountKernel
(rpvg_amd/csrc/em_sparse.hip: one workgroup per problem) and rpvg_amd/csrc/gibbs_grid.hip (the whole GPU per problem), in
doubles and in the kernels' order of operations.  The sampler is deterministic: Philox4x32-10 keyed by the problem's seed,
the counter laid out by the kernels.

  one workgroup   thread t of problem p owns ONE stream for the whole run: key = seed, counter = [block, 0, t, p].  Per
                  iteration it draws the chains of binomials of rows t, t + 256, ... and then the gammas of columns
                  t, t + 256, ... (the noise column is the last one), all from that stream.
  grid            a fresh stream per (iteration, row or column, domain): counter = [block, iteration, index, domain].
                  domain 0: the chain of binomials of a row; domain 1: the categorical draws of a row of at most 64 reads
                  (read k takes uniform k & 1 of block k >> 1); domain 2: the gamma of a column.

What the model cannot share with the device are the last bits of log, exp, lgamma, fused multiply-adds and the order of a
few sums.  They move the two sides of a comparison by ~1e-12 relative at the most, so the model records, for every
comparison that chooses a branch, the relative distance |lhs - rhs| / max(|lhs|, |rhs|) of its two sides (Margin): a run
whose smallest margin is far above that takes the same branches on the device, draws the same integer counts, and its
gammas then differ by a few ulp.
"""
from __future__ import annotations

import math

import numpy as np

MASK32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
TWO_POW_MINUS_53 = 1.0 / 9007199254740992.0

BLOCK = 256                    # threads of a workgroup, columns of an update workgroup
CATEGORICAL_MAX_READS = 64     # kCategoricalMaxReads
MIN_GIBBS_ABUNDANCE = 1e-8     # kMinGibbsAbundance
GRID_LDS_LIMIT = 64 * 1024     # kGibbsGridLdsLimit
DOMAIN_ROW_CHAIN, DOMAIN_ROW_CATEGORICAL, DOMAIN_COLUMN = 0, 1, 2


def philox4x32_10(ctr, key):
    """Ten rounds of Philox4x32 (Philox::round / refill)."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0 = PHILOX_M0 * c0
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK32, p1 & MASK32, ((p0 >> 32) ^ c3 ^ k1) & MASK32, p0 & MASK32
        k0 = (k0 + PHILOX_W0) & MASK32
        k1 = (k1 + PHILOX_W1) & MASK32
    return (c0, c1, c2, c3)


def cospi(t: float) -> float:
    """cos(pi t) for t in [0, 2] with the argument reduced exactly, as the device's cospi does."""
    if t > 1.0:
        t = 2.0 - t
    if t <= 0.25:
        return math.cos(math.pi * t)
    if t < 0.75:
        return math.sin(math.pi * (0.5 - t))
    return -math.cos(math.pi * (1.0 - t))


def relative_margin(lhs: float, rhs: float) -> float:
    scale = max(abs(lhs), abs(rhs))
    return abs(lhs - rhs) / scale if scale > 0.0 else math.inf


class Margin:
    """The smallest decision margin of a run and where it occurred."""

    def __init__(self):
        self.smallest = math.inf
        self.where = None
        self.decisions = 0
        self.kinds = {}  # decisions per kind of comparison
        self.context = None  # set by the kernels' models: (iteration, what, index)

    def record(self, m: float, lhs: float, rhs: float, what: str):
        self.decisions += 1
        self.kinds[what] = self.kinds.get(what, 0) + 1
        if m < self.smallest:
            self.smallest = m
            self.where = (what, self.context, lhs, rhs)

    def note(self, lhs: float, rhs: float, what: str):
        self.record(relative_margin(lhs, rhs), lhs, rhs, what)


class Stream:
    """Philox of gibbs_random.hpp: the words of a block are handed out as out[3], out[2], out[1], out[0]."""

    def __init__(self, seed: int, ctr):
        self.key = (seed & MASK32, (seed >> 32) & MASK32)
        self.ctr = [int(c) & MASK32 for c in ctr]
        self.out = (0, 0, 0, 0)
        self.have = 0
        self.uniforms = 0  # handed out so far

    def refill(self):
        self.out = philox4x32_10(self.ctr, self.key)
        self.ctr[0] = (self.ctr[0] + 1) & MASK32
        if self.ctr[0] == 0:
            self.ctr[1] = (self.ctr[1] + 1) & MASK32
        self.have = 4

    def next(self) -> int:
        if self.have == 0:
            self.refill()
        self.have -= 1
        return self.out[self.have]

    def uniform(self) -> float:
        hi = self.next()
        lo = self.next()
        self.uniforms += 1
        return (float(((hi << 32) | lo) >> 11) + 0.5) * TWO_POW_MINUS_53

    def normal(self) -> float:
        u1 = self.uniform()
        u2 = self.uniform()
        return math.sqrt(-2.0 * math.log(u1)) * cospi(2.0 * u2)


class GridUniforms:
    """A stream that replays a given sequence of uniforms (the law tests feed the inversion a regular grid)."""

    def __init__(self, values):
        self.values = list(values)
        self.uniforms = 0

    def uniform(self) -> float:
        u = self.values[self.uniforms]
        self.uniforms += 1
        return u


def sample_binomial(stream, n: int, p: float, margin: Margin | None = None):
    """sampleBinomial.  Returns (k, smallest margin of this draw's comparisons)."""
    own = [math.inf]

    def note(lhs, rhs, what):
        m = relative_margin(lhs, rhs)
        if m < own[0]:
            own[0] = m
        if margin is not None:
            margin.record(m, lhs, rhs, what)

    if n == 0 or not (p > 0.0):
        return 0, own[0]
    note(p, 1.0, "binomial p >= 1")
    if p >= 1.0:
        return n, own[0]
    note(p, 0.5, "binomial p > 0.5")
    flip = p > 0.5
    if flip:
        p = 1.0 - p
    q = 1.0 - p
    ratio = p / q
    note(n * p, 16.0, "binomial n p < 16")
    if n * p < 16.0:
        pmf = math.exp(n * math.log(q))
        u = stream.uniform()
        k = 0
        while k < n:
            note(u, pmf, "binomial u > pmf")
            if not (u > pmf):
                break
            u -= pmf
            pmf *= ratio * (float(n - k) / (k + 1.0))
            k += 1
    else:
        x = (n + 1.0) * p
        mode = int(x)
        # (the truncation chooses where the walk starts)
        note(x, float(mode), "binomial mode")
        note(x, float(mode + 1), "binomial mode")
        log_pmf_mode = (math.lgamma(n + 1.0) - math.lgamma(mode + 1.0) - math.lgamma(n - mode + 1.0) + mode * math.log(p)
                        + (n - mode) * math.log(q))
        pmf_mode = math.exp(log_pmf_mode)
        u = stream.uniform()
        up = down = pmf_mode
        ku = kd = mode
        k = mode
        note(u, pmf_mode, "binomial u > pmf")
        if u > pmf_mode:
            u -= pmf_mode
            while True:
                moved = False
                if ku < n:
                    up *= ratio * (float(n - ku) / (ku + 1.0))
                    ku += 1
                    moved = True
                    note(u, up, "binomial u <= up")
                    if u <= up:
                        k = ku
                        break
                    u -= up
                if kd > 0:
                    down *= (float(kd) / (n - kd + 1.0)) / ratio
                    kd -= 1
                    moved = True
                    note(u, down, "binomial u <= down")
                    if u <= down:
                        k = kd
                        break
                    u -= down
                if not moved:
                    k = mode
                    break
    return (n - k if flip else k), own[0]


def sample_gamma(stream, shape: float, margin: Margin | None = None):
    """sampleGamma (Marsaglia and Tsang; shape >= 1).  Returns (draw, smallest margin of this draw's comparisons)."""
    own = [math.inf]

    def note(lhs, rhs, what):
        m = relative_margin(lhs, rhs)
        if m < own[0]:
            own[0] = m
        if margin is not None:
            margin.record(m, lhs, rhs, what)

    d = shape - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    while True:
        x = stream.normal()
        cx = c * x
        v = 1.0 + cx
        # v <= 0 is 1 <= -c x
        note(1.0, -cx, "gamma v <= 0")
        if v <= 0.0:
            continue
        v = v * v * v
        u = stream.uniform()
        lhs = math.log(u)
        rhs = 0.5 * x * x + d - d * v + d * math.log(v)
        note(lhs, rhs, "gamma log u < squeeze")
        if lhs < rhs:
            return d * v, own[0]


# ---- the compacted CSR the kernels read (fillSegmentsKernel<true>, em_sparse.hip) -------------------------------------

class CompactedCsr:
    """Kept rows in batch order, their kept entries in batch order, values (P / rowsum) * (1 - noise) with the reference's two
    roundings (np_oracle.add_noise_and_normalize; the row sum runs over the kept entries in batch order), the read counts of
    the rows without a selected path in zero_mass, of all rows in total_mass."""

    def __init__(self, off, count, noise, col, val, zero_mass, total_mass, columns):
        self.off, self.count, self.noise, self.col, self.val = off, count, noise, col, val
        self.zero_mass, self.total_mass, self.columns = zero_mass, total_mass, columns

    @property
    def rows(self):
        return len(self.count)

    @property
    def entries(self):
        return len(self.col)


def compacted_csr(batch, cluster: int, columns) -> CompactedCsr:
    n_paths = int(batch.cluster_path_off[cluster + 1] - batch.cluster_path_off[cluster])
    column_of = np.full(n_paths, -1, dtype=np.int64)
    column_of[np.asarray(columns, dtype=np.int64)] = np.arange(len(columns))
    off, count, noise, col, val = [0], [], [], [], []
    zero_mass = total_mass = 0.0
    for r in range(int(batch.cluster_row_off[cluster]), int(batch.cluster_row_off[cluster + 1])):
        c = float(batch.row_count[r])
        total_mass += c
        kept = []
        for g in range(int(batch.row_grp_off[r]), int(batch.row_grp_off[r + 1])):
            prob = float(batch.grp_prob[g])
            for e in range(int(batch.grp_idx_off[g]), int(batch.grp_idx_off[g + 1])):
                j = int(column_of[int(batch.path_idx[e])])
                if j >= 0:
                    kept.append((j, prob))
        if not kept:
            zero_mass += c
            continue
        rowsum = 0.0
        for _, prob in kept:
            rowsum += prob
        nz = float(batch.row_noise[r])
        keep = 1.0 - nz
        for j, prob in kept:
            col.append(j)
            val.append((prob / rowsum) * keep)
        off.append(len(col))
        count.append(c)
        noise.append(nz)
    return CompactedCsr(np.asarray(off, dtype=np.int64), np.asarray(count), np.asarray(noise), np.asarray(col, dtype=np.int64),
                        np.asarray(val), zero_mass, total_mass, len(columns))


# ---- the two kernels' models --------------------------------------------------------------------------------------------

class Run:
    """Samples of a model run: noise [n], abundances [n x columns], the integer counts of every iteration [its x (columns + 1)]
    (noise last), the margin record and the route the host takes."""

    def __init__(self, noise, abundances, counts, margin, route):
        self.noise, self.abundances, self.counts, self.margin, self.route = noise, abundances, counts, margin, route


def _chain_of_binomials(stream, reads, terms, s, counts, margin):
    """The reference's chain of binomials over a row's terms val * a (entries in order); returns the reads left for noise."""
    remaining = reads
    remaining_prob = 1.0
    for j, term in terms:
        if remaining == 0:
            break
        prob = term / s
        if prob > 0.0:
            drawn, _ = sample_binomial(stream, remaining, min(1.0, prob / remaining_prob), margin)
            counts[j] += drawn
            remaining -= drawn
        remaining_prob -= prob
    return remaining


def _categorical_draws(seed, iteration, row, reads, terms, s, counts, margin):
    """A row of at most 64 reads: read k takes uniform k & 1 of block k >> 1 of the row's categorical stream, t_k = u_k s, and
    lands on the first entry whose inclusive prefix sum of the row's terms exceeds t_k; behind the last one, on noise."""
    noise_col = len(counts) - 1
    incl = []
    run = 0.0
    for _, term in terms:
        run += term
        incl.append(run)
    stream = None
    for k in range(reads):
        if (k & 1) == 0:
            stream = Stream(seed, [k >> 1, iteration, row, DOMAIN_ROW_CATEGORICAL])
        tk = stream.uniform() * s
        lo, hi = 0, len(incl)  # first entry with tk < incl
        while lo < hi:
            mid = (lo + hi) >> 1
            if tk < incl[mid]:
                hi = mid
            else:
                lo = mid + 1
        if margin is not None:
            if lo > 0:
                margin.note(tk, incl[lo - 1], "categorical t < incl")
            if lo < len(incl):
                margin.note(tk, incl[lo], "categorical t < incl")
        if lo < len(incl):
            counts[terms[lo][0]] += 1
        else:
            counts[noise_col] += 1


def _wave_sum(values):
    """A wavefront's sum of one double per lane (waveSumF64: butterflies inside rows of 16 lanes, then the four rows)."""
    v = list(values) + [0.0] * (64 - len(values))
    rows = []
    for r in range(4):
        x = v[16 * r:16 * r + 16]
        x = [x[i] + x[i ^ 1] for i in range(16)]
        x = [x[i] + x[i ^ 2] for i in range(16)]
        x = [x[i] + x[7 - i if i < 8 else 23 - i] for i in range(16)]  # row_half_mirror
        x = [x[i] + x[15 - i] for i in range(16)]                      # row_mirror
        rows.append(x[0])
    return (rows[0] + rows[1]) + (rows[2] + rows[3])


def _block_sum(values):
    """gibbsBlockSum over up to 256 values: a wave sum per 64 threads, the four waves in order."""
    v = list(values) + [0.0] * (BLOCK - len(values))
    total = _wave_sum(v[0:64])
    for w in range(1, BLOCK // 64):
        total += _wave_sum(v[64 * w:64 * w + 64])
    return total


def one_workgroup(csr: CompactedCsr, init_abundances, init_noise_count: float, num_samples: int, thin: int, seed: int, problem: int,
                  gamma: float = 1.0) -> Run:
    """gibbsReadCountKernel for the problem at index `problem` of its call."""
    C = csr.columns + 1
    noise_col = C - 1
    T = csr.total_mass
    Z = int(csr.zero_mass)
    margin = Margin()
    a = [float(x) / T for x in init_abundances] + [float(init_noise_count) / T]
    streams = [Stream(seed, [0, 0, t, problem]) for t in range(BLOCK)]
    noise_out = np.zeros(num_samples)
    abund_out = np.zeros((num_samples, noise_col))
    all_counts = []
    recorded = 0
    for it in range(1, num_samples * thin + 1):
        counts = [0] * C
        counts[noise_col] = Z
        a_noise = a[noise_col]
        # (thread t takes rows t, t + 256, ... in that order: ascending rows keep every thread's order)
        for r in range(csr.rows):
            margin.context = (it, "row", r)
            e0, e1 = int(csr.off[r]), int(csr.off[r + 1])
            s = csr.noise[r] * a_noise
            terms = []
            for e in range(e0, e1):
                term = csr.val[e] * a[csr.col[e]]
                s += term
                terms.append((int(csr.col[e]), term))
            counts[noise_col] += _chain_of_binomials(streams[r % BLOCK], int(csr.count[r]), terms, s, counts, margin)
        local = [0.0] * BLOCK
        for j in range(C):
            margin.context = (it, "column", j)
            g, _ = sample_gamma(streams[j % BLOCK], float(counts[j]) + gamma, margin)
            a[j] = g
            local[j % BLOCK] += g
        total = _block_sum(local)
        a = [x / total for x in a]
        all_counts.append(counts)
        if it % thin == 0:
            low = [0.0] * BLOCK
            for j in range(noise_col):
                margin.context = (it, "record", j)
                margin.note(a[j], MIN_GIBBS_ABUNDANCE, "record a < 1e-8")
                if a[j] < MIN_GIBBS_ABUNDANCE:
                    low[j % BLOCK] += a[j] * T
                    abund_out[recorded, j] = 0.0
                else:
                    abund_out[recorded, j] = a[j] * T
            noise_out[recorded] = _block_sum(low) + a[noise_col] * T
            recorded += 1
    return Run(noise_out, abund_out, np.asarray(all_counts, dtype=np.int64), margin, "one workgroup")


def gibbs_row_lanes(rows: int, entries: int) -> int:
    """gibbsRowLanes: a thread per row below a mean of twelve entries, a wavefront per row from there."""
    return 1 if float(entries) < 12.0 * max(1, rows) else 64


def grid(csr: CompactedCsr, init_abundances, init_noise_count: float, num_samples: int, thin: int, seed: int, gamma: float = 1.0) -> Run:
    """runGibbsGridProblems: the state stays unnormalised, the counter is [block, iteration, row or column, domain]."""
    C = csr.columns + 1
    noise_col = C - 1
    T = csr.total_mass
    Z = int(csr.zero_mass)
    margin = Margin()
    lanes = gibbs_row_lanes(csr.rows, csr.entries)
    lds = 16 * C <= GRID_LDS_LIMIT
    g = [float(x) / T for x in init_abundances] + [float(init_noise_count) / T]
    num_partials = (C + BLOCK - 1) // BLOCK
    noise_out = np.zeros(num_samples)
    abund_out = np.zeros((num_samples, noise_col))
    all_counts = []
    recorded = 0
    for it in range(1, num_samples * thin + 1):
        counts = [0] * C
        counts[noise_col] = Z
        g_noise = g[noise_col]
        for r in range(csr.rows):
            margin.context = (it, "row", r)
            e0, e1 = int(csr.off[r]), int(csr.off[r + 1])
            reads = int(csr.count[r])
            terms = [(int(csr.col[e]), csr.val[e] * g[csr.col[e]]) for e in range(e0, e1)]
            if lanes == 1:
                s = csr.noise[r] * g_noise
                for _, term in terms:
                    s += term
                counts[noise_col] += _chain_of_binomials(Stream(seed, [0, it, r, DOMAIN_ROW_CHAIN]), reads, terms, s, counts, margin)
                continue
            if reads == 0:
                continue
            x = [0.0] * 64
            for i, (_, term) in enumerate(terms):
                x[i & 63] += term
            s = _wave_sum(x) + csr.noise[r] * g_noise
            if reads > CATEGORICAL_MAX_READS:
                counts[noise_col] += _chain_of_binomials(Stream(seed, [0, it, r, DOMAIN_ROW_CHAIN]), reads, terms, s, counts, margin)
                continue
            _categorical_draws(seed, it, r, reads, terms, s, counts, margin)
        partials = []
        for b in range(num_partials):
            block = []
            for j in range(b * BLOCK, min(C, (b + 1) * BLOCK)):
                margin.context = (it, "column", j)
                gj, _ = sample_gamma(Stream(seed, [0, it, j, DOMAIN_COLUMN]), float(counts[j]) + gamma, margin)
                g[j] = gj
                block.append(gj)
            partials.append(_block_sum(block))
        all_counts.append(counts)
        if it % thin == 0:
            local = [0.0] * BLOCK
            for b, part in enumerate(partials):
                local[b % BLOCK] += part
            total = _block_sum(local)
            low = 0.0
            for b in range(num_partials):
                block = []
                for j in range(b * BLOCK, min(C, (b + 1) * BLOCK)):
                    aj = g[j] / total
                    if j == noise_col:
                        noise_base = aj * T
                        continue
                    margin.context = (it, "record", j)
                    margin.note(aj, MIN_GIBBS_ABUNDANCE, "record a < 1e-8")
                    if aj < MIN_GIBBS_ABUNDANCE:
                        block.append(aj * T)
                        abund_out[recorded, j] = 0.0
                    else:
                        block.append(0.0)
                        abund_out[recorded, j] = aj * T
                part = _block_sum(block)
                low = part if b == 0 else low + part
            noise_out[recorded] = low + noise_base
            recorded += 1
    route = "grid, %s per row, columns in %s" % ("thread" if lanes == 1 else "wavefront", "LDS" if lds else "global memory")
    return Run(noise_out, abund_out, np.asarray(all_counts, dtype=np.int64), margin, route)


# ---- numpy Philox for the law tests ---------------------------------------------------------------------------------------

def philox4x32_10_many(ctr, key):
    """philox4x32_10 over arrays: ctr [n x 4], key [2] (uint64 arithmetic on 32-bit words)."""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    mask, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [((p1 >> s32) ^ c[1] ^ k0) & mask, p1 & mask, ((p0 >> s32) ^ c[3] ^ k1) & mask, p0 & mask]
        k0 = (k0 + np.uint64(PHILOX_W0)) & mask
        k1 = (k1 + np.uint64(PHILOX_W1)) & mask
    return np.stack(c, axis=1)


def uniforms_many(seed: int, index, per_stream: int, domain: int = 0, iteration: int = 0):
    """The first `per_stream` uniforms of the streams with counter [block, iteration, index, domain] for every index of the array
    `index`: [len(index) x per_stream] (two uniforms per block: words 3, 2 and then 1, 0)."""
    index = np.asarray(index, dtype=np.uint64)
    streams = len(index)
    blocks = (per_stream + 1) // 2
    ctr = np.zeros((streams * blocks, 4), dtype=np.uint64)
    ctr[:, 0] = np.tile(np.arange(blocks, dtype=np.uint64), streams)
    ctr[:, 1] = iteration
    ctr[:, 2] = np.repeat(index, blocks)
    ctr[:, 3] = domain
    out = philox4x32_10_many(ctr, (seed & MASK32, (seed >> 32) & MASK32))
    first = ((out[:, 3] << np.uint64(32)) | out[:, 2]) >> np.uint64(11)
    second = ((out[:, 1] << np.uint64(32)) | out[:, 0]) >> np.uint64(11)
    u = np.stack([first, second], axis=1).astype(np.float64)
    u = (u + 0.5) * TWO_POW_MINUS_53
    return u.reshape(streams, 2 * blocks)[:, :per_stream]


def cospi_many(t):
    t = np.where(t > 1.0, 2.0 - t, t)
    return np.where(t <= 0.25, np.cos(np.pi * t), np.where(t < 0.75, np.sin(np.pi * (0.5 - t)), -np.cos(np.pi * (1.0 - t))))


def normals_many(u1, u2):
    return np.sqrt(-2.0 * np.log(u1)) * cospi_many(2.0 * u2)


def _gamma_rounds(u, shape: float, rounds: int):
    """sample_gamma over the rows of u (a stream's uniforms each): NaN where a stream has not accepted within `rounds` rounds."""
    streams = u.shape[0]
    d = shape - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    out = np.full(streams, np.nan)
    todo = np.ones(streams, dtype=bool)
    at = np.zeros(streams, dtype=np.int64)
    idx = np.arange(streams)
    for _ in range(rounds):
        x = normals_many(u[idx, at], u[idx, at + 1])
        v = 1.0 + c * x
        ok = v > 0.0
        v3 = np.where(ok, v * v * v, 1.0)
        accept = ok & (np.log(u[idx, at + 2]) < 0.5 * x * x + d - d * v3 + d * np.log(v3))
        take = todo & accept
        out[take] = d * v3[take]
        todo &= ~accept
        at = np.where(todo, at + np.where(ok, 3, 2), at)
    return out


def gammas_many(seed: int, shape: float, streams: int, rounds: int = 10):
    """sample_gamma of the streams of the grid's columns 0 .. streams - 1 at iteration 0, at once: every stream runs the
    rejection loop over its own uniforms, two for the normal and, unless v <= 0, one for the test.  Most streams accept in the
    first round (three uniforms, two blocks); the others get the uniforms of `rounds` rounds.  (A stream that has not accepted
    by then is an error: at shape >= 1 a round accepts with probability > 0.95.)"""
    out = _gamma_rounds(uniforms_many(seed, np.arange(streams), 4, DOMAIN_COLUMN), shape, 1)
    late = np.nonzero(np.isnan(out))[0]
    if len(late):
        out[late] = _gamma_rounds(uniforms_many(seed, late, 3 * rounds, DOMAIN_COLUMN), shape, rounds)
    if np.isnan(out).any():
        raise RuntimeError("a gamma stream did not accept within %d rounds" % rounds)
    return out
