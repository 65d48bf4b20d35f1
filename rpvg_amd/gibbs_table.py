"""The read-count Gibbs samples of a batch (-n) as the table of `<prefix>_gibbs.txt.gz`, built on the GPU (include/rpvg_samples.h,
rpvg_amd/csrc/gibbs_table.hip): per path its N sample columns in the order ReadCountGibbsSamplesWriter prints them, the rows it
prints (listed) and the per-sample noise totals of its `Unknown` row.  The table is a copy of the samples and the noise totals are
chains of IEEE additions in cluster order, so a table compares byte for byte with a host loop in that order.

  FlatGibbs      the samples of K clusters in the flat form of rpvg_gibbs_flat, host arrays
  GibbsSamples   the samples of one sampler call where they were drawn (rpvg_hip_gibbs_read_counts_resident)
  GibbsTable     over the C ABI (a hip.Context or an engine.Engine): build / build_flat / build_resident / view / rows / free
  HarnessGibbsTable  over the harness entry points: the table of the samples a run left in a prepared batch, and the file from it
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import hip
from ._flat import FlatArrays, HandleOwner, ctx_handle

u8p, u64p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_double)

ROUTE_RESIDENT, ROUTE_GLOBAL = 0, 1


class CGibbsFlat(C.Structure):
    """rpvg_gibbs_flat"""
    _fields_ = [("num_clusters", C.c_uint32), ("num_blocks", C.c_uint64), ("num_paths", C.c_uint64), ("num_gibbs_samples", C.c_uint32),
                ("num_path_ids", C.c_uint64), ("num_noise_samples", C.c_uint64), ("num_abundance_samples", C.c_uint64),
                ("gibbs_off", C.c_void_p), ("gibbs_path_off", C.c_void_p), ("gibbs_path", C.c_void_p), ("gibbs_noise_off", C.c_void_p),
                ("gibbs_noise", C.c_void_p), ("gibbs_abund_off", C.c_void_p), ("gibbs_abund", C.c_void_p), ("cluster_path_off", C.c_void_p),
                ("total_count", C.c_void_p), ("on_device", C.c_int32)]


class CGibbsTableView(C.Structure):
    """rpvg_gibbs_table_view"""
    _fields_ = [("num_clusters", C.c_uint32), ("num_blocks", C.c_uint64), ("num_paths", C.c_uint64), ("num_gibbs_samples", C.c_uint32),
                ("samples", f64p), ("listed", u8p), ("noise_counts", f64p), ("cluster_path_off", u64p), ("clusters_by_route", C.c_uint32 * 2)]


class CGibbsTableLimits(C.Structure):
    """rpvg_gibbs_table_limits"""
    _fields_ = [("resident_paths", C.c_uint32), ("resident_columns", C.c_uint32), ("sample_tile", C.c_uint32), ("global_paths", C.c_uint32),
                ("resident_lds_bytes", C.c_uint32)]


def limits() -> CGibbsTableLimits:
    """The sizes at which a cluster changes its route: at most resident_paths paths and blocks of at most resident_columns columns
    the resident route, beyond either the global route; the sample tile of a work item.  Needs no GPU."""
    out = CGibbsTableLimits()
    f = hip.lib().rpvg_hip_gibbs_table_limits
    f.restype = None
    f(C.byref(out))
    return out


_GIBBS_FIELDS = (("gibbs_off", np.uint64), ("gibbs_path_off", np.uint64), ("gibbs_path", np.uint32), ("gibbs_noise_off", np.uint64),
           ("gibbs_noise", np.float64), ("gibbs_abund_off", np.uint64), ("gibbs_abund", np.float64), ("cluster_path_off", np.uint64),
           ("total_count", np.float64))


@dataclass
class FlatGibbs(FlatArrays):
    """The Gibbs samples of K clusters in the flat form of rpvg_gibbs_flat, host arrays."""
    gibbs_off: np.ndarray
    gibbs_path_off: np.ndarray
    gibbs_path: np.ndarray
    gibbs_noise_off: np.ndarray
    gibbs_noise: np.ndarray
    gibbs_abund_off: np.ndarray
    gibbs_abund: np.ndarray
    cluster_path_off: np.ndarray
    total_count: np.ndarray
    num_gibbs_samples: int = 0
    _FIELDS, _C_STRUCT = _GIBBS_FIELDS, CGibbsFlat

    @staticmethod
    def from_estimates(batch, estimates: Sequence, num_gibbs_samples: int) -> "FlatGibbs":
        """batch: cluster_path_off (a ClusterBatch); estimates: one ClusterEstimates per cluster, each with total_count and
        gibbs_samples, a list of (path_ids, noise_samples [n], abundance_samples [n x columns])."""
        goff, poff, path, noff, noise, aoff, abund, total = [0], [0], [], [0], [], [0], [], []
        for e in estimates:
            for ids, ns, ab in e.gibbs_samples:
                path.extend(int(p) for p in ids)
                poff.append(len(path))
                noise.extend(float(x) for x in ns)
                noff.append(len(noise))
                abund.extend(float(x) for x in np.asarray(ab, dtype=np.float64).reshape(-1))
                aoff.append(len(abund))
            goff.append(len(poff) - 1)
            total.append(float(e.total_count))
        return FlatGibbs(goff, poff, path, noff, noise, aoff, abund, batch.cluster_path_off, total, num_gibbs_samples)

    def sizes(self) -> dict:
        return dict(num_clusters=len(self.total_count), num_blocks=max(len(self.gibbs_path_off) - 1, 0), num_paths=int(self.cluster_path_off[-1])
                    if len(self.cluster_path_off) else 0, num_gibbs_samples=int(self.num_gibbs_samples), num_path_ids=len(self.gibbs_path),
                    num_noise_samples=len(self.gibbs_noise), num_abundance_samples=len(self.gibbs_abund))


class GibbsSamples(HandleOwner):
    """The samples of one call of the read-count Gibbs sampler, left on the GPU (rpvg_hip_gibbs_samples)."""

    def __init__(self, ctx_handle, handle, problems, keep):
        self.ctx_handle, self.handle, self.problems, self._keep = ctx_handle, handle, problems, keep

    @classmethod
    def draw(cls, ctx: "hip.Context", batch, clusters, columns, init_abundances, init_noise_count, num_samples, seeds, thin: int,
             gamma: float = 1.0) -> "GibbsSamples":
        """The arguments of Context.gibbs_read_counts; the samples stay where they were drawn."""
        P = len(clusters)
        cl = np.ascontiguousarray(clusters, dtype=np.uint32)
        col_off = np.zeros(P + 1, dtype=np.uint64)
        col_off[1:] = np.cumsum([len(c) for c in columns])
        col_path = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint32) for c in columns]) if P else np.zeros(0), dtype=np.uint32)
        init = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64) for a in init_abundances]) if P else np.zeros(0), dtype=np.float64)
        init_noise = np.ascontiguousarray(init_noise_count, dtype=np.float64)
        n = np.ascontiguousarray(num_samples, dtype=np.uint32)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert init.size == int(col_off[-1]) and init_noise.size == n.size == sd.size == P
        problems = hip.CEmProblems(P, cl.ctypes.data, col_off.ctypes.data, col_path.ctypes.data, 0.0)
        handle = C.c_void_p()
        hip._check(hip.lib().rpvg_hip_gibbs_read_counts_resident(ctx.handle, batch.handle, C.byref(problems), C.c_void_p(init.ctypes.data),
                                                                 C.c_void_p(init_noise.ctypes.data), C.c_void_p(n.ctypes.data),
                                                                 C.c_void_p(sd.ctypes.data), C.c_uint32(thin), C.c_double(gamma), C.byref(handle)),
                   "rpvg_hip_gibbs_read_counts_resident")
        self = cls(ctx.handle, handle, problems, (cl, col_off, col_path))
        self.num_samples, self.widths = n.astype(np.int64), np.diff(col_off.astype(np.int64))
        return self

    def get(self):
        """(noise samples, abundance samples) in the layout of rpvg_hip_gibbs_read_counts (rpvg_hip_gibbs_samples_get)."""
        noise = np.zeros(int(self.num_samples.sum()), dtype=np.float64)
        abund = np.zeros(int((self.num_samples * self.widths).sum()), dtype=np.float64)
        hip._check(hip.lib().rpvg_hip_gibbs_samples_get(self.ctx_handle, self.handle, C.c_void_p(noise.ctypes.data if noise.size else None),
                                                        C.c_void_p(abund.ctypes.data if abund.size else None)), "rpvg_hip_gibbs_samples_get")
        return noise, abund

    def _release(self):
        hip.lib().rpvg_hip_gibbs_samples_free(self.ctx_handle, self.handle)


class GibbsTable(HandleOwner):
    """A table resident on the GPU (rpvg_hip_gibbs_table)."""

    def __init__(self, ctx_handle, handle):
        self.ctx_handle, self.handle = ctx_handle, handle

    @classmethod
    def build(cls, ctx_or_engine, flat: FlatGibbs) -> "GibbsTable":
        return cls.build_flat(ctx_or_engine, flat.as_c())

    @classmethod
    def build_flat(cls, ctx_or_engine, flat: CGibbsFlat) -> "GibbsTable":
        """flat: host pointers (on_device = 0) or device pointers of the context's GPU (on_device = 1)."""
        ctx = ctx_handle(ctx_or_engine)
        handle = C.c_void_p()
        hip._check(hip.lib().rpvg_hip_gibbs_table_build(ctx, C.byref(flat), C.byref(handle)), "rpvg_hip_gibbs_table_build")
        return cls(ctx, handle)

    @classmethod
    def build_resident(cls, ctx_or_engine, samples: GibbsSamples, cluster_path_off, total_count, num_gibbs_samples: int,
                       problems: Optional[hip.CEmProblems] = None) -> "GibbsTable":
        """The table of a sampler call's samples: its problems are the blocks (rpvg_hip_gibbs_table_build_resident)."""
        ctx = ctx_handle(ctx_or_engine)
        cpo = np.ascontiguousarray(cluster_path_off, dtype=np.uint64)
        total = np.ascontiguousarray(total_count, dtype=np.float64)
        assert len(cpo) == len(total) + 1
        handle = C.c_void_p()
        hip._check(hip.lib().rpvg_hip_gibbs_table_build_resident(ctx, samples.handle, C.byref(problems if problems is not None else samples.problems),
                                                                 C.c_uint32(len(total)), C.c_void_p(cpo.ctypes.data), C.c_void_p(total.ctypes.data if len(total) else None),
                                                                 C.c_uint32(num_gibbs_samples), C.byref(handle)), "rpvg_hip_gibbs_table_build_resident")
        return cls(ctx, handle)

    def view(self) -> dict:
        """Host copies by name: samples [P, N], listed [P], noise_counts [N], cluster_path_off [K + 1] and clusters_by_route."""
        v = CGibbsTableView()
        hip._check(hip.lib().rpvg_hip_gibbs_table_view(self.ctx_handle, self.handle, C.byref(v)), "rpvg_hip_gibbs_table_view")
        return _decode(v)

    def rows(self, first_path: int, num_paths: int, num_gibbs_samples: int) -> np.ndarray:
        """The sample rows of paths [first_path, first_path + num_paths) (rpvg_hip_gibbs_table_rows)."""
        out = np.zeros((num_paths, num_gibbs_samples), dtype=np.float64)
        hip._check(hip.lib().rpvg_hip_gibbs_table_rows(self.ctx_handle, self.handle, C.c_uint64(first_path), C.c_uint64(num_paths),
                                                       C.c_void_p(out.ctypes.data if out.size else None)), "rpvg_hip_gibbs_table_rows")
        return out

    def _release(self):
        hip.lib().rpvg_hip_gibbs_table_free(self.ctx_handle, self.handle)


# ---- the harness: the table of a prepared batch's Gibbs samples and the file from it ---------------------------------------------

def _harness():
    from . import engine
    L = engine.lib()
    L.rpvg_amd_gibbs_table_build.restype = C.c_void_p
    L.rpvg_amd_gibbs_table_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_double)]
    L.rpvg_amd_gibbs_table_view.argtypes = [C.c_void_p, C.POINTER(CGibbsTableView)]
    L.rpvg_amd_gibbs_table_write.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32]
    L.rpvg_amd_gibbs_table_free.argtypes = [C.c_void_p]
    L.rpvg_amd_gibbs_from_containers.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    return L, engine


def _decode(v: CGibbsTableView) -> dict:
    P, N, K = int(v.num_paths), int(v.num_gibbs_samples), int(v.num_clusters)
    samples = np.ctypeslib.as_array(v.samples, shape=(P * N,)).copy().reshape(P, N) if P * N else np.zeros((P, N), dtype=np.float64)
    listed = np.ctypeslib.as_array(v.listed, shape=(P,)).copy() if P else np.zeros(0, dtype=np.uint8)
    return dict(samples=samples, listed=listed, noise_counts=np.ctypeslib.as_array(v.noise_counts, shape=(N,)).copy(),
                cluster_path_off=np.ctypeslib.as_array(v.cluster_path_off, shape=(K + 1,)).copy(), num_clusters=K, num_blocks=int(v.num_blocks),
                clusters_by_route=[int(x) for x in v.clusters_by_route])


class HarnessGibbsTable(HandleOwner):
    """The table of the Gibbs samples the last run (-n > 0) left in a PreparedBatch, through the host class
    (rpvg_amd/host/gibbs_samples_table.hpp) and the writer's addTable()."""

    def __init__(self, engine, prepared, num_gibbs_samples: int):
        L, eng = _harness()
        secs = C.c_double(0)
        self.num_gibbs_samples = num_gibbs_samples
        self.handle = L.rpvg_amd_gibbs_table_build(engine.handle, prepared.handle, num_gibbs_samples, C.byref(secs))
        if not self.handle:
            raise hip.EngineError(f"gibbs table failed: {eng._err()}")
        self.build_seconds = secs.value

    def view(self) -> dict:
        L, eng = _harness()
        v = CGibbsTableView()
        if L.rpvg_amd_gibbs_table_view(self.handle, C.byref(v)) != 0:
            raise hip.EngineError(f"gibbs table view failed: {eng._err()}")
        return _decode(v)

    def write(self, prefix: str, unaligned_read_count: int = 0):
        """<prefix>.txt.gz from the table."""
        L, eng = _harness()
        if L.rpvg_amd_gibbs_table_write(self.handle, self.num_gibbs_samples, prefix.encode(), unaligned_read_count) != 0:
            raise hip.EngineError(f"gibbs table write failed: {eng._err()}")

    def _release(self):
        _harness()[0].rpvg_amd_gibbs_table_free(self.handle)


def from_containers(prepared, num_gibbs_samples: int, num_paths: int, prefix: str = "", unaligned_read_count: int = 0, table: bool = True):
    """The same from the containers of the prepared batch on one host thread: the file by the writer's addSamples() (prefix), and
    the writer's loops with stores into a dense table (table): dict(samples, listed, noise_counts, seconds) or None."""
    L, eng = _harness()
    samples = np.zeros((num_paths, num_gibbs_samples), dtype=np.float64) if table else None
    listed = np.zeros(num_paths, dtype=np.uint8) if table else None
    noise = np.zeros(num_gibbs_samples, dtype=np.float64) if table else None
    secs = C.c_double(0)
    if L.rpvg_amd_gibbs_from_containers(prepared.handle, num_gibbs_samples, prefix.encode(), unaligned_read_count,
                                        samples.ctypes.data if table and samples.size else None, listed.ctypes.data if table and listed.size else None,
                                        noise.ctypes.data if table else None, C.byref(secs)) != 0:
        raise hip.EngineError(f"gibbs from_containers failed: {eng._err()}")
    return dict(samples=samples, listed=listed, noise_counts=noise, seconds=secs.value) if table else None
