"""The estimates of a batch as the table rpvg writes, built on the GPU (include/rpvg_table.h, rpvg_amd/csrc/estimates_table.hip):
per path HaplotypeProbability, ReadCount, transcript count and TPM, per set member its transcript count and TPM, per cluster
its part of the TPM denominator, and the noise totals of the `Unknown` rows.  Every sum is a chain of IEEE additions in the
order rpvg_table.h states, so a table compares bit for bit with a host loop in that order.

  EstimatesTable   over the C ABI (a hip.Context or an engine.Engine), from a batch and decoded estimates or from flat arrays
  HarnessTable     over the harness entry points: the table of a prepared batch's estimates and the three result files from it
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Sequence

import numpy as np

from . import hip
from ._flat import FlatArrays, HandleOwner, ctx_handle

u32p, u64p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)

ROUTE_WAVE, ROUTE_LDS, ROUTE_GLOBAL = 0, 1, 2


class CEstimatesFlat(C.Structure):
    """rpvg_estimates_flat"""
    _fields_ = [("num_clusters", C.c_uint32), ("num_sets", C.c_uint64), ("num_members", C.c_uint64), ("num_abundances", C.c_uint64),
                ("num_paths", C.c_uint64), ("set_off", C.c_void_p), ("member_off", C.c_void_p), ("members", C.c_void_p),
                ("posteriors", C.c_void_p), ("abund_off", C.c_void_p), ("abundances", C.c_void_p), ("noise_count", C.c_void_p),
                ("cluster_path_off", C.c_void_p), ("path_effective_length", C.c_void_p), ("on_device", C.c_int32)]


class CEstimatesTableView(C.Structure):
    """rpvg_estimates_table_view"""
    _fields_ = [("num_clusters", C.c_uint32), ("num_paths", C.c_uint64), ("num_members", C.c_uint64), ("haplotype_prob", f64p),
                ("read_count", f64p), ("transcript_count", f64p), ("tpm", f64p), ("member_transcript_count", f64p), ("member_tpm", f64p),
                ("cluster_transcript_count", f64p), ("total_transcript_count", C.c_double), ("noise_count_total", C.c_double),
                ("noise_count_share_total", C.c_double), ("tpm_denominator", C.c_double), ("has_tpm", C.c_int32), ("ploidy", C.c_uint32),
                ("clusters_by_route", C.c_uint32 * 3)]


class CEstimatesTableLimits(C.Structure):
    """rpvg_estimates_table_limits"""
    _fields_ = [("wave_paths", C.c_uint32), ("wave_members", C.c_uint32), ("lds_paths", C.c_uint32), ("lds_members", C.c_uint32),
                ("wave_lds_bytes", C.c_uint32), ("lds_bytes", C.c_uint32)]


def limits() -> CEstimatesTableLimits:
    """The sizes at which a cluster changes its route: at most (wave_paths, wave_members) one wavefront, at most (lds_paths,
    lds_members) one workgroup, beyond either the global route."""
    out = CEstimatesTableLimits()
    hip.lib().rpvg_hip_estimates_table_limits(C.byref(out))
    return out


_ESTIMATES_FIELDS = (("set_off", np.uint64), ("member_off", np.uint64), ("members", np.uint32), ("posteriors", np.float64), ("abund_off", np.uint64),
           ("abundances", np.float64), ("noise_count", np.float64), ("cluster_path_off", np.uint64), ("path_effective_length", np.float64))


@dataclass
class FlatEstimates(FlatArrays):
    """The estimates of K clusters in the flat form of rpvg_estimates_flat, host arrays."""
    set_off: np.ndarray
    member_off: np.ndarray
    members: np.ndarray
    posteriors: np.ndarray
    abund_off: np.ndarray
    abundances: np.ndarray
    noise_count: np.ndarray
    cluster_path_off: np.ndarray
    path_effective_length: np.ndarray
    _FIELDS, _C_STRUCT = _ESTIMATES_FIELDS, CEstimatesFlat

    @staticmethod
    def from_estimates(batch, estimates: Sequence) -> "FlatEstimates":
        """batch: cluster_path_off and path_effective_length (a ClusterBatch); estimates: one ClusterEstimates per cluster."""
        set_off, member_off, members, posteriors, abund_off, abundances, noise = [0], [0], [], [], [0], [], []
        for e in estimates:
            for s, post in zip(e.path_group_sets, e.posteriors):
                members.extend(int(p) for p in s)
                member_off.append(len(members))
                posteriors.append(float(post))
            set_off.append(len(posteriors))
            abundances.extend(float(a) for a in e.abundances)
            abund_off.append(len(abundances))
            noise.append(float(e.noise_count))
        return FlatEstimates(set_off, member_off, members, posteriors, abund_off, abundances, noise, batch.cluster_path_off,
                             batch.path_effective_length)

    @property
    def num_clusters(self) -> int:
        return len(self.noise_count)

    def sizes(self) -> dict:
        return dict(num_clusters=len(self.noise_count), num_sets=len(self.posteriors), num_members=len(self.members),
                    num_abundances=len(self.abundances), num_paths=len(self.path_effective_length))


def _arr(ptr, n):
    return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dtype=np.float64)


def _decode(v: CEstimatesTableView) -> dict:
    P, M, K = int(v.num_paths), int(v.num_members), int(v.num_clusters)
    return dict(haplotype_prob=_arr(v.haplotype_prob, P), read_count=_arr(v.read_count, P), transcript_count=_arr(v.transcript_count, P),
                tpm=_arr(v.tpm, P), member_transcript_count=_arr(v.member_transcript_count, M), member_tpm=_arr(v.member_tpm, M),
                cluster_transcript_count=_arr(v.cluster_transcript_count, K), total_transcript_count=float(v.total_transcript_count),
                noise_count_total=float(v.noise_count_total), noise_count_share_total=float(v.noise_count_share_total),
                tpm_denominator=float(v.tpm_denominator), has_tpm=bool(v.has_tpm), ploidy=int(v.ploidy),
                clusters_by_route=[int(x) for x in v.clusters_by_route])


class EstimatesTable(HandleOwner):
    """A table resident on the GPU (rpvg_hip_estimates_table)."""

    def __init__(self, ctx_handle, handle):
        self.ctx_handle, self.handle = ctx_handle, handle

    @classmethod
    def build(cls, ctx_or_engine, batch, estimates, ploidy: int) -> "EstimatesTable":
        """batch: a ClusterBatch (its cluster_path_off and path_effective_length are read); estimates: what Engine.run returned
        for it, or a FlatEstimates (batch may then be None)."""
        flat = estimates if isinstance(estimates, FlatEstimates) else FlatEstimates.from_estimates(batch, estimates)
        return cls.build_flat(ctx_or_engine, flat.as_c(), ploidy)

    @classmethod
    def build_flat(cls, ctx_or_engine, flat: CEstimatesFlat, ploidy: int) -> "EstimatesTable":
        """flat: host pointers (on_device = 0) or device pointers of the context's GPU (on_device = 1)."""
        ctx = ctx_handle(ctx_or_engine)
        handle = C.c_void_p()
        hip._check(hip.lib().rpvg_hip_estimates_table_build(ctx, C.byref(flat), C.c_uint32(ploidy), C.byref(handle)),
                   "rpvg_hip_estimates_table_build")
        return cls(ctx, handle)

    def tpm(self, denominator: float):
        """transcript count / denominator * 1e6 for every path and member: the table's own total_transcript_count when the batch
        is the run, the sum over batches and ranks otherwise."""
        hip._check(hip.lib().rpvg_hip_estimates_table_tpm(self.ctx_handle, self.handle, C.c_double(denominator)), "rpvg_hip_estimates_table_tpm")

    def view(self) -> dict:
        """Host copies by name: the arrays of rpvg_estimates_table_view, its scalars and clusters_by_route."""
        v = CEstimatesTableView()
        hip._check(hip.lib().rpvg_hip_estimates_table_view(self.ctx_handle, self.handle, C.byref(v)), "rpvg_hip_estimates_table_view")
        return _decode(v)

    def _release(self):
        hip.lib().rpvg_hip_estimates_table_free(self.ctx_handle, self.handle)


# ---- the harness: the table of a prepared batch's estimates and the result files from it -----------------------------------------

WRITERS = ("abundance", "haplotype", "joint")  # <prefix>.txt, <prefix>.txt, <prefix>_joint.txt
POSTERIOR_WRITER = "posterior"                 # <prefix>.txt of a `haplotypes` result: no TPMs, no `Unknown` row, no transcript count


def _harness():
    from . import engine
    L = engine.lib()
    L.rpvg_amd_estimates_table_build.restype = C.c_void_p
    L.rpvg_amd_estimates_table_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.rpvg_amd_estimates_table_tpm.argtypes = [C.c_void_p, C.c_double]
    L.rpvg_amd_estimates_table_view.argtypes = [C.c_void_p, C.POINTER(CEstimatesTableView)]
    L.rpvg_amd_estimates_table_write.argtypes = [C.c_void_p, C.c_char_p, C.c_double, C.c_char_p, C.c_uint32]
    L.rpvg_amd_estimates_table_free.argtypes = [C.c_void_p]
    L.rpvg_amd_estimates_write_from_containers.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_double, C.c_double, C.c_char_p, C.c_uint32,
                                                           C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    return L, engine


class HarnessTable(HandleOwner):
    """The table of the estimates the last run left in a PreparedBatch (or of a result handle), through the host classes
    (rpvg_amd/host/estimates_table.hpp) and the writers' addTable()."""

    def __init__(self, engine, prepared, ploidy: int, result_handle=None):
        L, eng = _harness()
        self.handle = L.rpvg_amd_estimates_table_build(engine.handle, result_handle, prepared.handle, ploidy)
        if not self.handle:
            raise hip.EngineError(f"estimates table failed: {eng._err()}")

    @classmethod
    def from_handle(cls, handle) -> "HarnessTable":
        """A table handle another harness entry point made (rpvg_amd_estimates_table_build_resident)."""
        self = cls.__new__(cls)
        self.handle = handle
        return self

    def tpm(self, denominator: float):
        L, eng = _harness()
        if L.rpvg_amd_estimates_table_tpm(self.handle, denominator) != 0:
            raise hip.EngineError(f"estimates table tpm failed: {eng._err()}")

    def view(self) -> dict:
        L, eng = _harness()
        v = CEstimatesTableView()
        if L.rpvg_amd_estimates_table_view(self.handle, C.byref(v)) != 0:
            raise hip.EngineError(f"estimates table view failed: {eng._err()}")
        return _decode(v)

    def write(self, writer: str, prefix: str, min_posterior: float = 1e-8, unaligned_read_count: int = 0):
        """One of WRITERS from the table (after tpm())."""
        L, eng = _harness()
        if L.rpvg_amd_estimates_table_write(self.handle, writer.encode(), min_posterior, prefix.encode(), unaligned_read_count) != 0:
            raise hip.EngineError(f"estimates table write({writer}) failed: {eng._err()}")

    def _release(self):
        _harness()[0].rpvg_amd_estimates_table_free(self.handle)


def write_from_containers(prepared, writer: str, ploidy: int, prefix: str, denominator: float = 0.0, min_posterior: float = 1e-8,
                          unaligned_read_count: int = 0):
    """The same file by the writer's addEstimates() from the containers of the prepared batch (writer "": no file).  Returns
    (totalTranscriptCount of the containers, the seconds that sum took, the seconds of the writer from its constructor to
    close()); a denominator of 0 stands for that sum."""
    L, eng = _harness()
    total, secs, write_secs = C.c_double(0), C.c_double(0), C.c_double(0)
    if L.rpvg_amd_estimates_write_from_containers(prepared.handle, writer.encode(), ploidy, min_posterior, denominator, prefix.encode(),
                                                  unaligned_read_count, C.byref(total), C.byref(secs), C.byref(write_secs)) != 0:
        raise hip.EngineError(f"write_from_containers({writer}) failed: {eng._err()}")
    return total.value, secs.value, write_secs.value
