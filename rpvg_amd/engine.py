"""ctypes binding of the harness entry points (librpvg_amd_harness.so) over the host-side estimator classes
(librpvg_amd_host.so).

The work happens in C++ (``rpvg_amd/host``: PathEstimator classes over the C
ABI of the HIP engine); this module only marshals flat batches in and
estimates out for tests and bench.  No fallback: a missing library or GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from . import hip
from .batch import CClusterBatch, CEstimatesView, CParams, ClusterBatch, ClusterEstimates, decode_view

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "host", "librpvg_amd_harness.so")  # links librpvg_amd_host.so, the product

MODELS = ("transcripts", "strains", "haplotype-transcripts", "haplotypes")

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise hip.EngineError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() (there is no CPU fallback)")
        hip.lib()  # librpvg_hip.so first (also resolved through the rpath)
        L = C.CDLL(LIB_PATH)
        L.rpvg_amd_last_error.restype = C.c_char_p
        L.rpvg_amd_engine_create.restype = C.c_void_p
        L.rpvg_amd_engine_create.argtypes = [C.c_int]
        L.rpvg_amd_engine_create_uploader.restype = C.c_void_p
        L.rpvg_amd_engine_create_uploader.argtypes = [C.c_int]
        L.rpvg_amd_engine_destroy.argtypes = [C.c_void_p]
        L.rpvg_amd_engine_ctx.restype = C.c_void_p
        L.rpvg_amd_engine_ctx.argtypes = [C.c_void_p]
        L.rpvg_amd_engine_stats_get.argtypes = [C.c_void_p, C.c_void_p]
        L.rpvg_amd_engine_stats_reset.argtypes = [C.c_void_p]
        L.rpvg_amd_engine_independent_stats_get.argtypes = [C.c_void_p, C.c_void_p]
        L.rpvg_amd_run_generators_after.restype = C.c_int
        L.rpvg_amd_run_generators_after.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(CParams), C.POINTER(C.c_uint32)]
        L.rpvg_amd_host_threads.restype = C.c_int
        L.rpvg_amd_batch_prepare.restype = C.c_void_p
        L.rpvg_amd_batch_prepare.argtypes = [C.c_void_p, C.POINTER(CClusterBatch), C.c_int]
        L.rpvg_amd_batch_free.argtypes = [C.c_void_p]
        L.rpvg_amd_batch_reupload.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CClusterBatch), C.POINTER(C.c_double)]
        L.rpvg_amd_batch_prepare_from_alignments.restype = C.c_void_p
        L.rpvg_amd_batch_prepare_from_alignments.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CClusterBatch), C.c_double, C.c_double,
                                                             C.c_double, C.c_uint32, C.c_int, C.c_double, C.c_double,
                                                             C.POINTER(C.c_double)]
        L.rpvg_amd_batch_prepare_from_alignments_fit.restype = C.c_void_p
        L.rpvg_amd_batch_prepare_from_alignments_fit.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CClusterBatch), C.c_void_p, C.c_uint32, C.c_int,
                                                                 C.c_void_p, C.c_double, C.c_double, C.POINTER(hip.CFragLengthFit),
                                                                 C.c_void_p, C.POINTER(C.c_double)]
        L.rpvg_amd_batch_prepare_from_alignments_fitted.restype = C.c_void_p
        L.rpvg_amd_batch_prepare_from_alignments_fitted.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CClusterBatch), C.c_double, C.c_double,
                                                                    C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]
        L.rpvg_amd_batch_prepare_from_fragments.restype = C.c_void_p
        L.rpvg_amd_batch_prepare_from_fragments.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                            C.POINTER(CClusterBatch), C.c_double, C.c_double, C.c_double, C.c_uint32,
                                                            C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.POINTER(C.c_double)]
        L.rpvg_amd_batch_prepare_from_fragments_table.restype = C.c_void_p
        L.rpvg_amd_batch_prepare_from_fragments_table.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                                  C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_uint32,
                                                                  C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                  C.POINTER(C.c_double)]
        L.rpvg_amd_batch_has_source_columns.restype = C.c_int
        L.rpvg_amd_batch_has_source_columns.argtypes = [C.c_void_p]
        L.rpvg_amd_batch_prepare_synth_dense.restype = C.c_void_p
        L.rpvg_amd_batch_prepare_synth_dense.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32]
        L.rpvg_amd_run.restype = C.c_void_p
        L.rpvg_amd_run.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(CParams), C.POINTER(C.c_double)]
        L.rpvg_amd_run_team.restype = C.c_int
        L.rpvg_amd_run_team.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(CParams), C.c_int, C.POINTER(C.c_double)]
        L.rpvg_amd_run_team_result.restype = C.c_void_p
        L.rpvg_amd_run_team_result.argtypes = [C.c_void_p]
        L.rpvg_amd_run_inplace.restype = C.c_int
        L.rpvg_amd_run_inplace.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(CParams), C.POINTER(C.c_double)]
        L.rpvg_amd_run_from_alignments_inplace.restype = C.c_int
        L.rpvg_amd_run_from_alignments_inplace.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(CParams), C.POINTER(C.c_double),
                                                           C.POINTER(C.c_double)]
        L.rpvg_amd_group_create.restype = C.c_void_p
        L.rpvg_amd_group_create.argtypes = [C.POINTER(C.c_int), C.c_int]
        L.rpvg_amd_group_destroy.argtypes = [C.c_void_p]
        L.rpvg_amd_group_has_communicator.argtypes = [C.c_void_p]
        L.rpvg_amd_group_run.restype = C.c_void_p
        L.rpvg_amd_group_run.argtypes = [C.c_void_p, C.POINTER(CClusterBatch), C.c_char_p, C.POINTER(CParams), C.POINTER(C.c_double)]
        L.rpvg_amd_group_partition.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.rpvg_amd_group_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.rpvg_amd_pipeline_create.restype = C.c_void_p
        L.rpvg_amd_pipeline_create.argtypes = [C.c_int, C.c_char_p, C.POINTER(CParams), C.c_int]
        L.rpvg_amd_pipeline_destroy.argtypes = [C.c_void_p]
        L.rpvg_amd_pipeline_workers.argtypes = [C.c_void_p]
        L.rpvg_amd_pipeline_prepare_slots.argtypes = [C.c_void_p, C.POINTER(CClusterBatch), C.c_int]
        L.rpvg_amd_pipeline_submit.argtypes = [C.c_void_p, C.POINTER(CClusterBatch), C.c_int]
        L.rpvg_amd_pipeline_prepare_slot.argtypes = [C.c_void_p, C.POINTER(CClusterBatch), C.c_int]
        L.rpvg_amd_pipeline_wait.argtypes = [C.c_void_p]
        L.rpvg_amd_pipeline_result.restype = C.c_void_p
        L.rpvg_amd_pipeline_result.argtypes = [C.c_void_p, C.c_int]
        L.rpvg_amd_pipeline_stats_get.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.rpvg_amd_pipeline_stats_reset.argtypes = [C.c_void_p]
        L.rpvg_amd_pipeline_completions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.rpvg_amd_result_view.argtypes = [C.c_void_p, C.POINTER(CEstimatesView)]
        L.rpvg_amd_result_free.argtypes = [C.c_void_p]
        _lib = L
    return _lib


class FragLengthFit(NamedTuple):
    """What Engine.fit_frag_length returns: the FragmentLengthDist fitted to counts of fragment lengths.  Unlike the
    parametric (loc, scale, shape, sd_max_multi) it carries its maximum length; handed to prepare_from_alignments as
    `frag`, its density table is computed on the GPU."""
    loc: float
    scale: float
    shape: float
    max_length: int
    valid: bool
    stats: dict  # sample_size, iterations (outer passes), evaluations (log-likelihood sums)


def _fit_tuple(fit) -> FragLengthFit:
    return FragLengthFit(fit.loc, fit.scale, fit.shape, fit.max_length, bool(fit.valid),
                         dict(sample_size=fit.sample_size, iterations=fit.iterations, evaluations=fit.evaluations))


def _err() -> str:
    return lib().rpvg_amd_last_error().decode()


class Engine:
    """One GPU (HipEngine) shared by the estimators created on it."""

    def __init__(self, device: int = 0, uploader: bool = False):
        """uploader: an engine that only uploads batches (PreparedBatch.reupload) next to the one that estimates."""
        self.handle = lib().rpvg_amd_engine_create_uploader(device) if uploader else lib().rpvg_amd_engine_create(device)
        if not self.handle:
            raise hip.EngineError(f"engine create failed: {_err()}")

    def close(self):
        if self.handle:
            lib().rpvg_amd_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ctx(self):
        return C.c_void_p(lib().rpvg_amd_engine_ctx(self.handle))

    def stats(self) -> dict:
        s = hip.CKernelStats()
        if lib().rpvg_amd_engine_stats_get(self.handle, C.byref(s)) != 0:
            raise hip.EngineError(f"stats failed: {_err()}")
        return s.as_dict()

    def independent_stats(self) -> dict:
        """Calls of rpvg_hip_nested_independent_subset_em that completed, their draws and subsets, summed over the host lanes."""
        s = hip.CIndependentStats()
        if lib().rpvg_amd_engine_independent_stats_get(self.handle, C.byref(s)) != 0:
            raise hip.EngineError(f"stats failed: {_err()}")
        return {n: int(getattr(s, n)) for n, _ in s._fields_}

    def reset_stats(self):
        if lib().rpvg_amd_engine_stats_reset(self.handle) != 0:
            raise hip.EngineError(f"stats reset failed: {_err()}")

    def info(self) -> Tuple[str, int, int]:
        name = C.create_string_buffer(256)
        cus, mem = C.c_uint32(0), C.c_uint64(0)
        hip._check(hip.lib().rpvg_hip_device_info(self._ctx(), name, 256, C.byref(cus), C.byref(mem)), "rpvg_hip_device_info")
        return name.value.decode(), cus.value, mem.value

    def prepare(self, batch: ClusterBatch, per_cluster: bool = False) -> "PreparedBatch":
        return PreparedBatch(self, batch, per_cluster)

    def fit_frag_length(self, counts, skew_normal: bool = True) -> FragLengthFit:
        """FragmentLengthDist(frag_length_counts, skew_normal) fitted on the GPU: counts[v] = read pairs of fragment length v.
        Returns (loc, scale, shape, max_length, valid, stats); stats = {"sample_size", "iterations", "evaluations"}."""
        return _fit_tuple(hip.frag_length_fit(self._ctx(), counts, skew_normal))

    def effective_lengths(self, path_lengths, frag) -> np.ndarray:
        """PathsIndex::effectivePathLength of every path length on the GPU; frag = (loc, scale, shape, ...)."""
        return hip.effective_lengths(self._ctx(), path_lengths, float(frag[0]), float(frag[1]), float(frag[2]))

    def prepare_from_alignments(self, alignments, path_info: ClusterBatch, frag=None, is_single_end: bool = False,
                                min_noise_prob: float = 1e-4, prob_precision: float = 1e-8, frag_counts=None, path_lengths=None,
                                skew_normal: bool = True) -> "PreparedBatch":
        """Batch whose rows are constructed on the GPU from alignment-path lists (rpvg_amd/host/read_rows.hpp):
        alignments = rows.AlignmentBatch, path_info = a ClusterBatch whose path arrays describe the clusters' paths,
        frag = (loc, scale, shape, sd_max_multi) of the FragmentLengthDist (default (300, 50, 0, 10)), or a FragLengthFit
        (from fit_frag_length: the table of its log densities is then computed on the GPU and never leaves it).
        frag_counts + path_lengths instead of frag: the distribution is fitted to the counts of the observed fragment
        lengths and the effective lengths are derived from the path lengths, both on the GPU (paired-end only); the
        result carries .frag_fit (as fit_frag_length returns it) and .path_effective_length."""
        if frag is not None and frag_counts is not None:
            raise ValueError("prepare_from_alignments: frag and frag_counts exclude each other")
        if (frag_counts is None) != (path_lengths is None):
            raise ValueError("prepare_from_alignments: frag_counts and path_lengths come together")
        if frag_counts is not None and is_single_end:
            raise ValueError("prepare_from_alignments: a single-end run has no fragment lengths to fit")
        prep = PreparedBatch.__new__(PreparedBatch)
        prep.engine = self
        prep.batch = path_info
        ca, cb = alignments.as_c(), path_info.as_c()
        secs = C.c_double(0)
        if frag_counts is not None:
            counts = np.ascontiguousarray(frag_counts, dtype=np.uint32)
            lengths = np.ascontiguousarray(path_lengths, dtype=np.uint32)
            if lengths.size != len(alignments.path_effective_length):
                raise ValueError("prepare_from_alignments: one path length per path")
            fit = hip.CFragLengthFit()
            eff = np.zeros(lengths.size, dtype=np.float64)
            prep.handle = lib().rpvg_amd_batch_prepare_from_alignments_fit(
                self.handle, C.byref(ca), C.byref(cb), C.c_void_p(counts.ctypes.data if counts.size else None), counts.size,
                1 if skew_normal else 0, C.c_void_p(lengths.ctypes.data if lengths.size else None), min_noise_prob, prob_precision,
                C.byref(fit), C.c_void_p(eff.ctypes.data if eff.size else None), C.byref(secs))
            if not prep.handle:
                raise hip.EngineError(f"batch prepare from alignments failed: {_err()}")
            prep.frag_fit = _fit_tuple(fit)
            prep.path_effective_length = eff
            prep.row_construction_seconds = secs.value
            return prep
        if isinstance(frag, FragLengthFit):
            if is_single_end or not frag.valid:
                raise ValueError("prepare_from_alignments: a fitted distribution must be valid and belongs to a paired-end run")
            prep.handle = lib().rpvg_amd_batch_prepare_from_alignments_fitted(
                self.handle, C.byref(ca), C.byref(cb), frag.loc, frag.scale, frag.shape, min_noise_prob, prob_precision, C.byref(secs))
            if not prep.handle:
                raise hip.EngineError(f"batch prepare from alignments failed: {_err()}")
            prep.row_construction_seconds = secs.value
            return prep
        if frag is None:
            frag = (300.0, 50.0, 0.0, 10)
        prep.handle = lib().rpvg_amd_batch_prepare_from_alignments(
            self.handle, C.byref(ca), C.byref(cb), frag[0], frag[1], frag[2], int(frag[3]), 1 if is_single_end else 0,
            min_noise_prob, prob_precision, C.byref(secs))
        if not prep.handle:
            raise hip.EngineError(f"batch prepare from alignments failed: {_err()}")
        prep.row_construction_seconds = secs.value
        return prep

    def prepare_from_fragments(self, chunks, index_params, path_info: Optional[ClusterBatch] = None, extra_sets=None, frag=None,
                               min_noise_prob: float = 1e-4, prob_precision: float = 1e-8, path_table=None,
                               collapse_names: bool = False) -> "PreparedBatch":
        """Batch that starts from the stream of per-fragment alignment-path lists (rpvg_amd/host/align_index.hpp): chunks = a sequence of
        index.FragmentLists with GLOBAL path ids, index_params = index.IndexParams, path_info = a ClusterBatch whose paths, clusters
        back to back, are the global paths 0 .. P-1.  The index (histogram, equal lists, clusters, their order) and the rows are made
        on the GPU; the prepared batch holds the clusters in the index's order.  The result carries .index_info, .frag_counts,
        .cluster_path_off and .cluster_paths (the global paths of every cluster).
        path_table (an index.PathTable, instead of path_info): the PathInfo of the global paths goes to the GPU as a table and the
        path side of the batch — group ids, haplotype columns — is formed there: the result reports .has_source_columns when the
        table has source ids.  collapse_names (the table needs name_id): the batch's columns are the name groups of every cluster
        and its paths the collapsed ones (`-i transcripts --path-info`)."""
        from . import index as index_mod
        if (path_table is None) == (path_info is None):
            raise ValueError("prepare_from_fragments: either path_info or path_table")
        if collapse_names and (path_table is None or path_table.name_id is None):
            raise ValueError("prepare_from_fragments: collapse_names needs a path_table with name_id")
        chunks = list(chunks)
        cchunks = (index_mod.CFragmentLists * max(len(chunks), 1))(*[c.as_c() for c in chunks])
        cparams = index_params.as_c()
        sets = list(extra_sets or [])
        off = np.zeros(len(sets) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in sets], dtype=np.uint64) if sets else []
        flat = np.ascontiguousarray([p for x in sets for p in x], dtype=np.uint32)
        if frag is None:
            frag = (300.0, 50.0, 0.0, 10)
        P = index_params.num_paths
        info = index_mod.CIndexInfo()
        counts = np.zeros(index_params.max_frag_length + 1, dtype=np.uint32)
        cpo, cpaths = np.zeros(P + 1, dtype=np.uint64), np.zeros(max(P, 1), dtype=np.uint32)
        prep = PreparedBatch.__new__(PreparedBatch)
        prep.engine = self
        prep.batch = path_info
        secs = C.c_double(0)
        if path_table is not None:
            if path_table.num_paths != P:
                raise ValueError("prepare_from_fragments: one table entry per path of the index")
            ct = path_table.as_c()
            prep.handle = lib().rpvg_amd_batch_prepare_from_fragments_table(
                self.handle, C.addressof(cchunks), len(chunks), C.addressof(cparams), C.c_void_p(off.ctypes.data if sets else None),
                C.c_void_p(flat.ctypes.data if flat.size else None), len(sets), C.addressof(ct), 1 if collapse_names else 0,
                frag[0], frag[1], frag[2], int(frag[3]), min_noise_prob, prob_precision, C.addressof(info),
                C.c_void_p(counts.ctypes.data), C.c_void_p(cpo.ctypes.data), C.c_void_p(cpaths.ctypes.data), C.byref(secs))
        else:
            cb = path_info.as_c()
            prep.handle = lib().rpvg_amd_batch_prepare_from_fragments(
                self.handle, C.addressof(cchunks), len(chunks), C.addressof(cparams), C.c_void_p(off.ctypes.data if sets else None),
                C.c_void_p(flat.ctypes.data if flat.size else None), len(sets), C.byref(cb), frag[0], frag[1], frag[2], int(frag[3]),
                min_noise_prob, prob_precision, C.addressof(info), C.c_void_p(counts.ctypes.data), C.c_void_p(cpo.ctypes.data),
                C.c_void_p(cpaths.ctypes.data), C.byref(secs))
        if not prep.handle:
            raise hip.EngineError(f"batch prepare from fragments failed: {_err()}")
        prep.index_info = info
        prep.frag_counts = counts
        prep.cluster_path_off = cpo[:info.num_clusters + 1].copy()
        prep.cluster_paths = cpaths[:P].copy()
        prep.row_construction_seconds = secs.value
        return prep

    def prepare_synth_dense(self, seed: int, rows: int, paths: int) -> "PreparedBatch":
        """BASELINE.json configs[1] as a resident batch for the estimator classes: one cluster of `rows` rows over all `paths`
        paths, generated on the GPU (rpvg_hip_synth_dense_cluster_batch; every row one read pair)."""
        prep = PreparedBatch.__new__(PreparedBatch)
        prep.engine = self
        prep.batch = None
        prep.handle = lib().rpvg_amd_batch_prepare_synth_dense(self.handle, C.c_uint64(seed), C.c_uint64(rows), C.c_uint32(paths))
        if not prep.handle:
            raise hip.EngineError(f"synthetic dense batch failed: {_err()}")
        return prep

    def run(self, model: str, params: CParams, prepared: "PreparedBatch") -> Tuple[List[ClusterEstimates], float]:
        """Estimates of every cluster + wall seconds of the estimator call (inputs already on the GPU)."""
        secs = C.c_double(0)
        h = lib().rpvg_amd_run(self.handle, prepared.handle, model.encode(), C.byref(params), C.byref(secs))
        if not h:
            raise hip.EngineError(f"run({model}) failed: {_err()}")
        try:
            view = CEstimatesView()
            lib().rpvg_amd_result_view(h, C.byref(view))
            out = decode_view(view)
        finally:
            lib().rpvg_amd_result_free(h)
        return out, secs.value

    def generators_after(self, model: str, params: CParams, prepared: "PreparedBatch", num_clusters: int) -> List[int]:
        """Runs the batch estimate with cluster i on mt19937(rng_seed + i) and returns every generator's next output (tests: where
        a route leaves the callers' generators)."""
        out = (C.c_uint32 * max(num_clusters, 1))()
        if lib().rpvg_amd_run_generators_after(self.handle, prepared.handle, model.encode(), C.byref(params), out) != 0:
            raise hip.EngineError(f"generators_after({model}) failed: {_err()}")
        return [int(x) for x in out[:num_clusters]]

    def run_team(self, model: str, params: CParams, prepared: "PreparedBatch", threads: int, decode: bool = True):
        """The reference's cluster loop (src/main.cpp:829,976-977): PathEstimator::estimate() once per cluster from an OpenMP team
        of `threads`; `prepared` was made with per_cluster=True.  Returns (estimates or None, wall seconds)."""
        secs = C.c_double(0)
        if lib().rpvg_amd_run_team(self.handle, prepared.handle, model.encode(), C.byref(params), threads, C.byref(secs)) != 0:
            raise hip.EngineError(f"run_team({model}) failed: {_err()}")
        if not decode:
            return None, secs.value
        h = lib().rpvg_amd_run_team_result(prepared.handle)
        if not h:
            raise hip.EngineError(f"run_team({model}) result failed: {_err()}")
        try:
            view = CEstimatesView()
            lib().rpvg_amd_result_view(h, C.byref(view))
            out = decode_view(view)
        finally:
            lib().rpvg_amd_result_free(h)
        return out, secs.value

    def run_raw(self, model: str, params: CParams, prepared: "PreparedBatch") -> float:
        """Like run() but leaves the estimates in the C++ PathClusterEstimates containers of the prepared
        batch instead of flattening and decoding them (bench inner loop)."""
        secs = C.c_double(0)
        rc = lib().rpvg_amd_run_inplace(self.handle, prepared.handle, model.encode(), C.byref(params), C.byref(secs))
        if rc != 0:
            raise hip.EngineError(f"run({model}) failed: {_err()}")
        return secs.value


    def run_from_alignments_raw(self, model: str, params: CParams, prepared: "PreparedBatch") -> Tuple[float, float]:
        """One pass alignment-path lists (resident) -> rows -> estimates, everything on the GPU; returns the wall seconds
        of the row construction and of the estimator call.  `prepared` comes from prepare_from_alignments()."""
        rows_s, est_s = C.c_double(0), C.c_double(0)
        rc = lib().rpvg_amd_run_from_alignments_inplace(self.handle, prepared.handle, model.encode(), C.byref(params),
                                                        C.byref(rows_s), C.byref(est_s))
        if rc != 0:
            raise hip.EngineError(f"run_from_alignments({model}) failed: {_err()}")
        return rows_s.value, est_s.value


class DeviceGroup:
    """The GPUs of one node behind one call (rpvg_amd/host/device_group.hpp): one engine and one host thread per
    entry of `devices`, clusters bin-packed over them, final abundance gather over the group's communicator."""

    def __init__(self, devices):
        arr = (C.c_int * len(devices))(*devices)
        self.handle = lib().rpvg_amd_group_create(arr, len(devices))
        if not self.handle:
            raise hip.EngineError(f"device group create failed: {_err()}")
        self.num_clusters = 0

    def close(self):
        if self.handle:
            lib().rpvg_amd_group_destroy(self.handle)
            self.handle = None

    def has_communicator(self) -> bool:
        return bool(lib().rpvg_amd_group_has_communicator(self.handle))

    def run(self, model: str, params: CParams, batch: ClusterBatch) -> Tuple[List[ClusterEstimates], float]:
        secs = C.c_double(0)
        cb = batch.as_c()
        h = lib().rpvg_amd_group_run(self.handle, C.byref(cb), model.encode(), C.byref(params), C.byref(secs))
        if not h:
            raise hip.EngineError(f"group run({model}) failed: {_err()}")
        try:
            view = CEstimatesView()
            lib().rpvg_amd_result_view(h, C.byref(view))
            out = decode_view(view)
        finally:
            lib().rpvg_amd_result_free(h)
        self.num_clusters = batch.num_clusters
        return out, secs.value

    def partition(self):
        import numpy as np
        out = np.zeros(self.num_clusters, dtype=np.uint32)
        if lib().rpvg_amd_group_partition(self.handle, C.c_void_p(out.ctypes.data), self.num_clusters) != 0:
            raise hip.EngineError(f"group partition failed: {_err()}")
        return out

    def gather(self, capacity: int):
        """(abundances of all clusters in cluster order, TPM denominator) after the collective of the last run."""
        import numpy as np
        out = np.zeros(max(1, capacity), dtype=np.float64)
        count, total = C.c_uint64(0), C.c_double(0)
        if lib().rpvg_amd_group_gather(self.handle, C.c_void_p(out.ctypes.data), capacity, C.byref(count), C.byref(total)) != 0:
            raise hip.EngineError(f"group gather failed: {_err()}")
        return out[:count.value].copy(), total.value


class Pipeline:
    """Several batches in flight on one GPU (rpvg_amd/host/batch_pipeline.hpp): an uploader thread and `workers` estimator
    threads, each with an engine of its own; submit() returns at once, wait() when every submitted batch is done."""

    def __init__(self, model: str, params: CParams, device: int = 0, workers: int = 0):
        self.handle = lib().rpvg_amd_pipeline_create(device, model.encode(), C.byref(params), workers)
        if not self.handle:
            raise hip.EngineError(f"pipeline create failed: {_err()}")
        self._keep = []  # the host batches (and their C views) of the submissions since the last wait()

    @property
    def workers(self) -> int:
        return int(lib().rpvg_amd_pipeline_workers(self.handle))

    def prepare_slots(self, batch: ClusterBatch, slots: int):
        """`slots` sets of estimates containers for batches with the clusters (paths) of `batch`."""
        cb = batch.as_c()
        if lib().rpvg_amd_pipeline_prepare_slots(self.handle, C.byref(cb), slots) != 0:
            raise hip.EngineError(f"pipeline prepare failed: {_err()}")

    def prepare_slot(self, slot: int, part):
        """The containers of one slot for the clusters of `part` (a ClusterBatch or a ClusterRange of one): the parts of one data
        set go to slots of their own."""
        cb = part.as_c(True)
        if lib().rpvg_amd_pipeline_prepare_slot(self.handle, C.byref(cb), slot) != 0:
            raise hip.EngineError(f"pipeline prepare failed: {_err()}")

    def submit(self, batch, slot: int, compact: bool = False, narrow: bool = False):
        """compact / narrow: the forms of the batch's arrays made for the copy (ClusterBatch.as_c).  `batch`: a ClusterBatch or a
        ClusterRange."""
        cb = batch.as_c(compact, narrow) if narrow else batch.as_c(compact)
        self._keep.append((batch, cb))
        if lib().rpvg_amd_pipeline_submit(self.handle, C.byref(cb), slot) != 0:
            raise hip.EngineError(f"pipeline submit failed: {_err()}")

    def wait(self):
        rc = lib().rpvg_amd_pipeline_wait(self.handle)
        self._keep.clear()
        if rc != 0:
            raise hip.EngineError(f"pipeline batch failed: {_err()}")

    def result(self, slot: int) -> List[ClusterEstimates]:
        h = lib().rpvg_amd_pipeline_result(self.handle, slot)
        if not h:
            raise hip.EngineError(f"pipeline result failed: {_err()}")
        try:
            view = CEstimatesView()
            lib().rpvg_amd_result_view(h, C.byref(view))
            return decode_view(view)
        finally:
            lib().rpvg_amd_result_free(h)

    def stats(self) -> dict:
        s = hip.CKernelStats()
        up = (C.c_double * 6)()
        if lib().rpvg_amd_pipeline_stats_get(self.handle, C.byref(s), up) != 0:
            raise hip.EngineError(f"pipeline stats failed: {_err()}")
        out = s.as_dict()
        out["upload_seconds_per_batch"] = up[0]
        out["upload_copies_ms_per_batch"] = up[1]   # HIP-event span around the H2D copies of a batch
        out["upload_kernels_ms_per_batch"] = up[2]  # ... around the kernels behind them
        out["worker_finish_ms_per_batch"], out["worker_estimate_ms_per_batch"], out["worker_idle_ms_per_batch"] = up[3] * 1e3, up[4] * 1e3, up[5] * 1e3
        return out

    def reset_stats(self):
        if lib().rpvg_amd_pipeline_stats_reset(self.handle) != 0:
            raise hip.EngineError(f"pipeline stats reset failed: {_err()}")

    def completions(self, capacity: int = 4096):
        """Seconds since the last reset_stats() at which the batches since then were done, in order of completion."""
        import numpy as np
        out = np.zeros(capacity, dtype=np.float64)
        count = C.c_uint64(0)
        lib().rpvg_amd_pipeline_completions(self.handle, C.c_void_p(out.ctypes.data), capacity, C.byref(count))
        return out[:min(capacity, count.value)].copy()

    def close(self):
        if self.handle:
            lib().rpvg_amd_pipeline_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PreparedBatch:
    def __init__(self, engine: Engine, batch: ClusterBatch, per_cluster: bool):
        self.engine = engine
        self.batch = batch
        cb = batch.as_c()
        self.handle = lib().rpvg_amd_batch_prepare(engine.handle, C.byref(cb), 1 if per_cluster else 0)
        if not self.handle:
            raise hip.EngineError(f"batch prepare failed: {_err()}")

    def reupload(self, engine: "Engine", batch: Optional[ClusterBatch] = None, compact: bool = False) -> float:
        """Replaces the resident rows by a fresh upload of `batch` (default: the batch this was prepared from) through
        `engine` (an uploader engine on the same GPU keeps the copy off the estimating engine's streams); seconds."""
        if batch is None and self.batch is None:
            raise ValueError("reupload: this batch was prepared without a host batch (path_table=...): pass the batch to upload")
        cb = (batch or self.batch).as_c(compact)
        secs = C.c_double(0)
        if lib().rpvg_amd_batch_reupload(engine.handle, self.handle, C.byref(cb), C.byref(secs)) != 0:
            raise hip.EngineError(f"batch reupload failed: {_err()}")
        return secs.value

    @property
    def has_source_columns(self) -> bool:
        """Whether the resident batch holds the haplotype columns of its clusters (formed on the device)."""
        return bool(lib().rpvg_amd_batch_has_source_columns(self.handle))

    def free(self):
        if self.handle:
            lib().rpvg_amd_batch_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def run(model: str, params: CParams, batch: ClusterBatch, device: int = 0, per_cluster: bool = False) -> List[ClusterEstimates]:
    """One-shot convenience: upload, estimate, decode."""
    eng = Engine(device)
    try:
        prep = eng.prepare(batch, per_cluster)
        try:
            out, _ = eng.run(model, params, prep)
        finally:
            prep.free()
    finally:
        eng.close()
    return out
