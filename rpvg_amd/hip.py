"""ctypes binding of ``include/rpvg_hip.h`` (librpvg_hip.so) for tests and bench.

Thin: every function maps 1:1 to a C-ABI entry point.  There is no fallback:
if the shared library is missing or no GPU is usable, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .batch import CClusterBatch, ClusterBatch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librpvg_hip.so")

# every symbol include/rpvg_hip.h declares
EXPORTS = [
    "rpvg_hip_device_count", "rpvg_hip_create", "rpvg_hip_create_uploader", "rpvg_hip_destroy", "rpvg_hip_last_error", "rpvg_hip_synchronize",
    "rpvg_hip_device_info", "rpvg_hip_malloc", "rpvg_hip_free", "rpvg_hip_memcpy_h2d", "rpvg_hip_memcpy_d2h",
    "rpvg_hip_batch_upload", "rpvg_hip_batch_free", "rpvg_hip_em_solve", "rpvg_hip_em_dense",
    "rpvg_hip_dense_from_cluster", "rpvg_hip_groups_build", "rpvg_hip_groups_free", "rpvg_hip_groups_collapse_info", "rpvg_hip_group_loglik",
    "rpvg_hip_synth_dense_cluster", "rpvg_hip_stats_get", "rpvg_hip_stats_reset", "rpvg_hip_stats_intervals", "rpvg_hip_em_kernel_name",
    "rpvg_hip_gibbs_read_counts", "rpvg_hip_min_path_cover", "rpvg_hip_min_path_cover_any", "rpvg_hip_cover_limits", "rpvg_hip_bounded_pair_posteriors", "rpvg_hip_pair_posteriors_get", "rpvg_hip_pair_posteriors_free",
    "rpvg_hip_em_dense_sharded", "rpvg_hip_synth_dense_rows", "rpvg_hip_synth_dense_cluster_batch", "rpvg_hip_comm_unique_id", "rpvg_hip_comm_init",
    "rpvg_hip_comm_destroy", "rpvg_hip_comm_allreduce_sum_f64", "rpvg_hip_comm_init_all", "rpvg_hip_gather", "rpvg_hip_host_register", "rpvg_hip_host_unregister", "rpvg_hip_group_conditionals",
    "rpvg_hip_group_gibbs", "rpvg_hip_group_gibbs_polyploid", "rpvg_hip_gibbs_sets_get", "rpvg_hip_gibbs_sets_free",
    "rpvg_hip_alignments_upload", "rpvg_hip_alignments_free", "rpvg_hip_read_rows_build", "rpvg_hip_read_rows_to_batch",
    "rpvg_hip_read_rows_view", "rpvg_hip_read_rows_sizes", "rpvg_hip_read_rows_free", "rpvg_hip_path_clusters", "rpvg_hip_debug_log",
    "rpvg_hip_nested_subset_em", "rpvg_hip_subset_em_get", "rpvg_hip_subset_em_free",
    "rpvg_hip_subset_em_keep_device", "rpvg_hip_subset_em_part", "rpvg_hip_subset_em_kept_bytes", "rpvg_hip_flat_estimates_gather", "rpvg_hip_flat_estimates_view",
    "rpvg_hip_flat_estimates_get", "rpvg_hip_flat_estimates_free",
    "rpvg_hip_nested_full_subset_em", "rpvg_hip_subset_em_get_sets",
    "rpvg_hip_nested_independent_subset_em", "rpvg_hip_subset_em_get_independent", "rpvg_hip_independent_draws_get",
    "rpvg_hip_independent_limits", "rpvg_hip_independent_stats_get",
    "rpvg_hip_batch_cluster_totals", "rpvg_hip_batch_has_source_columns", "rpvg_hip_batch_source_columns_sizes",
    "rpvg_hip_batch_source_columns_get", "rpvg_hip_groups_build_from_sources", "rpvg_hip_groups_build_single_paths", "rpvg_hip_batch_upload_begin", "rpvg_hip_batch_upload_finish", "rpvg_hip_create_with_streams",
    "rpvg_hip_batch_upload_finish_queue", "rpvg_hip_batch_upload_finish_wait",
    "rpvg_hip_batch_upload_segments", "rpvg_hip_pinned_alloc", "rpvg_hip_pinned_free", "rpvg_hip_thread_wait_spin_us",
    "rpvg_hip_group_full_posteriors", "rpvg_hip_full_set_count",
    "rpvg_hip_frag_length_fit", "rpvg_hip_frag_length_table", "rpvg_hip_frag_length_table_get", "rpvg_hip_frag_length_table_free",
    "rpvg_hip_effective_lengths", "rpvg_hip_alignments_set_effective_lengths", "rpvg_hip_frag_length_eval",
    "rpvg_hip_align_index_create", "rpvg_hip_align_index_free", "rpvg_hip_align_index_add", "rpvg_hip_align_index_finish",
    "rpvg_hip_align_index_frag_counts", "rpvg_hip_align_index_view", "rpvg_hip_align_index_alignments",
    "rpvg_hip_path_table_upload", "rpvg_hip_path_table_free", "rpvg_hip_read_rows_to_batch_with_paths", "rpvg_hip_batch_path_group_ids",
    "rpvg_hip_name_groups_limits", "rpvg_hip_align_index_name_groups", "rpvg_hip_name_groups_view", "rpvg_hip_name_groups_free",
    "rpvg_hip_estimates_table_build", "rpvg_hip_estimates_table_tpm", "rpvg_hip_estimates_table_view", "rpvg_hip_estimates_table_limits",
    "rpvg_hip_estimates_table_free",
    "rpvg_hip_gibbs_table_build", "rpvg_hip_gibbs_table_view", "rpvg_hip_gibbs_table_rows", "rpvg_hip_gibbs_table_limits", "rpvg_hip_gibbs_table_free",
    "rpvg_hip_gibbs_read_counts_resident", "rpvg_hip_gibbs_samples_get", "rpvg_hip_gibbs_samples_free", "rpvg_hip_gibbs_table_build_resident",
    "rpvg_hip_gibbs_table_text", "rpvg_hip_estimates_table_text", "rpvg_hip_table_text_view", "rpvg_hip_table_text_get", "rpvg_hip_table_text_guards",
    "rpvg_hip_table_text_free", "rpvg_hip_estimates_set_text", "rpvg_hip_rows_text", "rpvg_hip_read_rows_text",
    "rpvg_hip_table_text_sizes", "rpvg_hip_table_text_bgzf", "rpvg_hip_bytes_bgzf", "rpvg_hip_text_bgzf_view", "rpvg_hip_text_bgzf_get", "rpvg_hip_text_bgzf_guards", "rpvg_hip_text_bgzf_free",
    "rpvg_hip_text_rows", "rpvg_hip_table_text_rows", "rpvg_hip_parsed_dump_rows", "rpvg_hip_parsed_dump_view", "rpvg_hip_parsed_dump_labels", "rpvg_hip_parsed_dump_free", "rpvg_hip_parse_stats_get",
    "rpvg_hip_align_index_alignments_collapsed",
    "rpvg_hip_batch_rows_sizes", "rpvg_hip_batch_rows_get",
    "rpvg_hip_segment_sort_words", "rpvg_hip_groups_rows",
]

COMM_ID_BYTES = 128  # RPVG_HIP_COMM_ID_BYTES


class EngineError(RuntimeError):
    pass


class CEmProblems(C.Structure):
    _fields_ = [("num_problems", C.c_uint32), ("cluster", C.c_void_p), ("col_off", C.c_void_p), ("col_path", C.c_void_p),
                ("collapse_precision", C.c_double)]


class CEmResults(C.Structure):
    _fields_ = [("abundances", C.c_void_p), ("noise_count", C.c_void_p), ("total_count", C.c_void_p),
                ("iterations", C.c_void_p)]


class CGroupSpec(C.Structure):
    _fields_ = [("num_matrices", C.c_uint32), ("cluster", C.c_void_p), ("group_off", C.c_void_p),
                ("group_path_off", C.c_void_p), ("group_path", C.c_void_p), ("normalise", C.c_int32),
                ("collapse_precision", C.c_double)]


class CGibbsSpec(C.Structure):
    _fields_ = [("num_problems", C.c_uint32), ("group_size", C.c_uint32), ("matrix", C.c_void_p), ("num_chains", C.c_void_p),
                ("num_burn_its", C.c_void_p), ("num_gibbs_its", C.c_void_p), ("log_freq", C.c_void_p), ("num_generators", C.c_uint32),
                ("generator_problem_off", C.c_void_p), ("generator_problem", C.c_void_p), ("generator_words", C.c_void_p)]


class CGibbsSetsView(C.Structure):
    _fields_ = [("num_problems", C.c_uint32), ("group_size", C.c_uint32), ("set_off", C.POINTER(C.c_uint64)),
                ("first", C.POINTER(C.c_uint32)), ("second", C.POINTER(C.c_uint32)), ("count", C.POINTER(C.c_uint32)),
                ("words_consumed", C.POINTER(C.c_uint64)), ("generator_state", C.POINTER(C.c_uint32)), ("rounds", C.c_uint32),
                ("conditionals", C.c_uint64), ("members", C.POINTER(C.c_uint32))]


class CPairPosteriorsView(C.Structure):
    _fields_ = [("num_matrices", C.c_uint32), ("pair_off", C.POINTER(C.c_uint64)), ("first", C.POINTER(C.c_uint32)),
                ("second", C.POINTER(C.c_uint32)), ("posterior", C.POINTER(C.c_double))]


class CSubsetEmSetsView(C.Structure):
    """rpvg_hip_subset_em_sets_view"""
    _fields_ = [("num_matrices", C.c_uint32), ("group_size", C.c_uint32), ("subset_off", C.POINTER(C.c_uint64)),
                ("weight", C.POINTER(C.c_double)), ("path_off", C.POINTER(C.c_uint64)), ("path", C.POINTER(C.c_uint32)),
                ("col_off", C.POINTER(C.c_uint64)), ("col_path", C.POINTER(C.c_uint32)), ("abundances", C.POINTER(C.c_double)),
                ("noise_count", C.POINTER(C.c_double)), ("total_count", C.POINTER(C.c_double)), ("iterations", C.POINTER(C.c_uint32)),
                ("retained_off", C.POINTER(C.c_uint64)), ("retained_rank", C.POINTER(C.c_uint64)),
                ("retained_posterior", C.POINTER(C.c_double)), ("set_count", C.POINTER(C.c_uint32)),
                ("cluster_noise_count", C.POINTER(C.c_double)), ("set_size", C.POINTER(C.c_uint32)), ("set_member", C.POINTER(C.c_uint32)),
                ("set_posterior", C.POINTER(C.c_double)), ("set_abundance", C.POINTER(C.c_double))]


class CIndependentSpec(C.Structure):
    """rpvg_hip_independent_spec"""
    _fields_ = [("num_clusters", C.c_uint32), ("matrix_off", C.c_void_p), ("group_size", C.c_uint32), ("column_counts", C.c_void_p),
                ("log_freq", C.c_void_p), ("min_hap_prob", C.c_double), ("max_em_its", C.c_uint32), ("max_rel_em_conv", C.c_double),
                ("collapse_precision", C.c_double), ("generator_words", C.c_void_p), ("keep_draws", C.c_int32)]


class CSubsetEmIndependentView(C.Structure):
    """rpvg_hip_subset_em_independent_view"""
    _fields_ = [("num_clusters", C.c_uint32), ("group_size", C.c_uint32), ("num_samples", C.c_uint32), ("subset_off", C.POINTER(C.c_uint64)),
                ("weight", C.POINTER(C.c_double)), ("path_off", C.POINTER(C.c_uint64)), ("path", C.POINTER(C.c_uint32)),
                ("col_off", C.POINTER(C.c_uint64)), ("col_path", C.POINTER(C.c_uint32)), ("abundances", C.POINTER(C.c_double)),
                ("noise_count", C.POINTER(C.c_double)), ("total_count", C.POINTER(C.c_double)), ("iterations", C.POINTER(C.c_uint32)),
                ("set_count", C.POINTER(C.c_uint32)), ("cluster_noise_count", C.POINTER(C.c_double)), ("set_size", C.POINTER(C.c_uint32)),
                ("set_member", C.POINTER(C.c_uint32)), ("set_posterior", C.POINTER(C.c_double)), ("set_abundance", C.POINTER(C.c_double)),
                ("sample_count", C.POINTER(C.c_uint32)), ("words_consumed", C.POINTER(C.c_uint64)), ("generator_state", C.POINTER(C.c_uint32))]


class CIndependentLimits(C.Structure):
    """rpvg_independent_limits"""
    _fields_ = [("max_group_size", C.c_uint32), ("max_samples", C.c_uint32), ("max_transcript_sets", C.c_uint64), ("words_per_draw", C.c_uint32),
                ("state_words", C.c_uint32), ("max_work_bytes", C.c_uint64)]


class CIndependentStats(C.Structure):
    """rpvg_hip_independent_stats"""
    _fields_ = [("calls_completed", C.c_uint64), ("draws", C.c_uint64), ("subsets", C.c_uint64)]


class CParseStats(C.Structure):
    """rpvg_hip_parse_stats"""
    _fields_ = [("calls_completed", C.c_uint64), ("exact_tokens", C.c_uint64)]


def independent_limits() -> CIndependentLimits:
    """The numbers of rpvg_hip_nested_independent_subset_em's plan (rpvg_amd/csrc/subset_independent_plan.hpp); needs no GPU."""
    out = CIndependentLimits()
    lib().rpvg_hip_independent_limits(C.byref(out))
    return out


EM_KERNELS = 12  # RPVG_HIP_EM_KERNELS


class CEmKernelStats(C.Structure):
    _fields_ = [("ms", C.c_double), ("launches", C.c_uint64), ("problems", C.c_uint64), ("iterations", C.c_uint64),
                ("max_iterations", C.c_uint64), ("alg_bytes", C.c_double)]


class CKernelStats(C.Structure):
    _fields_ = [
        ("em_sparse_ms", C.c_double), ("em_sparse_launches", C.c_uint64), ("em_sparse_alg_bytes", C.c_double),
        ("em_dense_ms", C.c_double), ("em_dense_launches", C.c_uint64), ("em_dense_alg_bytes", C.c_double),
        ("loglik_ms", C.c_double), ("loglik_launches", C.c_uint64), ("loglik_evals", C.c_double),
        ("build_ms", C.c_double), ("build_launches", C.c_uint64),
        ("h2d_ms", C.c_double), ("h2d_bytes", C.c_double),
        ("em_iterations_total", C.c_uint64),
        ("search_pairs_possible", C.c_double), ("search_pairs_table", C.c_double), ("search_pairs_kept", C.c_double),
        ("em_kernel", CEmKernelStats * EM_KERNELS),
        ("collapse_ms", C.c_double), ("busy_ms", C.c_double), ("gibbs_ms", C.c_double),
        ("search_tile_ms", C.c_double), ("search_tile_launches", C.c_uint64),
        ("gibbs_calls_completed", C.c_uint64),
        ("gibbs_count_grid_problems", C.c_uint64), ("gibbs_count_grid_iterations", C.c_uint64),
        ("cover_grid_problems", C.c_uint64), ("cover_grid_rounds", C.c_uint64),
        ("text_exact_cells", C.c_uint64),
        ("nested_full_calls", C.c_uint64), ("nested_full_sets", C.c_uint64), ("nested_full_retained", C.c_uint64),
    ]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "em_kernel"}
        d["em_kernel"] = {em_kernel_name(i): {n: getattr(self.em_kernel[i], n) for n, _ in CEmKernelStats._fields_} for i in range(EM_KERNELS)}
        return d


GRID_NEVER = 2 ** 64 - 1  # grid_min_work of Context.min_path_cover_any: every cluster that fits stays on the workgroup route


class CCoverLimits(C.Structure):
    """rpvg_cover_limits"""
    _fields_ = [("workgroup_max_paths", C.c_uint32), ("chunk_rounds", C.c_uint32), ("default_grid_min_work", C.c_uint64),
                ("grid_max_rows", C.c_uint64), ("grid_max_entries", C.c_uint64), ("pick_block", C.c_uint32), ("pick_per_thread", C.c_uint32),
                ("pick_max_blocks", C.c_uint32), ("strike_block", C.c_uint32), ("strike_max_blocks", C.c_uint32), ("hist_max_paths", C.c_uint32)]


def cover_limits() -> CCoverLimits:
    """The numbers of the minimum path cover's plan (rpvg_amd/csrc/cover_plan.hpp); needs no GPU."""
    out = CCoverLimits()
    lib().rpvg_hip_cover_limits(C.byref(out))
    return out


def em_kernel_name(index: int) -> str:
    f = lib().rpvg_hip_em_kernel_name
    f.restype = C.c_char_p
    return f(index).decode()


_lib = None


def lib() -> C.CDLL:
    """Loads librpvg_hip.so (built by __graft_entry__.build()); raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.rpvg_hip_last_error.restype = C.c_char_p
        L.rpvg_hip_full_set_count.restype = C.c_uint64
        L.rpvg_hip_subset_em_kept_bytes.restype = C.c_uint64
        L.rpvg_hip_cover_limits.restype = None
        L.rpvg_hip_parsed_dump_rows.restype = C.c_void_p
        L.rpvg_hip_parsed_dump_rows.argtypes = [C.c_void_p]
        L.rpvg_hip_parsed_dump_free.restype = None
        L.rpvg_hip_parsed_dump_free.argtypes = [C.c_void_p]
        L.rpvg_hip_independent_limits.restype = None
        for name in EXPORTS:
            getattr(L, name)
        _lib = L
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        raise EngineError(f"{what} failed ({rc}): {lib().rpvg_hip_last_error().decode()}")


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().rpvg_hip_device_count(C.byref(n))
    return n.value if rc == 0 else 0


class CClusterSegment(C.Structure):
    """rpvg_cluster_segment (include/rpvg_batch.h)."""
    _fields_ = [("base", C.c_void_p), ("bytes", C.c_uint64), ("num_rows", C.c_uint32), ("num_groups", C.c_uint32), ("num_entries", C.c_uint32),
                ("num_paths", C.c_uint32), ("num_sources", C.c_uint32), ("has_paths", C.c_uint32), ("total_read_count", C.c_uint64),
                ("row_count_at", C.c_uint64), ("row_noise_at", C.c_uint64), ("row_grp_off_at", C.c_uint64), ("grp_idx_off_at", C.c_uint64),
                ("grp_prob_at", C.c_uint64), ("path_idx_at", C.c_uint64), ("path_group_id_at", C.c_uint64), ("path_source_off_at", C.c_uint64),
                ("source_id_at", C.c_uint64), ("has_columns", C.c_uint32), ("num_columns", C.c_uint32), ("num_column_paths", C.c_uint32),
                ("max_column_paths", C.c_uint32), ("col_count_at", C.c_uint64), ("col_end_at", C.c_uint64), ("col_path_at", C.c_uint64)]


class PinnedSegments:
    """The clusters of a ClusterBatch as one rpvg_cluster_segment each, every segment in a page-locked block of its own
    (rpvg_hip_pinned_alloc) — what the threads of a team calling PathEstimator::estimate() hand to the call combiner."""

    def __init__(self, host: ClusterBatch, with_paths: bool = True, columns=None):
        """columns: per cluster (multiplicities, [path list of every column]) — the caller's own haplotype columns
        (rpvg_cluster_segment::has_columns); the source ids then stay behind."""
        L = lib()
        L.rpvg_hip_pinned_free.argtypes = [C.c_void_p]
        K = host.num_clusters
        self.blocks = []
        self.segments = (CClusterSegment * max(K, 1))()
        self.arrays = []  # numpy views of the blocks, per cluster: name -> array (tests corrupt them)
        for k in range(K):
            r0, r1 = int(host.cluster_row_off[k]), int(host.cluster_row_off[k + 1])
            p0, p1 = int(host.cluster_path_off[k]), int(host.cluster_path_off[k + 1])
            g0, g1 = int(host.row_grp_off[r0]), int(host.row_grp_off[r1])
            e0, e1 = int(host.grp_idx_off[g0]), int(host.grp_idx_off[g1])
            s0, s1 = (int(host.path_source_off[p0]), int(host.path_source_off[p1])) if with_paths else (0, 0)
            pieces = [("row_noise", host.row_noise[r0:r1], np.float64), ("grp_prob", host.grp_prob[g0:g1], np.float64),
                      ("row_count", host.row_count[r0:r1], np.uint32), ("row_grp_off", host.row_grp_off[r0:r1 + 1] - g0, np.uint32),
                      ("grp_idx_off", host.grp_idx_off[g0:g1 + 1] - e0, np.uint32), ("path_idx", host.path_idx[e0:e1], np.uint32)]
            if columns is not None:
                counts, lists = columns[k]
                ends = np.cumsum([len(x) for x in lists]).astype(np.uint32) if lists else np.zeros(0, dtype=np.uint32)
                flat = np.array([p for x in lists for p in x], dtype=np.uint32)
                pieces += [("path_group_id", host.path_group_id[p0:p1], np.uint32), ("col_count", np.array(counts, dtype=np.uint32), np.uint32),
                           ("col_end", ends, np.uint32), ("col_path", flat, np.uint32)]
            elif with_paths:
                pieces += [("path_group_id", host.path_group_id[p0:p1], np.uint32), ("path_source_off", host.path_source_off[p0:p1 + 1] - s0, np.uint32),
                           ("source_id", host.source_id[s0:s1], np.uint32)]
            at, places = 0, {}
            for name, values, dt in pieces:
                places[name] = at
                at += (len(values) * np.dtype(dt).itemsize + 7) & ~7
            block = C.c_void_p()
            _check(L.rpvg_hip_pinned_alloc(C.c_uint64(max(at, 8)), C.byref(block)), "rpvg_hip_pinned_alloc")
            self.blocks.append(block)
            raw = (C.c_ubyte * max(at, 8)).from_address(block.value)
            views = {}
            for name, values, dt in pieces:
                view = np.frombuffer(raw, dtype=dt, count=len(values), offset=places[name])
                view[:] = np.asarray(values).astype(dt)
                views[name] = view
            self.arrays.append(views)
            seg = self.segments[k]
            seg.base, seg.bytes = block.value, max(at, 8)
            seg.num_rows, seg.num_groups, seg.num_entries, seg.num_paths, seg.num_sources = r1 - r0, g1 - g0, e1 - e0, p1 - p0, s1 - s0
            seg.has_paths = 1 if (with_paths and columns is None) else 0
            if columns is not None:
                counts, lists = columns[k]
                seg.has_columns, seg.num_columns, seg.num_column_paths = 1, len(counts), sum(len(x) for x in lists)
                seg.max_column_paths = max([len(x) for x in lists], default=0)
                seg.num_sources = 0
            seg.total_read_count = int(host.row_count[r0:r1].astype(np.uint64).sum())
            for name in places:
                setattr(seg, name + "_at", places[name])
        self.count = K

    def free(self):
        for block in self.blocks:
            lib().rpvg_hip_pinned_free(block)
        self.blocks = []

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBatch:
    def __init__(self, ctx: "Context", host: ClusterBatch, compact: bool = False, segments: "PinnedSegments" = None, narrow: bool = False):
        self.ctx = ctx
        self.host = host
        self.handle = C.c_void_p()
        if segments is not None:
            _check(lib().rpvg_hip_batch_upload_segments(ctx.handle, segments.segments, C.c_uint32(segments.count), C.byref(self.handle)),
                   "rpvg_hip_batch_upload_segments")
            return
        cb = host.as_c(compact or narrow, narrow) if narrow else host.as_c(compact)
        _check(lib().rpvg_hip_batch_upload(ctx.handle, C.byref(cb), C.byref(self.handle)), "rpvg_hip_batch_upload")

    @classmethod
    def from_handle(cls, ctx: "Context", handle, num_clusters: int, num_paths: int) -> "DeviceBatch":
        """A batch made on the device (DeviceRows.to_batch): there is no host copy."""
        self = cls.__new__(cls)
        self.ctx, self.host, self.handle, self._shape = ctx, None, handle, (num_clusters, num_paths)
        return self

    @property
    def num_clusters(self) -> int:
        return self.host.num_clusters if self.host is not None else self._shape[0]

    @property
    def num_paths(self) -> int:
        return int(self.host.cluster_path_off[-1]) if self.host is not None else self._shape[1]

    def has_source_columns(self) -> bool:
        """Whether the upload formed the haplotype columns of the clusters on the device (path_sources.hip)."""
        return bool(lib().rpvg_hip_batch_has_source_columns(self.handle))

    def cluster_totals(self) -> np.ndarray:
        out = np.zeros(self.num_clusters, dtype=np.float64)
        _check(lib().rpvg_hip_batch_cluster_totals(self.handle, C.c_void_p(out.ctypes.data), self.num_clusters), "rpvg_hip_batch_cluster_totals")
        return out

    def path_group_ids(self) -> np.ndarray:
        """PathInfo::group_id of every path of a batch that has a path side (rpvg_hip_batch_path_group_ids)."""
        out = np.zeros(self.num_paths, dtype=np.uint32)
        _check(lib().rpvg_hip_batch_path_group_ids(self.ctx.handle, self.handle, C.c_void_p(out.ctypes.data)), "rpvg_hip_batch_path_group_ids")
        return out

    def rows(self):
        """The row side of the device batch (rpvg_hip_batch_rows_get; tests and tools): a dict of row_ent_off [R + 1], row_count
        [R] (doubles), row_noise [R], ent_path [NNZ] and ent_prob [NNZ]."""
        R, NNZ = C.c_uint64(0), C.c_uint64(0)
        _check(lib().rpvg_hip_batch_rows_sizes(self.handle, C.byref(R), C.byref(NNZ)), "rpvg_hip_batch_rows_sizes")
        out = dict(row_ent_off=np.zeros(R.value + 1, dtype=np.uint64), row_count=np.zeros(R.value, dtype=np.float64),
                   row_noise=np.zeros(R.value, dtype=np.float64), ent_path=np.zeros(NNZ.value, dtype=np.uint32),
                   ent_prob=np.zeros(NNZ.value, dtype=np.float64))
        _check(lib().rpvg_hip_batch_rows_get(self.ctx.handle, self.handle, *(C.c_void_p(out[name].ctypes.data) for name in
                                             ("row_ent_off", "row_count", "row_noise", "ent_path", "ent_prob"))), "rpvg_hip_batch_rows_get")
        return out

    def source_columns(self, cluster: int):
        """(multiplicities, [path list of every column]) of one cluster as the device formed them."""
        ncols, npaths = C.c_uint32(0), C.c_uint32(0)
        _check(lib().rpvg_hip_batch_source_columns_sizes(self.handle, cluster, C.byref(ncols), C.byref(npaths)), "rpvg_hip_batch_source_columns_sizes")
        counts = np.zeros(max(1, ncols.value), dtype=np.uint32)
        ends = np.zeros(max(1, ncols.value), dtype=np.uint32)
        paths = np.zeros(max(1, npaths.value), dtype=np.uint32)
        _check(lib().rpvg_hip_batch_source_columns_get(self.ctx.handle, self.handle, cluster, C.c_void_p(counts.ctypes.data),
                                                       C.c_void_p(ends.ctypes.data), C.c_void_p(paths.ctypes.data)), "rpvg_hip_batch_source_columns_get")
        lists, begin = [], 0
        for c in range(ncols.value):
            lists.append([int(p) for p in paths[begin:ends[c]]])
            begin = int(ends[c])
        return [int(x) for x in counts[:ncols.value]], lists

    def free(self):
        if self.handle:
            lib().rpvg_hip_batch_free(self.ctx.handle, self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceRows:
    """Rows resident on the GPU (rpvg_hip_read_rows)."""

    def __init__(self, ctx: "Context", handle):
        self.ctx = ctx
        self.handle = handle

    def download(self):
        """(ClusterBatch of the rows, build_ms, merge_ms)"""
        from . import rows as rows_mod
        view = CClusterBatch()
        b_ms, m_ms = C.c_double(0), C.c_double(0)
        _check(lib().rpvg_hip_read_rows_view(self.ctx.handle, self.handle, C.byref(view), C.byref(b_ms), C.byref(m_ms)),
               "rpvg_hip_read_rows_view")
        return rows_mod.rows_from_view(view), b_ms.value, m_ms.value

    def to_batch_handle(self) -> C.c_void_p:
        """rpvg_hip_batch made on the device from the rows (caller frees with rpvg_hip_batch_free)."""
        h = C.c_void_p()
        _check(lib().rpvg_hip_read_rows_to_batch(self.ctx.handle, self.handle, C.byref(h)), "rpvg_hip_read_rows_to_batch")
        return h

    def to_batch(self, index=None, table=None) -> "DeviceBatch":
        """The resident batch of the rows; with an index (rpvg_amd.index.AlignmentIndex) and its DevicePathTable the batch has its
        path side too (rpvg_hip_read_rows_to_batch_with_paths)."""
        assert (index is None) == (table is None)
        view = CClusterBatch()
        _check(lib().rpvg_hip_read_rows_sizes(self.ctx.handle, self.handle, C.byref(view)), "rpvg_hip_read_rows_sizes")
        K = view.num_clusters
        P = int(view.cluster_path_off[K])
        if index is None:
            return DeviceBatch.from_handle(self.ctx, self.to_batch_handle(), K, P)
        h = C.c_void_p()
        _check(lib().rpvg_hip_read_rows_to_batch_with_paths(self.ctx.handle, self.handle, index.handle, table.handle, C.byref(h)),
               "rpvg_hip_read_rows_to_batch_with_paths")
        return DeviceBatch.from_handle(self.ctx, h, K, P)

    def text(self, labels, effective_lengths, prob_precision: float = 1e-8, num_align_lists=None, cluster_index=None):
        """The --write-probs dump of the rows as a table_text.TableText, formatted on the GPU from the resident arrays: nothing is
        downloaded and the rows stay usable.  labels: table_text.Labels of the rows' columns with path_length (the name groups of a
        collapsed build); effective_lengths: one per column; num_align_lists and cluster_index: both or neither, one per cluster."""
        from . import table_text
        return table_text.TableText.resident_rows(self.ctx, self.handle, labels, effective_lengths, prob_precision, num_align_lists, cluster_index)

    def free(self):
        if self.handle:
            lib().rpvg_hip_read_rows_free(self.ctx.handle, self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceAlignments:
    """Alignment-path lists resident on the GPU (rpvg_hip_alignments)."""

    def __init__(self, ctx: "Context", host):
        self.ctx = ctx
        self.host = host
        self.handle = C.c_void_p()
        cb = host.as_c()
        _check(lib().rpvg_hip_alignments_upload(ctx.handle, C.byref(cb), C.byref(self.handle)), "rpvg_hip_alignments_upload")
        self.num_paths = len(host.path_effective_length)

    @classmethod
    def from_handle(cls, ctx: "Context", handle, num_paths: int) -> "DeviceAlignments":
        """A batch made on the device (rpvg_hip_align_index_alignments, rpvg_amd/index.py): there is no host copy."""
        self = cls.__new__(cls)
        self.ctx, self.host, self.handle, self.num_paths = ctx, None, handle, num_paths
        return self

    def build_rows(self, row_params, merge: bool = True) -> DeviceRows:
        cp = row_params.as_c()
        h = C.c_void_p()
        _check(lib().rpvg_hip_read_rows_build(self.ctx.handle, self.handle, C.byref(cp), C.c_int32(1 if merge else 0), C.byref(h)),
               "rpvg_hip_read_rows_build")
        return DeviceRows(self.ctx, h)

    def set_effective_lengths(self, path_lengths, loc: float, scale: float, shape: float) -> np.ndarray:
        """Replaces the resident path_effective_length by effectivePathLength(path length) and returns the values."""
        path_lengths = np.ascontiguousarray(path_lengths, dtype=np.uint32)
        assert path_lengths.size == self.num_paths
        out = np.zeros(path_lengths.size, dtype=np.float64)
        _check(lib().rpvg_hip_alignments_set_effective_lengths(
            self.ctx.handle, self.handle, C.c_double(loc), C.c_double(scale), C.c_double(shape),
            C.c_void_p(path_lengths.ctypes.data if path_lengths.size else None), C.c_void_p(out.ctypes.data if out.size else None)),
            "rpvg_hip_alignments_set_effective_lengths")
        return out

    def free(self):
        if self.handle:
            lib().rpvg_hip_alignments_free(self.ctx.handle, self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- fragment-length model (include/rpvg_frag.h) ------------------------------------
class CFragLengthFit(C.Structure):
    """rpvg_frag_length_fit"""
    _fields_ = [("loc", C.c_double), ("scale", C.c_double), ("shape", C.c_double), ("max_length", C.c_uint32),
                ("sample_size", C.c_uint32), ("iterations", C.c_uint32), ("evaluations", C.c_uint32), ("valid", C.c_int32)]


def frag_length_fit(ctx_handle, counts, skew_normal: bool = True) -> CFragLengthFit:
    """FragmentLengthDist(counts, skew_normal) on the GPU (one kernel launch)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    fit = CFragLengthFit()
    _check(lib().rpvg_hip_frag_length_fit(ctx_handle, C.c_void_p(counts.ctypes.data if counts.size else None), C.c_uint32(counts.size),
                                          C.c_int(1 if skew_normal else 0), C.byref(fit)), "rpvg_hip_frag_length_fit")
    return fit


def effective_lengths(ctx_handle, path_lengths, loc: float, scale: float, shape: float) -> np.ndarray:
    """PathsIndex::effectivePathLength for every path length, on the GPU."""
    path_lengths = np.ascontiguousarray(path_lengths, dtype=np.uint32)
    out = np.zeros(path_lengths.size, dtype=np.float64)
    _check(lib().rpvg_hip_effective_lengths(ctx_handle, C.c_double(loc), C.c_double(scale), C.c_double(shape),
                                            C.c_void_p(path_lengths.ctypes.data if path_lengths.size else None),
                                            C.c_uint64(path_lengths.size), C.c_void_p(out.ctypes.data if out.size else None)),
           "rpvg_hip_effective_lengths")
    return out


class DeviceFragTable:
    """logProb(v), v = 0 .. 65535, computed and resident on the GPU (rpvg_hip_frag_table)."""

    def __init__(self, ctx_handle, loc: float, scale: float, shape: float):
        self.ctx_handle = ctx_handle
        self.handle = C.c_void_p()
        _check(lib().rpvg_hip_frag_length_table(ctx_handle, C.c_double(loc), C.c_double(scale), C.c_double(shape), C.byref(self.handle)),
               "rpvg_hip_frag_length_table")

    def download(self) -> np.ndarray:
        out = np.zeros(65536, dtype=np.float64)
        _check(lib().rpvg_hip_frag_length_table_get(self.ctx_handle, self.handle, C.c_void_p(out.ctypes.data)),
               "rpvg_hip_frag_length_table_get")
        return out

    def free(self):
        if self.handle:
            lib().rpvg_hip_frag_length_table_free(self.ctx_handle, self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def host_register(array: np.ndarray):
    """Page-locks the memory of a numpy array (rpvg_hip_host_register): uploads from it skip the staging copy."""
    if array.nbytes:
        _check(lib().rpvg_hip_host_register(C.c_void_p(array.ctypes.data), C.c_uint64(array.nbytes)), "rpvg_hip_host_register")


def host_unregister(array: np.ndarray):
    if array.nbytes:
        _check(lib().rpvg_hip_host_unregister(C.c_void_p(array.ctypes.data)), "rpvg_hip_host_unregister")


class DeviceGroups:
    def __init__(self, ctx: "Context", batch: DeviceBatch, clusters: Sequence[int], groups: Sequence[Sequence[Sequence[int]]],
                 normalise: bool, collapse_precision: float = 0.0):
        """groups[m] = list of path lists (one per column) for matrix m on clusters[m]; collapse_precision > 0 replays
        readCollapseProbabilityMatrix on the (normalised) matrices."""
        self.ctx = ctx
        self.batch = batch
        cl = np.ascontiguousarray(clusters, dtype=np.uint32)
        host = batch.host  # (None: a batch made on the device — rows() needs the host's sizes)
        self._rows = [int(host.cluster_row_off[k + 1] - host.cluster_row_off[k]) for k in cl] if host is not None else None
        if groups is None:  # column c of a matrix = path c of its cluster alone: rpvg_hip_groups_build_single_paths
            self._cols = [int(host.cluster_path_off[k + 1] - host.cluster_path_off[k]) for k in cl] if host is not None else None
            self.handle = C.c_void_p()
            _check(lib().rpvg_hip_groups_build_single_paths(ctx.handle, batch.handle, C.c_uint32(len(cl)), C.c_void_p(cl.ctypes.data),
                                                            C.c_int32(1 if normalise else 0), C.c_double(float(collapse_precision)),
                                                            C.byref(self.handle)), "rpvg_hip_groups_build_single_paths")
            return
        self._cols = [len(cols) for cols in groups]
        goff, gpoff, gp = [0], [0], []
        for cols in groups:
            for paths in cols:
                gp.extend(paths)
                gpoff.append(len(gp))
            goff.append(len(gpoff) - 1)
        goff = np.ascontiguousarray(goff, dtype=np.uint64)
        gpoff = np.ascontiguousarray(gpoff, dtype=np.uint64)
        gp = np.ascontiguousarray(gp, dtype=np.uint32)
        spec = CGroupSpec(len(cl), cl.ctypes.data, goff.ctypes.data, gpoff.ctypes.data, gp.ctypes.data, 1 if normalise else 0,
                          float(collapse_precision))
        self.handle = C.c_void_p()
        _check(lib().rpvg_hip_groups_build(ctx.handle, batch.handle, C.byref(spec), C.byref(self.handle)),
               "rpvg_hip_groups_build")

    @classmethod
    def from_sources(cls, ctx: "Context", batch: DeviceBatch, clusters: Sequence[int], normalise: bool, collapse_precision: float = 0.0) -> "DeviceGroups":
        """rpvg_hip_groups_build_from_sources: the columns of matrix m are the haplotype columns the upload formed for clusters[m]
        (DeviceBatch.source_columns); their multiplicities stay on the device (bounded_pair_posteriors(None, ...)).  With a
        collapse_precision the last stage of the collapse is held back for the diploid search."""
        self = cls.__new__(cls)
        self.ctx, self.batch = ctx, batch
        cl = np.ascontiguousarray(clusters, dtype=np.uint32)
        self._rows = [int(batch.host.cluster_row_off[k + 1] - batch.host.cluster_row_off[k]) for k in cl]
        self._cols = [len(batch.source_columns(int(k))[0]) for k in cl]
        self.handle = C.c_void_p()
        _check(lib().rpvg_hip_groups_build_from_sources(ctx.handle, batch.handle, C.c_uint32(len(cl)), C.c_void_p(cl.ctypes.data),
                                                        C.c_int32(1 if normalise else 0), C.c_double(float(collapse_precision)),
                                                        C.byref(self.handle)), "rpvg_hip_groups_build_from_sources")
        return self

    def rows(self, m: int):
        """rpvg_hip_groups_rows (a test entry): matrix m as its readers see it behind the row collapse — (values [R, G], noise [R],
        row maxima [R], counts [R]), rows in the matrix's own order."""
        if self._rows is None or self._cols is None:
            raise EngineError("DeviceGroups.rows: the batch has no host copy to take the matrix's sizes from")
        R, G = self._rows[m], self._cols[m]
        values = np.zeros((G, R), dtype=np.float64)  # column-major on the device
        noise, rowmax, count = (np.zeros(R, dtype=np.float64) for _ in range(3))
        _check(lib().rpvg_hip_groups_rows(self.ctx.handle, self.handle, C.c_uint32(m), C.c_void_p(values.ctypes.data),
                                          C.c_void_p(noise.ctypes.data), C.c_void_p(rowmax.ctypes.data), C.c_void_p(count.ctypes.data)),
               "rpvg_hip_groups_rows")
        return np.ascontiguousarray(values.T), noise, rowmax, count

    def collapse_info(self):
        """(matrices whose runs were replayed, rows that took the values of their run head, matrices sorted as a
        whole, rows that took part in a replay)."""
        out = [C.c_uint32(0) for _ in range(4)]
        _check(lib().rpvg_hip_groups_collapse_info(self.ctx.handle, self.handle, *[C.byref(x) for x in out]),
               "rpvg_hip_groups_collapse_info")
        return tuple(int(x.value) for x in out)

    def loglik(self, matrix, members, divisor: float, add_rowmax=None) -> np.ndarray:
        mt = np.ascontiguousarray(matrix, dtype=np.uint32)
        mem = np.ascontiguousarray(members, dtype=np.uint32)
        if mem.ndim == 1:
            mem = mem.reshape(len(mt), -1)
        width = mem.shape[1]
        out = np.zeros(len(mt), dtype=np.float64)
        flag = None if add_rowmax is None else np.ascontiguousarray(add_rowmax, dtype=np.uint8)
        _check(lib().rpvg_hip_group_loglik(self.ctx.handle, self.handle, C.c_uint32(len(mt)), C.c_void_p(mt.ctypes.data),
                                           C.c_void_p(mem.ctypes.data), C.c_uint32(width), C.c_double(divisor),
                                           C.c_void_p(flag.ctypes.data if flag is not None else None),
                                           C.c_void_p(out.ctypes.data)), "rpvg_hip_group_loglik")
        return out

    def conditionals(self, matrix, others, width: int, divisor: float, num_cols) -> List[np.ndarray]:
        """Per request: log-likelihood of every candidate column given the other width-1 members."""
        mt = np.ascontiguousarray(matrix, dtype=np.uint32)
        oth = np.ascontiguousarray(others, dtype=np.uint32).reshape(len(mt), max(width - 1, 0))
        sizes = [int(num_cols[int(m)]) for m in mt]
        out = np.zeros(sum(sizes), dtype=np.float64)
        _check(lib().rpvg_hip_group_conditionals(self.ctx.handle, self.handle, C.c_uint32(len(mt)), C.c_void_p(mt.ctypes.data),
                                                 C.c_void_p(oth.ctypes.data if oth.size else None), C.c_uint32(width),
                                                 C.c_double(divisor), C.c_void_p(out.ctypes.data)),
               "rpvg_hip_group_conditionals")
        return np.split(out, np.cumsum(sizes)[:-1]) if sizes else []

    def full_posteriors(self, matrix, group_size: int, log_freq, num_cols) -> List[np.ndarray]:
        """rpvg_hip_group_full_posteriors: per problem, the posterior of every multiset of group_size columns of its matrix
        (num_cols[m] columns), in lexicographic order of the member lists; log_freq[q] = the log frequencies of problem q's
        columns."""
        mt = np.ascontiguousarray(matrix, dtype=np.uint32)
        lf = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64) for x in log_freq]) if len(log_freq) else np.zeros(0))
        sizes = [int(lib().rpvg_hip_full_set_count(C.c_uint32(int(num_cols[int(m)])), C.c_uint32(group_size))) for m in mt]
        out = np.zeros(sum(s for s in sizes if s <= 0x7fffffff), dtype=np.float64)
        _check(lib().rpvg_hip_group_full_posteriors(self.ctx.handle, self.handle, C.c_uint32(len(mt)), C.c_void_p(mt.ctypes.data),
                                                    C.c_uint32(group_size), C.c_void_p(lf.ctypes.data if lf.size else None),
                                                    C.c_void_p(out.ctypes.data if out.size else None)),
               "rpvg_hip_group_full_posteriors")
        return np.split(out, np.cumsum(sizes)[:-1]) if sizes else []

    def nested_full_subset_em(self, group_size: int, log_freq, min_hap_prob: float, max_em_its: int = 10000, max_rel_em_conv: float = 1e-3,
                              collapse_precision: float = 0.0, keep_handle: bool = False):
        """rpvg_hip_nested_full_subset_em on every matrix: full enumeration, retained sets, path subsets, EM and the weighted merge
        in one call (group sizes 1 and 3 .. 8).  log_freq[m] = the log frequencies of matrix m's columns.  Returns the fields of
        rpvg_hip_subset_em_sets_view as numpy arrays (copies; set_member and set_abundance as [slots, group_size]), plus
        num_matrices and group_size; with keep_handle (the view, the rpvg_hip_subset_em handle), which the caller frees with
        rpvg_hip_subset_em_free.  Raises EngineError; a refusal carries RPVG_HIP_ERR_UNSUPPORTED, "(-5)", and its reason."""
        lf = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64) for x in log_freq]) if len(log_freq) else np.zeros(0))
        h = C.c_void_p()
        _check(lib().rpvg_hip_nested_full_subset_em(self.ctx.handle, self.batch.handle, self.handle, C.c_uint32(group_size),
                                                    C.c_void_p(lf.ctypes.data if lf.size else None), C.c_double(float(min_hap_prob)),
                                                    C.c_uint32(max_em_its), C.c_double(float(max_rel_em_conv)),
                                                    C.c_double(float(collapse_precision)), C.byref(h)), "rpvg_hip_nested_full_subset_em")
        free_handle = not keep_handle
        try:
            v = CSubsetEmSetsView()
            _check(lib().rpvg_hip_subset_em_get_sets(h, C.byref(v)), "rpvg_hip_subset_em_get_sets")
            M, g = int(v.num_matrices), int(v.group_size)

            def take(pointer, n, dtype, shape=None):
                if n == 0 or not pointer:
                    return np.zeros(shape if shape is not None else (0,), dtype=dtype)
                a = np.ctypeslib.as_array(pointer, shape=(n,)).copy()
                return a.reshape(shape) if shape is not None else a

            out = {"num_matrices": M, "group_size": g}
            if M == 0:
                out.update({"subset_off": np.zeros(1, np.uint64), "path_off": np.zeros(1, np.uint64), "col_off": np.zeros(1, np.uint64),
                            "retained_off": np.zeros(1, np.uint64)})
                for name, dtype in (("weight", np.float64), ("path", np.uint32), ("col_path", np.uint32), ("abundances", np.float64),
                                    ("noise_count", np.float64), ("total_count", np.float64), ("iterations", np.uint32),
                                    ("retained_rank", np.uint64), ("retained_posterior", np.float64), ("set_count", np.uint32),
                                    ("cluster_noise_count", np.float64), ("set_size", np.uint32), ("set_posterior", np.float64)):
                    out[name] = np.zeros(0, dtype)
                out["set_member"] = np.zeros((0, g), np.uint32)
                out["set_abundance"] = np.zeros((0, g), np.float64)
                return (out, h) if keep_handle else out
            out["subset_off"] = take(v.subset_off, M + 1, np.uint64)
            S = int(out["subset_off"][-1])
            out["path_off"] = take(v.path_off, S + 1, np.uint64)
            out["col_off"] = take(v.col_off, S + 1, np.uint64)
            L, Cn = int(out["path_off"][-1]), int(out["col_off"][-1])
            out["weight"] = take(v.weight, S, np.float64)
            out["path"] = take(v.path, L, np.uint32)
            out["col_path"] = take(v.col_path, Cn, np.uint32)
            out["abundances"] = take(v.abundances, Cn, np.float64)
            out["noise_count"] = take(v.noise_count, S, np.float64)
            out["total_count"] = take(v.total_count, S, np.float64)
            out["iterations"] = take(v.iterations, S, np.uint32)
            out["retained_off"] = take(v.retained_off, M + 1, np.uint64)
            R = int(out["retained_off"][-1])
            out["retained_rank"] = take(v.retained_rank, R, np.uint64)
            out["retained_posterior"] = take(v.retained_posterior, R, np.float64)
            out["set_count"] = take(v.set_count, M, np.uint32)
            out["cluster_noise_count"] = take(v.cluster_noise_count, M, np.float64)
            out["set_size"] = take(v.set_size, L, np.uint32)
            out["set_member"] = take(v.set_member, L * g, np.uint32, (L, g))
            out["set_posterior"] = take(v.set_posterior, L, np.float64)
            out["set_abundance"] = take(v.set_abundance, L * g, np.float64, (L, g))
            return (out, h) if keep_handle else out
        except BaseException:
            free_handle = True
            raise
        finally:
            if free_handle:
                lib().rpvg_hip_subset_em_free(h)

    def nested_independent_subset_em(self, matrix_off, group_size: int, min_hap_prob: float, generator_words, column_counts=None, log_freq=None,
                                     max_em_its: int = 10000, max_rel_em_conv: float = 1e-3, collapse_precision: float = 0.0,
                                     keep_draws: bool = False, keep_handle: bool = False):
        """rpvg_hip_nested_independent_subset_em: unit k is the cluster whose transcripts are the matrices
        [matrix_off[k], matrix_off[k + 1]), one column per path.  column_counts (group size 2): the multiplicity of every column,
        matrices back to back; log_freq[m] (other group sizes): the log frequencies of matrix m's columns; generator_words: [K, 624]
        the next outputs of every cluster's std::mt19937.  Returns the fields of rpvg_hip_subset_em_independent_view as numpy arrays
        (copies; set_member and set_abundance as [slots, group_size]) and, with keep_draws, "draws": per unit an array
        [num_samples, transcripts]; with keep_handle (the view, the rpvg_hip_subset_em handle), which the caller frees with
        rpvg_hip_subset_em_free.  Raises EngineError; a refusal carries RPVG_HIP_ERR_UNSUPPORTED, "(-5)", and its reason."""
        mo = np.ascontiguousarray(matrix_off, dtype=np.uint32)
        K = len(mo) - 1
        gw = np.ascontiguousarray(generator_words, dtype=np.uint32).reshape(K, 624)
        cc = None if column_counts is None else np.ascontiguousarray(column_counts, dtype=np.uint32)
        lf = None
        if log_freq is not None:
            lf = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64) for x in log_freq]) if len(log_freq) else np.zeros(0))
        spec = CIndependentSpec(K, mo.ctypes.data, group_size, cc.ctypes.data if cc is not None and cc.size else None,
                                lf.ctypes.data if lf is not None and lf.size else None, float(min_hap_prob), max_em_its, float(max_rel_em_conv),
                                float(collapse_precision), gw.ctypes.data if gw.size else None, 1 if keep_draws else 0)
        h = C.c_void_p()
        _check(lib().rpvg_hip_nested_independent_subset_em(self.ctx.handle, self.batch.handle, self.handle, C.byref(spec), C.byref(h)),
               "rpvg_hip_nested_independent_subset_em")
        free_handle = not keep_handle
        try:
            v = CSubsetEmIndependentView()
            _check(lib().rpvg_hip_subset_em_get_independent(h, C.byref(v)), "rpvg_hip_subset_em_get_independent")
            g = int(v.group_size)

            def take(pointer, n, dtype, shape=None):
                if n == 0 or not pointer:
                    return np.zeros(shape if shape is not None else (0,), dtype=dtype)
                a = np.ctypeslib.as_array(pointer, shape=(n,)).copy()
                return a.reshape(shape) if shape is not None else a

            out = {"num_clusters": K, "group_size": g, "num_samples": int(v.num_samples)}
            out["subset_off"] = take(v.subset_off, K + 1, np.uint64) if K else np.zeros(1, np.uint64)
            S = int(out["subset_off"][-1])
            out["path_off"] = take(v.path_off, S + 1, np.uint64) if K else np.zeros(1, np.uint64)
            out["col_off"] = take(v.col_off, S + 1, np.uint64) if K else np.zeros(1, np.uint64)
            L, Cn = int(out["path_off"][-1]), int(out["col_off"][-1])
            out["weight"] = take(v.weight, S, np.float64)
            out["path"] = take(v.path, L, np.uint32)
            out["col_path"] = take(v.col_path, Cn, np.uint32)
            out["abundances"] = take(v.abundances, Cn, np.float64)
            out["noise_count"] = take(v.noise_count, S, np.float64)
            out["total_count"] = take(v.total_count, S, np.float64)
            out["iterations"] = take(v.iterations, S, np.uint32)
            out["set_count"] = take(v.set_count, K, np.uint32)
            out["cluster_noise_count"] = take(v.cluster_noise_count, K, np.float64)
            out["set_size"] = take(v.set_size, L, np.uint32)
            out["set_member"] = take(v.set_member, L * g, np.uint32, (L, g))
            out["set_posterior"] = take(v.set_posterior, L, np.float64)
            out["set_abundance"] = take(v.set_abundance, L * g, np.float64, (L, g))
            out["sample_count"] = take(v.sample_count, S, np.uint32)
            out["words_consumed"] = take(v.words_consumed, K, np.uint64)
            out["generator_state"] = take(v.generator_state, K * 624, np.uint32, (K, 624))
            if keep_draws:
                out["draws"] = []
                for k in range(K):
                    T = int(mo[k + 1]) - int(mo[k])
                    d = np.zeros(max(out["num_samples"] * T, 1), dtype=np.uint32)
                    _check(lib().rpvg_hip_independent_draws_get(h, C.c_uint32(k), C.c_void_p(d.ctypes.data)), "rpvg_hip_independent_draws_get")
                    out["draws"].append(d[:out["num_samples"] * T].reshape(out["num_samples"], T))
            return (out, h) if keep_handle else out
        except BaseException:
            free_handle = True
            raise
        finally:
            if free_handle:
                lib().rpvg_hip_subset_em_free(h)

    def gibbs(self, matrix, group_size: int, num_chains, num_burn_its, num_gibbs_its, log_freq, generator_problems, generator_words):
        """rpvg_hip_group_gibbs: per problem ([sorted member tuples in order of first appearance], counts); plus the words each
        generator gave, the state words of the generators that gave at least 624, and (rounds, conditionals)."""
        return self._gibbs("rpvg_hip_group_gibbs", matrix, group_size, num_chains, num_burn_its, num_gibbs_its, log_freq, generator_problems,
                           generator_words)

    def gibbs_polyploid(self, matrix, group_size: int, num_chains, num_burn_its, num_gibbs_its, log_freq, generator_problems, generator_words):
        """rpvg_hip_group_gibbs_polyploid (group sizes 3 .. 8): the arguments and the return shape of gibbs(), member tuples of
        length group_size."""
        return self._gibbs("rpvg_hip_group_gibbs_polyploid", matrix, group_size, num_chains, num_burn_its, num_gibbs_its, log_freq,
                           generator_problems, generator_words)

    def _gibbs(self, entry, matrix, group_size, num_chains, num_burn_its, num_gibbs_its, log_freq, generator_problems, generator_words):
        mt = np.ascontiguousarray(matrix, dtype=np.uint32)
        ch = np.ascontiguousarray(num_chains, dtype=np.uint32)
        bu = np.ascontiguousarray(num_burn_its, dtype=np.uint32)
        it = np.ascontiguousarray(num_gibbs_its, dtype=np.uint32)
        lf = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64) for x in log_freq]) if len(log_freq) else np.zeros(0))
        goff = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(g) for g in generator_problems])]), dtype=np.uint32)
        gp = np.ascontiguousarray([p for g in generator_problems for p in g], dtype=np.uint32)
        gw = np.ascontiguousarray(generator_words, dtype=np.uint32).reshape(len(generator_problems), 624)
        spec = CGibbsSpec(len(mt), group_size, mt.ctypes.data, ch.ctypes.data, bu.ctypes.data, it.ctypes.data, lf.ctypes.data,
                          len(generator_problems), goff.ctypes.data, gp.ctypes.data, gw.ctypes.data)
        h = C.c_void_p()
        _check(getattr(lib(), entry)(self.ctx.handle, self.handle, C.byref(spec), C.byref(h)), entry)
        try:
            v = CGibbsSetsView()
            _check(lib().rpvg_hip_gibbs_sets_get(h, C.byref(v)), "rpvg_hip_gibbs_sets_get")
            off = np.ctypeslib.as_array(v.set_off, shape=(len(mt) + 1,)).copy()
            total = int(off[-1])
            by_members = bool(v.members)
            if by_members:
                members = np.ctypeslib.as_array(v.members, shape=(total, group_size)).copy()
            else:
                first = np.ctypeslib.as_array(v.first, shape=(total,)).copy() if total else np.zeros(0, np.uint32)
                second = np.ctypeslib.as_array(v.second, shape=(total,)).copy() if total else np.zeros(0, np.uint32)
            count = np.ctypeslib.as_array(v.count, shape=(total,)).copy() if total else np.zeros(0, np.uint32)
            if len(generator_problems):
                words = np.ctypeslib.as_array(v.words_consumed, shape=(len(generator_problems),)).copy()
                state = np.ctypeslib.as_array(v.generator_state, shape=(len(generator_problems), 624)).copy()
            else:
                words, state = np.zeros(0, np.uint64), np.zeros((0, 624), np.uint32)
            out = []
            for i in range(len(mt)):
                a, b = int(off[i]), int(off[i + 1])
                if by_members:
                    sets = [tuple(int(x) for x in row) for row in members[a:b]]
                else:
                    sets = [(int(x),) if group_size == 1 else (int(x), int(y)) for x, y in zip(first[a:b], second[a:b])]
                out.append((sets, [int(c) for c in count[a:b]]))
            return out, words, state, (int(v.rounds), int(v.conditionals))
        finally:
            lib().rpvg_hip_gibbs_sets_free(h)

    def bounded_pair_posteriors(self, column_counts, min_rel_likelihood: float):
        """Per matrix: ([(first, second)...], posteriors) of the on-device branch-and-bound.  column_counts None: the
        multiplicities that matrices built from_sources carry."""
        cc = None if column_counts is None else np.ascontiguousarray(column_counts, dtype=np.uint32)
        h = C.c_void_p()
        _check(lib().rpvg_hip_bounded_pair_posteriors(self.ctx.handle, self.handle, C.c_void_p(cc.ctypes.data if cc is not None else None),
                                                      C.c_double(min_rel_likelihood), C.byref(h)),
               "rpvg_hip_bounded_pair_posteriors")
        try:
            v = CPairPosteriorsView()
            _check(lib().rpvg_hip_pair_posteriors_get(h, C.byref(v)), "rpvg_hip_pair_posteriors_get")
            M = v.num_matrices
            off = np.ctypeslib.as_array(v.pair_off, shape=(M + 1,)).astype(np.int64)
            n = int(off[-1])
            first = np.ctypeslib.as_array(v.first, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
            second = np.ctypeslib.as_array(v.second, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
            post = np.ctypeslib.as_array(v.posterior, shape=(n,)).copy() if n else np.zeros(0)
        finally:
            lib().rpvg_hip_pair_posteriors_free(h)
        return [([(int(a), int(b)) for a, b in zip(first[off[m]:off[m + 1]], second[off[m]:off[m + 1]])],
                 post[off[m]:off[m + 1]]) for m in range(M)]

    def free(self):
        if self.handle:
            lib().rpvg_hip_groups_free(self.ctx.handle, self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One GPU + one HIP stream (rpvg_hip_ctx)."""

    def __init__(self, device: int = 0):
        self.handle = C.c_void_p()
        _check(lib().rpvg_hip_create(C.c_int(device), C.byref(self.handle)), "rpvg_hip_create")

    def close(self):
        if self.handle:
            lib().rpvg_hip_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> Tuple[str, int, int]:
        name = C.create_string_buffer(256)
        cus, mem = C.c_uint32(0), C.c_uint64(0)
        _check(lib().rpvg_hip_device_info(self.handle, name, 256, C.byref(cus), C.byref(mem)), "rpvg_hip_device_info")
        return name.value.decode(), cus.value, mem.value

    def synchronize(self):
        _check(lib().rpvg_hip_synchronize(self.handle), "rpvg_hip_synchronize")

    def upload(self, host: ClusterBatch, compact: bool = False, narrow: bool = False) -> DeviceBatch:
        """compact / narrow: the forms of the batch's arrays made for the copy (ClusterBatch.as_c)."""
        return DeviceBatch(self, host, compact, narrow=narrow)

    def upload_segments(self, host: ClusterBatch, segments: PinnedSegments) -> DeviceBatch:
        """The batch from one page-locked segment per cluster (rpvg_hip_batch_upload_segments)."""
        return DeviceBatch(self, host, segments=segments)

    def groups(self, batch: DeviceBatch, clusters, groups, normalise: bool, collapse_precision: float = 0.0) -> DeviceGroups:
        return DeviceGroups(self, batch, clusters, groups, normalise, collapse_precision)

    # ---- EM -----------------------------------------------------------------
    def em_solve(self, batch: DeviceBatch, clusters: Sequence[int], columns: Sequence[Sequence[int]],
                 max_em_its: int = 10000, max_rel_em_conv: float = 1e-3, collapse_precision: float = 0.0):
        """Returns (abundances list per problem, noise_count[P], total_count[P], iterations[P])."""
        P = len(clusters)
        cl = np.ascontiguousarray(clusters, dtype=np.uint32)
        col_off = np.zeros(P + 1, dtype=np.uint64)
        col_off[1:] = np.cumsum([len(c) for c in columns])
        col_path = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint32) for c in columns])
                                        if P else np.zeros(0), dtype=np.uint32)
        abund = np.zeros(int(col_off[-1]), dtype=np.float64)
        noise = np.zeros(P, dtype=np.float64)
        total = np.zeros(P, dtype=np.float64)
        iters = np.zeros(P, dtype=np.uint32)
        probs = CEmProblems(P, cl.ctypes.data, col_off.ctypes.data, col_path.ctypes.data, collapse_precision)
        res = CEmResults(abund.ctypes.data, noise.ctypes.data, total.ctypes.data, iters.ctypes.data)
        _check(lib().rpvg_hip_em_solve(self.handle, batch.handle, C.c_uint32(max_em_its), C.c_double(max_rel_em_conv),
                                       C.byref(probs), C.byref(res)), "rpvg_hip_em_solve")
        off = col_off.astype(np.int64)
        return [abund[off[p]:off[p + 1]] for p in range(P)], noise, total, iters

    def gibbs_read_counts(self, batch: DeviceBatch, clusters: Sequence[int], columns: Sequence[Sequence[int]], init_abundances,
                          init_noise_count, num_samples, seeds, thin: int, gamma: float = 1.0):
        """rpvg_hip_gibbs_read_counts: per problem (noise samples [n], abundance samples [n x columns]), starting from
        init_abundances[p] (expected read counts per column) and init_noise_count[p]."""
        P = len(clusters)
        cl = np.ascontiguousarray(clusters, dtype=np.uint32)
        col_off = np.zeros(P + 1, dtype=np.uint64)
        col_off[1:] = np.cumsum([len(c) for c in columns])
        col_path = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint32) for c in columns])
                                        if P else np.zeros(0), dtype=np.uint32)
        init = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64) for a in init_abundances])
                                    if P else np.zeros(0), dtype=np.float64)
        assert init.size == int(col_off[-1])
        init_noise = np.ascontiguousarray(init_noise_count, dtype=np.float64)
        n = np.ascontiguousarray(num_samples, dtype=np.uint32)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert init_noise.size == n.size == sd.size == P
        widths = np.diff(col_off.astype(np.int64))
        noise = np.zeros(int(n.sum()), dtype=np.float64)
        abund = np.zeros(int((n.astype(np.int64) * widths).sum()), dtype=np.float64)
        probs = CEmProblems(P, cl.ctypes.data, col_off.ctypes.data, col_path.ctypes.data, 0.0)
        _check(lib().rpvg_hip_gibbs_read_counts(self.handle, batch.handle, C.byref(probs), C.c_void_p(init.ctypes.data),
                                                C.c_void_p(init_noise.ctypes.data), C.c_void_p(n.ctypes.data), C.c_void_p(sd.ctypes.data),
                                                C.c_uint32(thin), C.c_double(gamma), C.c_void_p(noise.ctypes.data),
                                                C.c_void_p(abund.ctypes.data)), "rpvg_hip_gibbs_read_counts")
        out, at_n, at_a = [], 0, 0
        for p in range(P):
            k, w = int(n[p]), int(widths[p])
            out.append((noise[at_n:at_n + k], abund[at_a:at_a + k * w].reshape(k, w)))
            at_n, at_a = at_n + k, at_a + k * w
        return out

    def min_path_cover(self, batch: DeviceBatch, clusters: Sequence[int], extra: Optional[Sequence[int]] = None) -> List[List[int]]:
        """The ascending cover of every listed cluster; extra[i]: cells of listing i's output range beyond the cluster's paths."""
        cl = np.ascontiguousarray(clusters, dtype=np.uint32)
        n_paths = [int(batch.host.cluster_path_off[k + 1] - batch.host.cluster_path_off[k]) for k in clusters]
        off = np.zeros(len(cl) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(n_paths if extra is None else [n + int(x) for n, x in zip(n_paths, extra)])
        cover = np.zeros(int(off[-1]), dtype=np.uint32)
        size = np.zeros(len(cl), dtype=np.uint32)
        _check(lib().rpvg_hip_min_path_cover(self.handle, batch.handle, C.c_uint32(len(cl)), C.c_void_p(cl.ctypes.data),
                                             C.c_void_p(off.ctypes.data), C.c_void_p(cover.ctypes.data),
                                             C.c_void_p(size.ctypes.data)), "rpvg_hip_min_path_cover")
        return [[int(x) for x in cover[int(off[i]):int(off[i]) + int(size[i])]] for i in range(len(cl))]

    def segment_sort_words(self, words, segment_off) -> np.ndarray:
        """rpvg_hip_segment_sort_words: every segment words[segment_off[s]:segment_off[s + 1]] in ascending order, by the segment
        sort of the row collapse (a test entry: the words of a segment distinct and below 2^64 - 1)."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        off = np.ascontiguousarray(segment_off, dtype=np.uint64)
        assert len(off) >= 1 and int(off[-1]) == len(w)
        out = np.zeros(len(w), dtype=np.uint64)
        _check(lib().rpvg_hip_segment_sort_words(self.handle, C.c_void_p(w.ctypes.data), C.c_void_p(off.ctypes.data),
                                                 C.c_uint32(len(off) - 1), C.c_void_p(out.ctypes.data)), "rpvg_hip_segment_sort_words")
        return out

    def min_path_cover_any(self, batch: DeviceBatch, clusters: Sequence[int], extra: Optional[Sequence[int]] = None, grid_min_work: int = 0,
                           order: bool = False):
        """rpvg_hip_min_path_cover_any: the covers of clusters of any size, each on the route cover_limits() and grid_min_work give it
        (0: the library default, 1: every cluster of two paths and more over the whole GPU, GRID_NEVER: width only).  With order=True
        also, per listing, the paths in the order the rounds chose them — None for a cluster of the workgroup route."""
        cl = np.ascontiguousarray(clusters, dtype=np.uint32)
        n_paths = [int(batch.host.cluster_path_off[k + 1] - batch.host.cluster_path_off[k]) for k in clusters]
        off = np.zeros(len(cl) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(n_paths if extra is None else [n + int(x) for n, x in zip(n_paths, extra)])
        cover = np.zeros(int(off[-1]), dtype=np.uint32)
        chosen = np.zeros(int(off[-1]), dtype=np.uint32)
        size = np.zeros(len(cl), dtype=np.uint32)
        _check(lib().rpvg_hip_min_path_cover_any(self.handle, batch.handle, C.c_uint32(len(cl)), C.c_void_p(cl.ctypes.data),
                                                 C.c_void_p(off.ctypes.data), C.c_void_p(cover.ctypes.data), C.c_void_p(size.ctypes.data),
                                                 C.c_uint64(grid_min_work), C.c_void_p(chosen.ctypes.data if order else None)),
               "rpvg_hip_min_path_cover_any")
        covers = [[int(x) for x in cover[int(off[i]):int(off[i]) + int(size[i])]] for i in range(len(cl))]
        if not order:
            return covers
        orders = [None if n_paths[i] and int(chosen[int(off[i])]) == 0xFFFFFFFF else [int(x) for x in chosen[int(off[i]):int(off[i]) + int(size[i])]]
                  for i in range(len(cl))]
        return covers, orders

    # ---- dense ----------------------------------------------------------------
    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _check(lib().rpvg_hip_malloc(self.handle, C.c_uint64(nbytes), C.byref(p)), "rpvg_hip_malloc")
        return p.value

    def free(self, ptr: int):
        _check(lib().rpvg_hip_free(self.handle, C.c_void_p(ptr)), "rpvg_hip_free")

    def h2d(self, dst: int, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        _check(lib().rpvg_hip_memcpy_h2d(self.handle, C.c_void_p(dst), C.c_void_p(a.ctypes.data), C.c_uint64(a.nbytes)),
               "rpvg_hip_memcpy_h2d")

    def d2h(self, src: int, shape, dtype=np.float64) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        _check(lib().rpvg_hip_memcpy_d2h(self.handle, C.c_void_p(out.ctypes.data), C.c_void_p(src), C.c_uint64(out.nbytes)),
               "rpvg_hip_memcpy_d2h")
        return out

    def em_dense(self, d_matrix: int, R: int, Cn: int, ld: int, d_counts: int, total: float, max_em_its: int = 10000,
                 max_rel_em_conv: float = 1e-3, sharded: bool = False):
        """EM on a resident dense matrix.  sharded=True: the R rows are this rank's share of one cluster spread
        over the ranks of the context's communicator (comm_init) and `total` is the whole cluster's read count."""
        ab = np.zeros(Cn - 1, dtype=np.float64)
        noise = C.c_double(0)
        its = C.c_uint32(0)
        fn, name = ((lib().rpvg_hip_em_dense_sharded, "rpvg_hip_em_dense_sharded") if sharded
                    else (lib().rpvg_hip_em_dense, "rpvg_hip_em_dense"))
        _check(fn(self.handle, C.c_void_p(d_matrix), C.c_uint64(R), C.c_uint32(Cn), C.c_uint64(ld),
                  C.c_void_p(d_counts), C.c_double(total), C.c_uint32(max_em_its),
                  C.c_double(max_rel_em_conv), C.c_void_p(ab.ctypes.data), C.byref(noise),
                  C.byref(its)), name)
        return ab, noise.value, its.value

    # ---- communicator (RCCL) ----------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        _check(lib().rpvg_hip_comm_unique_id(buf), "rpvg_hip_comm_unique_id")
        return bytes(buf)

    def comm_init(self, unique_id: bytes, world_size: int, rank: int):
        assert len(unique_id) == COMM_ID_BYTES
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(lib().rpvg_hip_comm_init(self.handle, buf, C.c_int(world_size), C.c_int(rank)), "rpvg_hip_comm_init")

    def comm_destroy(self):
        _check(lib().rpvg_hip_comm_destroy(self.handle), "rpvg_hip_comm_destroy")

    def comm_init_all(self):
        """A communicator over the contexts of this process (rpvg_hip_comm_init_all) — here: this one context."""
        arr = (C.c_void_p * 1)(self.handle)
        _check(lib().rpvg_hip_comm_init_all(arr, C.c_int(1)), "rpvg_hip_comm_init_all")

    def gather(self, local: np.ndarray, counts) -> np.ndarray:
        """rpvg_hip_gather: this rank's values in, the values of all ranks (counts[r] each) out."""
        local = np.ascontiguousarray(local, dtype=np.float64)
        cnt = np.ascontiguousarray(counts, dtype=np.uint64)
        out = np.zeros(int(cnt.sum()), dtype=np.float64)
        _check(lib().rpvg_hip_gather(self.handle, C.c_void_p(local.ctypes.data), C.c_uint64(local.size), C.c_void_p(cnt.ctypes.data),
                                     C.c_void_p(out.ctypes.data)), "rpvg_hip_gather")
        return out

    def allreduce_sum_f64(self, d_buf: int, n: int):
        _check(lib().rpvg_hip_comm_allreduce_sum_f64(self.handle, C.c_void_p(d_buf), C.c_uint64(n)),
               "rpvg_hip_comm_allreduce_sum_f64")

    def dense_from_cluster(self, batch: DeviceBatch, cluster: int, d_matrix: int, ld: int, d_counts: int) -> float:
        total = C.c_double(0)
        _check(lib().rpvg_hip_dense_from_cluster(self.handle, batch.handle, C.c_uint32(cluster), C.c_void_p(d_matrix),
                                                 C.c_uint64(ld), C.c_void_p(d_counts), C.byref(total)),
               "rpvg_hip_dense_from_cluster")
        return total.value

    def synth_dense_cluster(self, seed: int, R: int, N: int, d_matrix: int, ld: int, d_counts: int):
        _check(lib().rpvg_hip_synth_dense_cluster(self.handle, C.c_uint64(seed), C.c_uint64(R), C.c_uint32(N),
                                                  C.c_void_p(d_matrix), C.c_uint64(ld), C.c_void_p(d_counts)),
               "rpvg_hip_synth_dense_cluster")

    def synth_dense_rows(self, seed: int, row_begin: int, R: int, N: int, d_matrix: int, ld: int, d_counts: int):
        """Rows [row_begin, row_begin + R) of the synthetic dense cluster `seed` (a rank's shard)."""
        _check(lib().rpvg_hip_synth_dense_rows(self.handle, C.c_uint64(seed), C.c_uint64(row_begin), C.c_uint64(R),
                                               C.c_uint32(N), C.c_void_p(d_matrix), C.c_uint64(ld), C.c_void_p(d_counts)),
               "rpvg_hip_synth_dense_rows")

    # ---- row construction (include/rpvg_rows.h) ------------------------------------
    def upload_alignments(self, align_batch) -> "DeviceAlignments":
        return DeviceAlignments(self, align_batch)

    def build_rows(self, align_batch, row_params, merge: bool = True):
        """addPathProbs for every read (+ sort / merge) on the GPU -> (ClusterBatch of rows, build_ms, merge_ms).
        align_batch: an AlignmentBatch (uploaded for this call) or DeviceAlignments (already resident)."""
        dev = align_batch if isinstance(align_batch, DeviceAlignments) else DeviceAlignments(self, align_batch)
        try:
            rows = dev.build_rows(row_params, merge)
            try:
                return rows.download()
            finally:
                rows.free()
        finally:
            if dev is not align_batch:
                dev.free()

    # ---- fragment-length model (include/rpvg_frag.h) ---------------------------------
    def frag_length_fit(self, counts, skew_normal: bool = True) -> CFragLengthFit:
        return frag_length_fit(self.handle, counts, skew_normal)

    def frag_length_table(self, loc: float, scale: float, shape: float) -> DeviceFragTable:
        return DeviceFragTable(self.handle, loc, scale, shape)

    def effective_lengths(self, path_lengths, loc: float, scale: float, shape: float) -> np.ndarray:
        return effective_lengths(self.handle, path_lengths, loc, scale, shape)

    def frag_length_eval(self, what: str, rows) -> np.ndarray:
        """what = "cdf": rows (x, m, s, a); "truncated_mean": (m, s, a, c, d); "owens_t": (h, a) -> one double per row."""
        kind = {"cdf": 0, "truncated_mean": 1, "owens_t": 2}[what]
        rows = np.asarray(rows, dtype=np.float64)
        padded = np.zeros((rows.shape[0], 5), dtype=np.float64)
        padded[:, :rows.shape[1]] = rows
        out = np.zeros(rows.shape[0], dtype=np.float64)
        _check(lib().rpvg_hip_frag_length_eval(self.handle, C.c_int(kind), C.c_void_p(padded.ctypes.data), C.c_uint64(rows.shape[0]),
                                               C.c_void_p(out.ctypes.data)), "rpvg_hip_frag_length_eval")
        return out

    # ---- path clustering ----------------------------------------------------------
    def path_clusters(self, num_paths: int, sets):
        """sets: id sets (lists of path ids) -> (path_to_cluster[num_paths], [members of cluster 0, 1, ...])."""
        off = np.zeros(len(sets) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in sets])
        flat = np.ascontiguousarray([p for x in sets for p in x], dtype=np.uint32)
        return self.path_clusters_flat(num_paths, off, flat)

    def path_clusters_flat(self, num_paths: int, set_off: np.ndarray, set_path: np.ndarray):
        set_off = np.ascontiguousarray(set_off, dtype=np.uint64)
        set_path = np.ascontiguousarray(set_path, dtype=np.uint32)
        p2c = np.zeros(max(num_paths, 1), dtype=np.uint32)
        coff = np.zeros(num_paths + 1, dtype=np.uint64)
        cpaths = np.zeros(max(num_paths, 1), dtype=np.uint32)
        nc = C.c_uint32(0)
        _check(lib().rpvg_hip_path_clusters(self.handle, C.c_uint32(num_paths), C.c_uint64(len(set_off) - 1),
                                            C.c_void_p(set_off.ctypes.data), C.c_void_p(set_path.ctypes.data if set_path.size else None),
                                            C.c_void_p(p2c.ctypes.data), C.byref(nc), C.c_void_p(coff.ctypes.data),
                                            C.c_void_p(cpaths.ctypes.data)), "rpvg_hip_path_clusters")
        k = nc.value
        members = [cpaths[int(coff[c]):int(coff[c + 1])].tolist() for c in range(k)]
        return p2c[:num_paths].copy(), members

    def debug_log(self, x: np.ndarray, use_table: bool = True) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros_like(x)
        _check(lib().rpvg_hip_debug_log(self.handle, C.c_uint64(x.size), C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data),
                                        C.c_int32(1 if use_table else 0)), "rpvg_hip_debug_log")
        return out

    # ---- stats ----------------------------------------------------------------
    def stats(self) -> dict:
        s = CKernelStats()
        _check(lib().rpvg_hip_stats_get(self.handle, C.byref(s)), "rpvg_hip_stats_get")
        return s.as_dict()

    def independent_stats(self) -> dict:
        """rpvg_hip_independent_stats: calls of rpvg_hip_nested_independent_subset_em that completed, their draws and subsets."""
        s = CIndependentStats()
        _check(lib().rpvg_hip_independent_stats_get(self.handle, C.byref(s)), "rpvg_hip_independent_stats_get")
        return {n: int(getattr(s, n)) for n, _ in s._fields_}

    def parse_stats(self) -> dict:
        """rpvg_hip_parse_stats: parses of a --write-probs text that completed, and the numbers the exact comparison decided."""
        s = CParseStats()
        _check(lib().rpvg_hip_parse_stats_get(self.handle, C.byref(s)), "rpvg_hip_parse_stats_get")
        return {n: int(getattr(s, n)) for n, _ in s._fields_}

    def reset_stats(self):
        _check(lib().rpvg_hip_stats_reset(self.handle), "rpvg_hip_stats_reset")
