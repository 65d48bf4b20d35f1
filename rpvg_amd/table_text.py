"""The rows of a result file as text, formatted on the GPU from a resident table (include/rpvg_text.h, rpvg_amd/csrc/table_text.hip):
the rows ReadCountGibbsSamplesWriter, AbundanceEstimatesWriter and HaplotypeAbundanceEstimatesWriter print, every double as glibc's
"%.*g" writes it, byte for byte.  The header row and the `Unknown` row stay with the host writers.

  Labels      the names, lengths and ClusterIDs of a batch's paths in the flat form of rpvg_table_labels, host arrays
  RowsInput   the rows of a batch and the path side of the --write-probs dump in the flat form of rpvg_rows_text_input
  TableText   over the C ABI (a hip.Context or an engine.Engine): gibbs / estimates / sets / rows / resident_rows / view / bytes /
              guards_intact / free; rows: the --write-probs dump (rpvg_amd/csrc/rows_text.hip), whose rows are the lines of the file;
              bgzf: the text as the members of a .gz file, deflated on the GPU (rpvg_amd/csrc/text_deflate.hip)
  BgzfText    BGZF members resident on the GPU (rpvg_hip_text_bgzf): view / bytes / guards_intact / free; bgzf_bytes(ctx, data)
              makes one of any bytes, bgzf_model(data) the same members on the host without a GPU
  parse_rows  the way back: the text of a --write-probs dump parsed on the GPU (rpvg_amd/csrc/rows_parse.hip) into a ParsedDump —
              resident rows (rows / to_batch), the path side (view) and device labels (labels); TableText.parse() does it for a
              resident text where it lies.  host_line_parse(data) is readProbabilityClusters flattened to the same arrays and
              plan_parse(data) the kernels' functions on the host; neither needs a GPU
  HarnessTableText  over the harness entry points: the text of a HarnessGibbsTable or a HarnessTable through the host class
              (rpvg_amd/host/table_text.hpp), the file from it by the writer's addText(), and the same rows from one host thread
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import hip
from ._flat import FlatArrays, HandleOwner, ctx_handle

PER_PATH, HAPLOTYPE = 0, 1  # RPVG_TEXT_PER_PATH, RPVG_TEXT_HAPLOTYPE
JOINT, POSTERIOR = 2, 3     # RPVG_TEXT_JOINT, RPVG_TEXT_POSTERIOR: a row per path group set (TableText.sets)
ROWS = 4                    # HarnessTableText only: the --write-probs dump of a prepared batch's rows (TableText.rows)


class CTableLabels(C.Structure):
    """rpvg_table_labels"""
    _fields_ = [("num_clusters", C.c_uint32), ("num_paths", C.c_uint64), ("num_name_bytes", C.c_uint64), ("name_off", C.c_void_p),
                ("name_bytes", C.c_void_p), ("path_length", C.c_void_p), ("cluster_id", C.c_void_p), ("on_device", C.c_int32)]


class CTableTextView(C.Structure):
    """rpvg_table_text_view"""
    _fields_ = [("num_paths", C.c_uint64), ("num_rows", C.c_uint64), ("num_bytes", C.c_uint64), ("row_off", C.POINTER(C.c_uint64)),
                ("bytes", C.POINTER(C.c_char))]


class CTextBgzfView(C.Structure):
    """rpvg_text_bgzf_view"""
    _fields_ = [("num_members", C.c_uint64), ("num_text_bytes", C.c_uint64), ("num_bytes", C.c_uint64), ("num_stored_members", C.c_uint64),
                ("member_off", C.POINTER(C.c_uint64)), ("bytes", C.POINTER(C.c_char))]


CHUNK_BYTES = 65280  # the text of member i starts at byte i * CHUNK_BYTES


def _bgzf_view_dict(v) -> dict:
    M, n = int(v.num_members), int(v.num_bytes)
    return dict(num_members=M, num_text_bytes=int(v.num_text_bytes), num_bytes=n, num_stored_members=int(v.num_stored_members),
                member_off=np.ctypeslib.as_array(v.member_off, shape=(M + 1,)).copy(), bytes=C.string_at(v.bytes, n) if n else b"")


class CRowsTextInput(C.Structure):
    """rpvg_rows_text_input"""
    _fields_ = [("num_clusters", C.c_uint32), ("num_rows", C.c_uint64), ("num_groups", C.c_uint64), ("num_entries", C.c_uint64), ("num_paths", C.c_uint64),
                ("cluster_row_off", C.c_void_p), ("cluster_path_off", C.c_void_p), ("row_count", C.c_void_p), ("row_noise", C.c_void_p),
                ("row_grp_off", C.c_void_p), ("grp_prob", C.c_void_p), ("grp_idx_off", C.c_void_p), ("path_idx", C.c_void_p),
                ("path_effective_length", C.c_void_p), ("num_align_lists", C.c_void_p), ("cluster_index", C.c_void_p), ("on_device", C.c_int32)]


_LABEL_FIELDS = (("name_off", np.uint64), ("name_bytes", np.uint8), ("path_length", np.uint32), ("cluster_id", np.uint32))


@dataclass
class Labels(FlatArrays):
    """TableLabels of rpvg_amd/host/io/estimates_writers.hpp, flat.  path_length may be empty for the Gibbs file."""
    name_off: np.ndarray
    name_bytes: np.ndarray
    path_length: np.ndarray
    cluster_id: np.ndarray
    _FIELDS, _C_STRUCT = _LABEL_FIELDS, CTableLabels

    @staticmethod
    def of(names: Sequence, cluster_ids: Sequence[int], lengths: Optional[Sequence[int]] = None) -> "Labels":
        """names: one str or bytes per path; cluster_ids: one per cluster; lengths: one per path, or None."""
        raw = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        off = np.zeros(len(raw) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(n) for n in raw])
        return Labels(off, np.frombuffer(b"".join(raw), dtype=np.uint8), [] if lengths is None else lengths, cluster_ids)

    def sizes(self) -> dict:
        return dict(num_clusters=len(self.cluster_id), num_paths=max(len(self.name_off) - 1, 0), num_name_bytes=len(self.name_bytes))


_ROWS_FIELDS = (("cluster_row_off", np.uint64), ("cluster_path_off", np.uint64), ("row_count", np.uint32), ("row_noise", np.float64),
                ("row_grp_off", np.uint64), ("grp_prob", np.float64), ("grp_idx_off", np.uint64), ("path_idx", np.uint32),
                ("path_effective_length", np.float64), ("num_align_lists", np.uint64), ("cluster_index", np.uint64))


@dataclass
class RowsInput(FlatArrays):
    """rpvg_rows_text_input: the row fields of a ClusterBatch with 64-bit offsets, the effective lengths of the paths and the rank
    keys of the clusters (both empty: bare "#" markers)."""
    cluster_row_off: np.ndarray
    cluster_path_off: np.ndarray
    row_count: np.ndarray
    row_noise: np.ndarray
    row_grp_off: np.ndarray
    grp_prob: np.ndarray
    grp_idx_off: np.ndarray
    path_idx: np.ndarray
    path_effective_length: np.ndarray
    num_align_lists: np.ndarray
    cluster_index: np.ndarray
    _FIELDS, _C_STRUCT = _ROWS_FIELDS, CRowsTextInput

    @staticmethod
    def of(batch, effective_lengths, num_align_lists=None, cluster_index=None) -> "RowsInput":
        """batch: anything with the row arrays of a ClusterBatch as attributes or keys."""
        get = (lambda n: batch[n]) if isinstance(batch, dict) else (lambda n: getattr(batch, n))
        return RowsInput(*[get(n) for n, _ in _ROWS_FIELDS[:8]], effective_lengths, [] if num_align_lists is None else num_align_lists,
                         [] if cluster_index is None else cluster_index)

    def sizes(self) -> dict:
        return dict(num_clusters=max(len(self.cluster_row_off) - 1, 0), num_rows=len(self.row_count), num_groups=len(self.grp_prob),
                    num_entries=len(self.path_idx), num_paths=len(self.path_effective_length))


class TableText(HandleOwner):
    """A text resident on the GPU (rpvg_hip_table_text)."""

    def __init__(self, handle):
        self.handle = handle

    @classmethod
    def gibbs(cls, ctx_or_engine, table, labels, precision: int = 8) -> "TableText":
        """table: a gibbs_table.GibbsTable; labels: Labels, or a CTableLabels (host or device pointers)."""
        handle = C.c_void_p()
        flat = labels.as_c() if isinstance(labels, Labels) else labels
        hip._check(hip.lib().rpvg_hip_gibbs_table_text(ctx_handle(ctx_or_engine), table.handle, C.byref(flat), C.c_int32(precision), C.byref(handle)),
                   "rpvg_hip_gibbs_table_text")
        return cls(handle)

    @classmethod
    def estimates(cls, ctx_or_engine, table, estimates_flat, labels, kind: int, precision: int = 8) -> "TableText":
        """table: an estimates_table.EstimatesTable with TPMs; estimates_flat: the CEstimatesFlat it was built from."""
        handle = C.c_void_p()
        flat = labels.as_c() if isinstance(labels, Labels) else labels
        hip._check(hip.lib().rpvg_hip_estimates_table_text(ctx_handle(ctx_or_engine), table.handle, C.byref(estimates_flat), C.byref(flat), C.c_int32(kind),
                                                          C.c_int32(precision), C.byref(handle)), "rpvg_hip_estimates_table_text")
        return cls(handle)

    @classmethod
    def sets(cls, ctx_or_engine, table, estimates_flat, labels, kind: int, ploidy: int, min_posterior: float, precision: int = 8) -> "TableText":
        """A row per path group set.  JOINT: the rows of JointHaplotypeAbundanceEstimatesWriter, from a table with TPMs built for
        `ploidy`; POSTERIOR: those of JointHaplotypeEstimatesWriter, which read neither abundances nor TPMs.  A set is printed iff
        not (posterior < min_posterior).  In the view the rows are the sets: row_off has num_sets + 1 entries."""
        handle = C.c_void_p()
        flat = labels.as_c() if isinstance(labels, Labels) else labels
        hip._check(hip.lib().rpvg_hip_estimates_set_text(ctx_handle(ctx_or_engine), table.handle, C.byref(estimates_flat), C.byref(flat), C.c_int32(kind),
                                                        C.c_uint32(ploidy), C.c_double(min_posterior), C.c_int32(precision), C.byref(handle)),
                   "rpvg_hip_estimates_set_text")
        return cls(handle)

    @classmethod
    def rows(cls, ctx_or_engine, rows_input, labels, prob_precision: float = 1e-8) -> "TableText":
        """The --write-probs dump: marker, path line and row lines of every cluster that has paths and rows.  rows_input: a RowsInput,
        or a CRowsTextInput (host or device pointers); labels need path_length.  In the view the rows are the LINES of the text:
        row_off has 2 K + R + 1 entries."""
        handle = C.c_void_p()
        flat = labels.as_c() if isinstance(labels, Labels) else labels
        inp = rows_input.as_c() if isinstance(rows_input, RowsInput) else rows_input
        hip._check(hip.lib().rpvg_hip_rows_text(ctx_handle(ctx_or_engine), C.byref(inp), C.byref(flat), C.c_double(prob_precision), C.byref(handle)),
                   "rpvg_hip_rows_text")
        return cls(handle)

    @classmethod
    def resident_rows(cls, ctx_or_engine, rows_handle, labels, effective_lengths, prob_precision: float = 1e-8, num_align_lists=None,
                      cluster_index=None) -> "TableText":
        """The same from a rpvg_hip_read_rows handle, read where it lies (hip.DeviceRows.text)."""
        handle = C.c_void_p()
        flat = labels.as_c() if isinstance(labels, Labels) else labels
        eff = np.ascontiguousarray(effective_lengths, dtype=np.float64)
        keys = [None if a is None else np.ascontiguousarray(a, dtype=np.uint64) for a in (num_align_lists, cluster_index)]
        pointers = [C.c_void_p(a.ctypes.data if a is not None and a.size else None) for a in [eff] + keys]
        hip._check(hip.lib().rpvg_hip_read_rows_text(ctx_handle(ctx_or_engine), rows_handle, C.byref(flat), *pointers, C.c_double(prob_precision),
                                                    C.byref(handle)), "rpvg_hip_read_rows_text")
        return cls(handle)

    def view(self) -> dict:
        """row_off [P + 1], the text as bytes (copied out of the page-locked block), num_rows (printed)."""
        v = CTableTextView()
        hip._check(hip.lib().rpvg_hip_table_text_view(self.handle, C.byref(v)), "rpvg_hip_table_text_view")
        P, n = int(v.num_paths), int(v.num_bytes)
        return dict(row_off=np.ctypeslib.as_array(v.row_off, shape=(P + 1,)).copy(), bytes=C.string_at(v.bytes, n) if n else b"", num_rows=int(v.num_rows),
                    num_bytes=n)

    def bytes(self, begin: int, end: int) -> bytes:
        """Bytes [begin, end) of the text (rpvg_hip_table_text_get)."""
        out = C.create_string_buffer(max(end - begin, 1))
        hip._check(hip.lib().rpvg_hip_table_text_get(self.handle, C.c_uint64(begin), C.c_uint64(end), out), "rpvg_hip_table_text_get")
        return out.raw[:max(end - begin, 0)]

    def guards_intact(self) -> bool:
        """Whether the 64 pattern bytes on either side of the text on the device are as they were written."""
        intact = C.c_int32(0)
        hip._check(hip.lib().rpvg_hip_table_text_guards(self.handle, C.byref(intact)), "rpvg_hip_table_text_guards")
        return bool(intact.value)

    def bgzf(self) -> "BgzfText":
        """The text as BGZF members, deflated on the GPU (rpvg_hip_table_text_bgzf).  The text stays as it is."""
        handle = C.c_void_p()
        hip._check(hip.lib().rpvg_hip_table_text_bgzf(self.handle, C.byref(handle)), "rpvg_hip_table_text_bgzf")
        return BgzfText(handle)

    def parse(self, prob_precision: float = 1e-8) -> "ParsedDump":
        """The text of a --write-probs dump parsed where it lies (rpvg_hip_table_text_rows): nothing is downloaded."""
        handle = C.c_void_p()
        hip._check(hip.lib().rpvg_hip_table_text_rows(self.handle, C.c_double(prob_precision), C.byref(handle)), "rpvg_hip_table_text_rows")
        return ParsedDump(handle)

    def _release(self):
        hip.lib().rpvg_hip_table_text_free(self.handle)


class CParsedDumpView(C.Structure):
    """rpvg_parsed_dump_view"""
    _fields_ = [("num_clusters", C.c_uint32), ("num_paths", C.c_uint64), ("num_name_bytes", C.c_uint64), ("cluster_path_off", C.POINTER(C.c_uint64)),
                ("name_off", C.POINTER(C.c_uint64)), ("name_bytes", C.POINTER(C.c_char)), ("path_length", C.POINTER(C.c_uint32)),
                ("path_effective_length", C.POINTER(C.c_double)), ("has_rank_key", C.POINTER(C.c_uint8)), ("num_align_lists", C.POINTER(C.c_uint64)),
                ("cluster_index", C.POINTER(C.c_uint64))]


def _array(pointer, n, dtype):
    return np.ctypeslib.as_array(pointer, shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype=dtype)


class ParsedDump(HandleOwner):
    """A dump parsed on the GPU (rpvg_hip_parsed_dump): it owns the resident rows and the path side."""

    def __init__(self, handle):
        self.handle = handle

    @property
    def rows(self):
        """The handle of the resident rows (rpvg_hip_read_rows *), valid until free(): what rpvg_hip_read_rows_to_batch, _view, _sizes
        and rpvg_hip_read_rows_text take."""
        return C.c_void_p(hip.lib().rpvg_hip_parsed_dump_rows(self.handle))

    def view(self) -> dict:
        """Host copies of the path side by name: cluster_path_off, name_off, name_bytes (bytes), path_length, path_effective_length,
        has_rank_key, num_align_lists, cluster_index."""
        v = CParsedDumpView()
        hip._check(hip.lib().rpvg_hip_parsed_dump_view(self.handle, C.byref(v)), "rpvg_hip_parsed_dump_view")
        K, P, n = int(v.num_clusters), int(v.num_paths), int(v.num_name_bytes)
        return dict(cluster_path_off=_array(v.cluster_path_off, K + 1, np.uint64), name_off=_array(v.name_off, P + 1, np.uint64),
                    name_bytes=C.string_at(v.name_bytes, n) if n else b"", path_length=_array(v.path_length, P, np.uint32),
                    path_effective_length=_array(v.path_effective_length, P, np.float64), has_rank_key=_array(v.has_rank_key, K, np.uint8),
                    num_align_lists=_array(v.num_align_lists, K, np.uint64), cluster_index=_array(v.cluster_index, K, np.uint64))

    def rows_view(self, ctx_or_engine) -> dict:
        """Host copies of the rows by name (rpvg_hip_read_rows_view): the row arrays of rpvg_rows_text_input."""
        v = hip.CClusterBatch()
        hip._check(hip.lib().rpvg_hip_read_rows_view(ctx_handle(ctx_or_engine), self.rows, C.byref(v), None, None), "rpvg_hip_read_rows_view")
        K = int(v.num_clusters)
        cro = _array(C.cast(v.cluster_row_off, C.POINTER(C.c_uint64)), K + 1, np.uint64)
        R = int(cro[K])
        rgo = _array(C.cast(v.row_grp_off, C.POINTER(C.c_uint64)), R + 1, np.uint64)
        G = int(rgo[R])
        gio = _array(C.cast(v.grp_idx_off, C.POINTER(C.c_uint64)), G + 1, np.uint64)
        M = int(gio[G])
        return dict(cluster_row_off=cro, cluster_path_off=_array(C.cast(v.cluster_path_off, C.POINTER(C.c_uint64)), K + 1, np.uint64),
                    row_count=_array(C.cast(v.row_count, C.POINTER(C.c_uint32)), R, np.uint32), row_noise=_array(C.cast(v.row_noise, C.POINTER(C.c_double)), R, np.float64),
                    row_grp_off=rgo, grp_prob=_array(C.cast(v.grp_prob, C.POINTER(C.c_double)), G, np.float64), grp_idx_off=gio,
                    path_idx=_array(C.cast(v.path_idx, C.POINTER(C.c_uint32)), M, np.uint32))

    def labels(self) -> CTableLabels:
        """The names, lengths and ClusterIDs where they lie on the GPU (on_device = 1), valid until free()."""
        out = CTableLabels()
        hip._check(hip.lib().rpvg_hip_parsed_dump_labels(self.handle, C.byref(out)), "rpvg_hip_parsed_dump_labels")
        return out

    def to_batch(self, ctx: "hip.Context") -> "hip.DeviceBatch":
        """The batch the estimators take, made on the GPU from the resident rows (rpvg_hip_read_rows_to_batch)."""
        rows = hip.DeviceRows(ctx, self.rows)
        try:
            return rows.to_batch()
        finally:
            rows.handle = C.c_void_p()  # the dump's, not the wrapper's

    def text(self, ctx_or_engine, prob_precision: float = 1e-8) -> TableText:
        """The rows back as text with the dump's own labels, effective lengths and markers (rpvg_hip_read_rows_text)."""
        v = self.view()
        ranked = bool(v["has_rank_key"].any())
        return TableText.resident_rows(ctx_or_engine, self.rows, self.labels(), v["path_effective_length"], prob_precision,
                                       v["num_align_lists"] if ranked else None, v["cluster_index"] if ranked else None)

    def _release(self):
        hip.lib().rpvg_hip_parsed_dump_free(self.handle)


def parse_rows(ctx_or_engine, data, device_pointer=None, num_bytes: Optional[int] = None, prob_precision: float = 1e-8) -> ParsedDump:
    """The text of a --write-probs dump parsed on the GPU (rpvg_hip_text_rows): data is a bytes-like object in host memory, or None
    with device_pointer and num_bytes for a text in the memory of the context's GPU.  A refused text raises hip.EngineError with
    the 1-based line and the reason."""
    handle = C.c_void_p()
    if device_pointer is not None:
        pointer, n, on_device = C.c_void_p(device_pointer), int(num_bytes), 1
    else:
        raw = bytes(data)
        pointer, n, on_device = C.cast(C.c_char_p(raw), C.c_void_p), len(raw), 0
    hip._check(hip.lib().rpvg_hip_text_rows(ctx_handle(ctx_or_engine), pointer, C.c_uint64(n), C.c_int32(on_device), C.c_double(prob_precision), C.byref(handle)),
               "rpvg_hip_text_rows")
    return ParsedDump(handle)


class CRowsParseView(C.Structure):
    """rpvg_amd_rows_parse_view of the harness"""
    _fields_ = [(n, C.c_uint64) for n in ("num_clusters", "num_paths", "num_rows", "num_groups", "num_entries", "num_name_bytes")] + \
               [(n, C.POINTER(C.c_uint64)) for n in ("cluster_row_off", "cluster_path_off", "row_grp_off", "grp_idx_off", "name_off", "num_align_lists", "cluster_index")] + \
               [(n, C.POINTER(C.c_uint32)) for n in ("row_count", "path_idx", "path_length")] + \
               [(n, C.POINTER(C.c_double)) for n in ("row_noise", "grp_prob", "path_effective_length")] + \
               [("has_rank_key", C.POINTER(C.c_uint8)), ("name_bytes", C.POINTER(C.c_char)), ("seconds", C.c_double)]


PARSED_ARRAYS = ("cluster_row_off", "cluster_path_off", "row_count", "row_noise", "row_grp_off", "grp_prob", "grp_idx_off", "path_idx", "name_off", "name_bytes",
                 "path_length", "path_effective_length", "has_rank_key", "num_align_lists", "cluster_index")


def _parse_harness():
    from . import engine
    L = engine.lib()
    L.rpvg_amd_rows_parse_last_error.restype = C.c_char_p
    for name, argtypes in (("rpvg_amd_rows_parse", [C.c_void_p, C.c_char_p, C.c_uint64, C.c_double]), ("rpvg_amd_rows_parse_host_line", [C.c_char_p, C.c_uint64, C.c_double]),
                           ("rpvg_amd_rows_parse_plan", [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]), ("rpvg_amd_rows_parse_file", [C.c_void_p, C.c_char_p, C.c_double, C.c_int])):
        getattr(L, name).restype, getattr(L, name).argtypes = C.c_void_p, argtypes
    L.rpvg_amd_rows_parse_view.argtypes = [C.c_void_p, C.POINTER(CRowsParseView)]
    L.rpvg_amd_rows_parse_free.argtypes = [C.c_void_p]
    L.rpvg_amd_read_text_file_seconds.restype = C.c_double
    L.rpvg_amd_read_text_file_seconds.argtypes = [C.c_char_p, C.POINTER(C.c_uint64)]
    return L


def _flat_of(L, handle, what: str) -> dict:
    """The arrays of PARSED_ARRAYS by name (copies) and the reader's seconds."""
    if not handle:
        raise hip.EngineError(f"{what} failed: {L.rpvg_amd_rows_parse_last_error().decode()}")
    try:
        v = CRowsParseView()
        L.rpvg_amd_rows_parse_view(handle, C.byref(v))
        K, P, R, G, M, n = (int(getattr(v, f)) for f in ("num_clusters", "num_paths", "num_rows", "num_groups", "num_entries", "num_name_bytes"))
        sizes = dict(cluster_row_off=K + 1, cluster_path_off=K + 1, row_grp_off=R + 1, grp_idx_off=G + 1, name_off=P + 1, num_align_lists=K, cluster_index=K, row_count=R,
                     path_idx=M, path_length=P, row_noise=R, grp_prob=G, path_effective_length=P, has_rank_key=K)
        out = {name: _array(getattr(v, name), size, getattr(v, name)._type_) for name, size in sizes.items()}
        out["name_bytes"] = C.string_at(v.name_bytes, n) if n else b""
        out["seconds"] = v.seconds
        return out
    finally:
        L.rpvg_amd_rows_parse_free(handle)


def host_line_parse(data, prob_precision: float = 1e-8) -> dict:
    """readProbabilityClusters on the text, flattened to the arrays of PARSED_ARRAYS: the reader the device parse replaces.  No GPU."""
    L, raw = _parse_harness(), bytes(data)
    return _flat_of(L, L.rpvg_amd_rows_parse_host_line(raw, len(raw), prob_precision), "the host reader")


def plan_parse(data) -> dict:
    """The functions of rpvg_amd/csrc/rows_parse_plan.hpp over serial scans on the host: the arrays the kernels make, and
    exact_tokens; a refused text raises hip.EngineError("... line <n>: <reason>").  No GPU."""
    L, raw, exact = _parse_harness(), bytes(data), C.c_uint64(0)
    out = _flat_of(L, L.rpvg_amd_rows_parse_plan(raw, len(raw), C.byref(exact)), "the plan's parse")
    return dict(out, exact_tokens=int(exact.value))


def harness_parse(engine, data, prob_precision: float = 1e-8) -> dict:
    """The device parse through the host class (rpvg_amd::ParsedDump), flat from its views."""
    L, raw = _parse_harness(), bytes(data)
    return _flat_of(L, L.rpvg_amd_rows_parse(engine.handle, raw, len(raw), prob_precision), "the device parse")


def harness_parse_file(engine, filename: str, prob_precision: float = 1e-8, on_device: bool = True) -> dict:
    """A file through readProbabilityClustersDevice (on_device) or readProbabilityClusters, flattened."""
    L = _parse_harness()
    return _flat_of(L, L.rpvg_amd_rows_parse_file(engine.handle if engine is not None else None, filename.encode(), prob_precision, int(on_device)), "the reader")


class BgzfText(HandleOwner):
    """BGZF members resident on the GPU (rpvg_hip_text_bgzf): the bytes of a .gz file but for the end-of-file block."""

    def __init__(self, handle):
        self.handle = handle

    def view(self) -> dict:
        """num_members, num_text_bytes, num_bytes, num_stored_members, member_off [num_members + 1] and the members as bytes."""
        v = CTextBgzfView()
        hip._check(hip.lib().rpvg_hip_text_bgzf_view(self.handle, C.byref(v)), "rpvg_hip_text_bgzf_view")
        return _bgzf_view_dict(v)

    def bytes(self, begin: int, end: int) -> bytes:
        """Bytes [begin, end) of the members (rpvg_hip_text_bgzf_get)."""
        out = C.create_string_buffer(max(end - begin, 1))
        hip._check(hip.lib().rpvg_hip_text_bgzf_get(self.handle, C.c_uint64(begin), C.c_uint64(end), out), "rpvg_hip_text_bgzf_get")
        return out.raw[:max(end - begin, 0)]

    def guards_intact(self) -> bool:
        intact = C.c_int32(0)
        hip._check(hip.lib().rpvg_hip_text_bgzf_guards(self.handle, C.byref(intact)), "rpvg_hip_text_bgzf_guards")
        return bool(intact.value)

    def _release(self):
        hip.lib().rpvg_hip_text_bgzf_free(self.handle)


def bgzf_bytes(ctx_or_engine, data, device_pointer=None, num_bytes: Optional[int] = None) -> BgzfText:
    """Any bytes as BGZF members (rpvg_hip_bytes_bgzf): data is a bytes-like object in host memory, or None with device_pointer
    and num_bytes for bytes that lie in the memory of the context's GPU."""
    handle = C.c_void_p()
    if device_pointer is not None:
        pointer, n, on_device = C.c_void_p(device_pointer), int(num_bytes), 1
    else:
        raw = bytes(data) if data is not None else b""
        n = len(raw) if num_bytes is None else int(num_bytes)
        pointer, on_device = C.cast(C.c_char_p(raw), C.c_void_p) if data is not None else C.c_void_p(None), 0
    hip._check(hip.lib().rpvg_hip_bytes_bgzf(ctx_handle(ctx_or_engine), pointer, C.c_uint64(n), C.c_int32(on_device), C.byref(handle)), "rpvg_hip_bytes_bgzf")
    return BgzfText(handle)


def bgzf_model(data) -> dict:
    """The members the GPU makes of these bytes, from the host's model of its kernel (rpvg_amd/csrc/text_deflate_plan.hpp:
    modelMembers), without a GPU: bytes and num_stored_members."""
    from . import engine
    L = engine.lib()
    L.rpvg_amd_bytes_bgzf_model.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    raw = bytes(data)
    n, stored = C.c_uint64(0), C.c_uint64(0)
    if L.rpvg_amd_bytes_bgzf_model(raw, len(raw), None, C.byref(n), C.byref(stored)) != 0:
        raise hip.EngineError(f"bgzf model failed: {engine._err()}")
    out = C.create_string_buffer(max(n.value, 1))
    if L.rpvg_amd_bytes_bgzf_model(raw, len(raw), out, None, None) != 0:
        raise hip.EngineError(f"bgzf model failed: {engine._err()}")
    return dict(bytes=out.raw[:n.value], num_stored_members=int(stored.value))


# ---- the harness: the text of a prepared batch's tables, the files from it and the host line ------------------------------------

def _harness():
    from . import engine
    L = engine.lib()
    L.rpvg_amd_table_text_gibbs.restype = C.c_void_p
    L.rpvg_amd_table_text_gibbs.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_double)]
    L.rpvg_amd_table_text_estimates.restype = C.c_void_p
    L.rpvg_amd_table_text_estimates.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    L.rpvg_amd_table_text_sets.restype = C.c_void_p
    L.rpvg_amd_table_text_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_double, C.c_int32, C.POINTER(C.c_double)]
    L.rpvg_amd_table_text_rows.restype = C.c_void_p
    L.rpvg_amd_table_text_rows.argtypes = [C.c_void_p, C.POINTER(CRowsTextInput), C.POINTER(CTableLabels), C.c_double, C.POINTER(C.c_double)]
    L.rpvg_amd_table_text_resident_rows.restype = C.c_void_p
    L.rpvg_amd_table_text_resident_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CTableLabels), C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_double)]
    L.rpvg_amd_table_text_view.argtypes = [C.c_void_p, C.POINTER(CTableTextView)]
    L.rpvg_amd_table_text_write.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32]
    L.rpvg_amd_table_text_write_compressed.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32]
    L.rpvg_amd_table_text_bgzf.argtypes = [C.c_void_p, C.POINTER(CTextBgzfView), C.POINTER(C.c_double)]
    L.rpvg_amd_table_text_host_line.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                                C.POINTER(C.c_double)]
    L.rpvg_amd_table_text_parent_route.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rpvg_amd_table_text_free.argtypes = [C.c_void_p]
    return L, engine


class HarnessTableText(HandleOwner):
    """The text of a harness table (gibbs_table.HarnessGibbsTable or estimates_table.HarnessTable, which must outlive it)."""

    def __init__(self, engine, table, kind: Optional[int] = None, precision: int = 8, ploidy: int = 0, min_posterior: float = 0.0, labels: Optional[Labels] = None,
                 prob_precision: float = 1e-8, effective_lengths=None, num_align_lists=None, cluster_index=None):
        """kind None: the Gibbs text; PER_PATH, HAPLOTYPE: a row per path; JOINT, POSTERIOR: a row per path group set, for a writer of
        `ploidy` and `min_posterior` (in view() and host_line() the rows are then the sets).  ROWS: the --write-probs dump at
        `prob_precision` with `labels` (with path_length); `table` is a RowsInput, or the handle of resident rows built on the
        engine's context (engine._ctx()), which takes effective_lengths and the rank keys beside it.  The rows of view() and
        host_line() are then the 2 K + R lines, and write(name) writes the file `name`."""
        L, eng = _harness()
        secs = C.c_double(0)
        if kind == ROWS:
            self._keep = [labels.as_c()]
            if isinstance(table, RowsInput):
                self._keep.append(table.as_c())
                self.handle = L.rpvg_amd_table_text_rows(engine.handle, C.byref(self._keep[1]), C.byref(self._keep[0]), prob_precision, C.byref(secs))
            else:
                arrays = [np.ascontiguousarray(effective_lengths, dtype=np.float64)] + [None if a is None else np.ascontiguousarray(a, dtype=np.uint64) for a in (num_align_lists, cluster_index)]
                pointers = [C.c_void_p(a.ctypes.data if a is not None and a.size else None) for a in arrays]
                self.handle = L.rpvg_amd_table_text_resident_rows(engine.handle, table, C.byref(self._keep[0]), *pointers, prob_precision, C.byref(secs))
        elif kind is None:
            self.handle = L.rpvg_amd_table_text_gibbs(engine.handle, table.handle, precision, C.byref(secs))
        elif kind in (JOINT, POSTERIOR):
            self.handle = L.rpvg_amd_table_text_sets(engine.handle, table.handle, kind, ploidy, min_posterior, precision, C.byref(secs))
        else:
            self.handle = L.rpvg_amd_table_text_estimates(engine.handle, table.handle, kind, precision, C.byref(secs))
        if not self.handle:
            raise hip.EngineError(f"table text failed: {eng._err()}")
        self.build_seconds, self._table = secs.value, table

    def view(self, copy: bool = True) -> dict:
        L, eng = _harness()
        v = CTableTextView()
        if L.rpvg_amd_table_text_view(self.handle, C.byref(v)) != 0:
            raise hip.EngineError(f"table text view failed: {eng._err()}")
        P, n = int(v.num_paths), int(v.num_bytes)
        return dict(row_off=np.ctypeslib.as_array(v.row_off, shape=(P + 1,)).copy(), bytes=C.string_at(v.bytes, n) if n and copy else b"", num_rows=int(v.num_rows),
                    num_bytes=n)

    def write(self, prefix: str, num_gibbs_samples: int = 0, unaligned_read_count: int = 0, compressed: bool = False):
        """<prefix>.txt.gz (a Gibbs text) or <prefix>.txt (an estimates text) through the writer's addText().  compressed: the rows
        go into the file as the BGZF members the GPU deflated (the Gibbs file through addCompressedText(), the dump through
        writeProbabilityClustersBgzf); the estimates files are plain text and refuse it."""
        L, eng = _harness()
        write = L.rpvg_amd_table_text_write_compressed if compressed else L.rpvg_amd_table_text_write
        if write(self.handle, num_gibbs_samples, prefix.encode(), unaligned_read_count) != 0:
            raise hip.EngineError(f"table text write failed: {eng._err()}")

    def bgzf(self, copy: bool = True) -> dict:
        """The text as BGZF members deflated on the GPU (the host class's TableText::bgzf): the dict of BgzfText.view(), and the
        seconds the compression and the download of the members took in this call (0 when an earlier call had done them)."""
        L, eng = _harness()
        v = CTextBgzfView()
        seconds = (C.c_double * 2)()
        if L.rpvg_amd_table_text_bgzf(self.handle, C.byref(v), seconds) != 0:
            raise hip.EngineError(f"table text bgzf failed: {eng._err()}")
        if not copy:
            v.num_bytes, n = 0, int(v.num_bytes)
        out = _bgzf_view_dict(v)
        if not copy:
            out["num_bytes"] = n
        return dict(out, compress_seconds=seconds[0], download_seconds=seconds[1])

    def host_line(self, num_paths: int, want_bytes: bool = True, recompute: bool = False) -> dict:
        """The same rows from the host views of the table on one host thread: bytes, row_off, exact_cells, seconds (of the walk,
        when this call walked), and equal: whether bytes and row_off are the device text's (compared by the harness)."""
        L, eng = _harness()
        n, exact, equal, secs = C.c_uint64(0), C.c_uint64(0), C.c_int32(0), C.c_double(0)
        row_off = np.zeros(num_paths + 1, dtype=np.uint64)
        if L.rpvg_amd_table_text_host_line(self.handle, int(recompute), None, row_off.ctypes.data, C.byref(n), C.byref(exact), C.byref(equal), C.byref(secs)) != 0:
            raise hip.EngineError(f"table text host line failed: {eng._err()}")
        out = C.create_string_buffer(max(n.value, 1) if want_bytes else 1)
        if want_bytes and L.rpvg_amd_table_text_host_line(self.handle, 0, out, None, None, None, None, None) != 0:
            raise hip.EngineError(f"table text host line failed: {eng._err()}")
        return dict(bytes=out.raw[:n.value] if want_bytes else b"", row_off=row_off, exact_cells=int(exact.value), seconds=secs.value, num_bytes=int(n.value),
                    equal=bool(equal.value))

    def parent_route(self, num_gibbs_samples: int = 0):
        """(seconds of the table's host view, seconds of the writer's addTable() into its stream): the route the text replaces."""
        L, eng = _harness()
        viewed, added = C.c_double(0), C.c_double(0)
        if L.rpvg_amd_table_text_parent_route(self.handle, num_gibbs_samples, C.byref(viewed), C.byref(added)) != 0:
            raise hip.EngineError(f"table text parent route failed: {eng._err()}")
        return viewed.value, added.value

    def _release(self):
        _harness()[0].rpvg_amd_table_text_free(self.handle)


def host_line_rows(rows_input: RowsInput, labels: Labels, prob_precision: float = 1e-8) -> dict:
    """The --write-probs dump of host arrays from one host thread, without a GPU (rpvg_amd/host/table_text.hpp: hostLineRows over the
    plan's rowBytes and rowWrite): bytes, row_off [2 K + R + 1], exact_cells and the seconds of the walk."""
    from . import engine
    L = engine.lib()
    L.rpvg_amd_rows_text_host_line.argtypes = [C.POINTER(CRowsTextInput), C.POINTER(CTableLabels), C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    inp, flat = rows_input.as_c(), labels.as_c()
    n, exact, secs = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
    row_off = np.zeros(2 * inp.num_clusters + inp.num_rows + 1, dtype=np.uint64)
    if L.rpvg_amd_rows_text_host_line(C.byref(inp), C.byref(flat), prob_precision, None, row_off.ctypes.data, C.byref(n), C.byref(exact), C.byref(secs)) != 0:
        raise hip.EngineError(f"rows text host line failed: {engine._err()}")
    out = C.create_string_buffer(max(n.value, 1))
    if L.rpvg_amd_rows_text_host_line(C.byref(inp), C.byref(flat), prob_precision, out, None, None, None, None) != 0:
        raise hip.EngineError(f"rows text host line failed: {engine._err()}")
    return dict(bytes=out.raw[:n.value], row_off=row_off, exact_cells=int(exact.value), seconds=secs.value, num_bytes=int(n.value))


def read_text_file_seconds(filename: str) -> float:
    """The seconds readTextFile takes on the file (tools/rows_parse_ab.py)."""
    L, n = _parse_harness(), C.c_uint64(0)
    seconds = L.rpvg_amd_read_text_file_seconds(filename.encode(), C.byref(n))
    if seconds < 0:
        raise hip.EngineError(f"readTextFile failed: {L.rpvg_amd_rows_parse_last_error().decode()}")
    return seconds
