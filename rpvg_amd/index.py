"""The alignment-path index (include/rpvg_index.h, rpvg_amd/csrc/align_index.hip): a stream of per-fragment
alignment-path lists in, distinct lists with multiplicities in the reference's cluster order out
(addAlignmentPathsBufferToIndexes, src/main.cpp:200-237, and the caller's loop, :731-754,811-827,846-857).
Marshalling for tests, tools and the harness."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import hip
from .batch import f64p, u32p, u64p, _ptr
from .rows import AlignmentBatch, CAlignmentBatch, i32p, u8p, u16p


def _arr(ptr, n, dt):
    if n == 0:
        return np.zeros(0, dtype=dt)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True)


class CFragmentLists(C.Structure):
    """rpvg_fragment_lists"""
    _fields_ = [("num_lists", C.c_uint64), ("list_is_simple", u8p), ("list_min_mapq", u8p), ("list_noise_score", i32p),
                ("list_align_off", u64p), ("align_score_sum", i32p), ("align_length", u16p), ("align_frag_length", u16p),
                ("align_path_off", u64p), ("align_path_id", u32p)]


class CIndexParams(C.Structure):
    """rpvg_index_params"""
    _fields_ = [("num_paths", C.c_uint32), ("is_single_end", C.c_int32), ("frag_length_min_mapq", C.c_uint32),
                ("max_frag_length", C.c_uint32), ("pre_frag_loc", C.c_uint16), ("hash_bits", C.c_uint32)]


class CIndexInfo(C.Structure):
    """rpvg_index_info"""
    _fields_ = [("num_lists", C.c_uint64), ("num_distinct", C.c_uint64), ("num_clusters", C.c_uint32),
                ("num_collision_lists", C.c_uint64)]


class CIndexView(C.Structure):
    """rpvg_index_view"""
    _fields_ = [("batch", CAlignmentBatch), ("rank_cluster", u32p), ("path_to_cluster", u32p), ("cluster_paths", u32p),
                ("first_occurrence", u64p)]


class CPathTable(C.Structure):
    """rpvg_path_table"""
    _fields_ = [("num_paths", C.c_uint32), ("num_sources", C.c_uint64), ("group_id", u32p), ("source_count", u32p), ("source_off", u64p),
                ("source_id", u32p), ("name_id", u32p), ("length", u32p), ("effective_length", f64p)]


class CNameGroupsLimits(C.Structure):
    """rpvg_name_groups_limits"""
    _fields_ = [("wave_paths", C.c_uint32), ("lds_paths", C.c_uint32)]


class CNameGroupsView(C.Structure):
    """rpvg_name_groups_view"""
    _fields_ = [("num_clusters", C.c_uint32), ("num_paths", C.c_uint32), ("path_group", u32p), ("cluster_group_off", u64p),
                ("group_first_path", u32p), ("group_name_id", u32p), ("group_group_id", u32p), ("group_source_count", u32p),
                ("group_length", u32p), ("group_effective_length", f64p)]


@dataclass
class PathTable:
    """The PathInfo of every path of a run by global path id (rpvg_path_table).  source_off / source_id None: no haplotype ids;
    name_id None: no names (equal ids = equal names)."""
    group_id: np.ndarray
    source_count: np.ndarray
    length: np.ndarray
    effective_length: np.ndarray
    source_off: Optional[np.ndarray] = None
    source_id: Optional[np.ndarray] = None
    name_id: Optional[np.ndarray] = None

    _DTYPES = dict(group_id=np.uint32, source_count=np.uint32, length=np.uint32, effective_length=np.float64, source_off=np.uint64,
                   source_id=np.uint32, name_id=np.uint32)

    def __post_init__(self):
        for name, dt in self._DTYPES.items():
            v = getattr(self, name)
            if v is not None:
                setattr(self, name, np.ascontiguousarray(v, dtype=dt))

    @property
    def num_paths(self) -> int:
        return len(self.group_id)

    @staticmethod
    def from_paths(paths: Sequence[dict]) -> "PathTable":
        """paths: [{"group_id", "source_count", "length", "effective_length", "source_ids"?: [...], "name"?: hashable}...];
        names become ids in order of first appearance; source ids are kept in the order given."""
        names, name_id, off, ids = {}, [], [0], []
        with_names = any("name" in p for p in paths)
        with_sources = any("source_ids" in p for p in paths)
        for p in paths:
            if with_names:
                name_id.append(names.setdefault(p["name"], len(names)))
            if with_sources:
                ids.extend(p.get("source_ids", ()))
                off.append(len(ids))
        return PathTable([p["group_id"] for p in paths], [p["source_count"] for p in paths], [p["length"] for p in paths],
                         [p["effective_length"] for p in paths], off if with_sources else None, ids if with_sources else None,
                         name_id if with_names else None)

    def as_c(self) -> CPathTable:
        def opt(a, ty):
            return _ptr(a, ty) if a is not None else None
        S = len(self.source_id) if self.source_id is not None else 0
        return CPathTable(self.num_paths, S, _ptr(self.group_id, u32p), _ptr(self.source_count, u32p), opt(self.source_off, u64p),
                          opt(self.source_id, u32p), opt(self.name_id, u32p), _ptr(self.length, u32p), _ptr(self.effective_length, f64p))


class DevicePathTable:
    """A PathTable resident on the GPU (rpvg_hip_path_table)."""

    def __init__(self, ctx: "hip.Context", host: PathTable):
        self.ctx, self.host = ctx, host
        self.handle = C.c_void_p()
        ct = host.as_c()
        hip._check(hip.lib().rpvg_hip_path_table_upload(ctx.handle, C.byref(ct), C.byref(self.handle)), "rpvg_hip_path_table_upload")

    def free(self):
        if self.handle:
            hip.lib().rpvg_hip_path_table_free(self.ctx.handle, self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def name_groups_limits() -> CNameGroupsLimits:
    """The largest cluster of the one-wavefront route and of the LDS route of AlignmentIndex.name_groups."""
    limits = CNameGroupsLimits()
    hip.lib().rpvg_hip_name_groups_limits(C.byref(limits))
    return limits


class NameGroups:
    """The name groups of an index and their collapsed paths, resident (rpvg_hip_name_groups)."""

    def __init__(self, ctx: "hip.Context", handle):
        self.ctx, self.handle = ctx, handle

    def view(self) -> dict:
        """Host copies by name: path_group [P], cluster_group_off [K+1] and the group_* arrays [G]."""
        v = CNameGroupsView()
        hip._check(hip.lib().rpvg_hip_name_groups_view(self.ctx.handle, self.handle, C.byref(v)), "rpvg_hip_name_groups_view")
        cgo = _arr(v.cluster_group_off, v.num_clusters + 1, np.uint64)
        G = int(cgo[-1])
        return dict(path_group=_arr(v.path_group, v.num_paths, np.uint32), cluster_group_off=cgo,
                    group_first_path=_arr(v.group_first_path, G, np.uint32), group_name_id=_arr(v.group_name_id, G, np.uint32),
                    group_group_id=_arr(v.group_group_id, G, np.uint32), group_source_count=_arr(v.group_source_count, G, np.uint32),
                    group_length=_arr(v.group_length, G, np.uint32), group_effective_length=_arr(v.group_effective_length, G, np.float64))

    def free(self):
        if self.handle:
            hip.lib().rpvg_hip_name_groups_free(self.ctx.handle, self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


@dataclass
class IndexParams:
    num_paths: int
    is_single_end: bool = False
    frag_length_min_mapq: int = 30
    max_frag_length: int = 1000
    pre_frag_loc: int = 300
    hash_bits: int = 0

    def as_c(self) -> CIndexParams:
        return CIndexParams(self.num_paths, 1 if self.is_single_end else 0, self.frag_length_min_mapq, self.max_frag_length,
                            self.pre_frag_loc, self.hash_bits)


@dataclass
class FragmentLists:
    """One chunk of the stream, flat (rpvg_fragment_lists)."""
    list_is_simple: np.ndarray
    list_min_mapq: np.ndarray
    list_noise_score: np.ndarray
    list_align_off: np.ndarray
    align_score_sum: np.ndarray
    align_length: np.ndarray
    align_frag_length: np.ndarray
    align_path_off: np.ndarray
    align_path_id: np.ndarray

    _DTYPES = dict(list_is_simple=np.uint8, list_min_mapq=np.uint8, list_noise_score=np.int32, list_align_off=np.uint64,
                   align_score_sum=np.int32, align_length=np.uint16, align_frag_length=np.uint16, align_path_off=np.uint64,
                   align_path_id=np.uint32)

    def __post_init__(self):
        for name, dt in self._DTYPES.items():
            setattr(self, name, np.ascontiguousarray(getattr(self, name), dtype=dt))

    @property
    def num_lists(self) -> int:
        return len(self.list_is_simple)

    @staticmethod
    def from_lists(lists: Sequence[dict]) -> "FragmentLists":
        """lists: [{"is_simple", "min_mapq", "noise_score", "aligns": [(score_sum, align_length, frag_length, [path id...])...]}...]
        Nothing is sorted or checked: an invalid list reaches the device as it is."""
        simple, mapq, noise, lao = [], [], [], [0]
        score, alen, flen, apo, ids = [], [], [], [0], []
        for ls in lists:
            simple.append(1 if ls["is_simple"] else 0)
            mapq.append(ls["min_mapq"])
            noise.append(ls["noise_score"])
            for (s, a, f, paths) in ls["aligns"]:
                score.append(s)
                alen.append(a)
                flen.append(f)
                ids.extend(paths)
                apo.append(len(ids))
            lao.append(len(score))
        return FragmentLists(simple, mapq, noise, lao, score, alen, flen, apo, ids)

    def slice(self, begin: int, end: int) -> "FragmentLists":
        """Lists [begin, end) as a chunk of their own."""
        a0, a1 = int(self.list_align_off[begin]), int(self.list_align_off[end])
        e0, e1 = int(self.align_path_off[a0]), int(self.align_path_off[a1])
        return FragmentLists(self.list_is_simple[begin:end], self.list_min_mapq[begin:end], self.list_noise_score[begin:end],
                             self.list_align_off[begin:end + 1] - np.uint64(a0), self.align_score_sum[a0:a1], self.align_length[a0:a1],
                             self.align_frag_length[a0:a1], self.align_path_off[a0:a1 + 1] - np.uint64(e0), self.align_path_id[e0:e1])

    def as_c(self) -> CFragmentLists:
        return CFragmentLists(self.num_lists, _ptr(self.list_is_simple, u8p), _ptr(self.list_min_mapq, u8p), _ptr(self.list_noise_score, i32p),
                              _ptr(self.list_align_off, u64p), _ptr(self.align_score_sum, i32p), _ptr(self.align_length, u16p),
                              _ptr(self.align_frag_length, u16p), _ptr(self.align_path_off, u64p), _ptr(self.align_path_id, u32p))


@dataclass
class IndexView:
    """Host copy of a finished index (rpvg_index_view).  batch.path_effective_length is all ones: the index does not know it."""
    batch: AlignmentBatch
    rank_cluster: np.ndarray
    path_to_cluster: np.ndarray
    cluster_paths: np.ndarray
    first_occurrence: np.ndarray

    def arrays(self) -> dict:
        """Every array the index itself computed, by name (what tests compare)."""
        b = self.batch
        out = {n: getattr(b, n) for n in ("cluster_read_off", "cluster_path_off", "read_count", "read_min_mapq", "read_noise_score",
                                          "read_align_off", "align_score_sum", "align_length", "align_frag_length", "align_path_off",
                                          "align_path_idx")}
        out.update(rank_cluster=self.rank_cluster, path_to_cluster=self.path_to_cluster, cluster_paths=self.cluster_paths,
                   first_occurrence=self.first_occurrence)
        return out


class AlignmentIndex:
    """rpvg_hip_align_index on a hip.Context: add() chunks, finish(), then frag_counts() / view() / alignments()."""

    def __init__(self, ctx: "hip.Context", params: IndexParams):
        self.ctx = ctx
        self.params = params
        self.handle = C.c_void_p()
        self.info: Optional[CIndexInfo] = None
        cp = params.as_c()
        hip._check(hip.lib().rpvg_hip_align_index_create(ctx.handle, C.byref(cp), C.byref(self.handle)), "rpvg_hip_align_index_create")

    def add(self, chunk: FragmentLists):
        cc = chunk.as_c()
        hip._check(hip.lib().rpvg_hip_align_index_add(self.ctx.handle, self.handle, C.byref(cc)), "rpvg_hip_align_index_add")

    def finish(self, extra_sets: Optional[Sequence[Sequence[int]]] = None) -> CIndexInfo:
        sets = list(extra_sets or [])
        off = np.zeros(len(sets) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in sets], dtype=np.uint64) if sets else []
        flat = np.ascontiguousarray([p for s in sets for p in s], dtype=np.uint32)
        info = CIndexInfo()
        hip._check(hip.lib().rpvg_hip_align_index_finish(
            self.ctx.handle, self.handle, C.c_void_p(off.ctypes.data if sets else None), C.c_void_p(flat.ctypes.data if flat.size else None),
            C.c_uint64(len(sets)), C.byref(info)), "rpvg_hip_align_index_finish")
        self.info = info
        return info

    def frag_counts(self) -> np.ndarray:
        counts = np.zeros(self.params.max_frag_length + 1, dtype=np.uint32)
        hip._check(hip.lib().rpvg_hip_align_index_frag_counts(self.ctx.handle, self.handle, C.c_void_p(counts.ctypes.data)),
                   "rpvg_hip_align_index_frag_counts")
        return counts

    def view(self) -> IndexView:
        v = CIndexView()
        hip._check(hip.lib().rpvg_hip_align_index_view(self.ctx.handle, self.handle, C.byref(v)), "rpvg_hip_align_index_view")
        b = v.batch
        K, P = b.num_clusters, self.params.num_paths
        cro, cpo = _arr(b.cluster_read_off, K + 1, np.uint64), _arr(b.cluster_path_off, K + 1, np.uint64)
        D = int(cro[-1])
        rao = _arr(b.read_align_off, D + 1, np.uint64)
        A = int(rao[-1])
        apo = _arr(b.align_path_off, A + 1, np.uint64)
        batch = AlignmentBatch(cro, cpo, np.ones(P, np.float64), np.ones(P, np.uint32), None, None, _arr(b.read_count, D, np.uint32),
                               _arr(b.read_min_mapq, D, np.uint8), _arr(b.read_noise_score, D, np.int32), rao,
                               _arr(b.align_score_sum, A, np.int32), _arr(b.align_length, A, np.uint16), _arr(b.align_frag_length, A, np.uint16),
                               apo, _arr(b.align_path_idx, int(apo[-1]), np.uint32))
        return IndexView(batch, _arr(v.rank_cluster, K, np.uint32), _arr(v.path_to_cluster, P, np.uint32), _arr(v.cluster_paths, P, np.uint32),
                         _arr(v.first_occurrence, D, np.uint64))

    def alignments(self, path_effective_length, path_source_count=None) -> "hip.DeviceAlignments":
        """The resident alignment batch of the result (rpvg_hip_align_index_alignments); the two arrays are per global path."""
        eff = np.ascontiguousarray(path_effective_length, dtype=np.float64)
        assert eff.size == self.params.num_paths
        src = None if path_source_count is None else np.ascontiguousarray(path_source_count, dtype=np.uint32)
        h = C.c_void_p()
        hip._check(hip.lib().rpvg_hip_align_index_alignments(
            self.ctx.handle, self.handle, C.c_void_p(eff.ctypes.data if eff.size else None),
            C.c_void_p(src.ctypes.data if src is not None and src.size else None), C.byref(h)), "rpvg_hip_align_index_alignments")
        return hip.DeviceAlignments.from_handle(self.ctx, h, self.params.num_paths)

    def name_groups(self, table: DevicePathTable) -> NameGroups:
        """group_name_index of every cluster and the collapsed path of every group (rpvg_hip_align_index_name_groups)."""
        h = C.c_void_p()
        hip._check(hip.lib().rpvg_hip_align_index_name_groups(self.ctx.handle, self.handle, table.handle, C.byref(h)),
                   "rpvg_hip_align_index_name_groups")
        return NameGroups(self.ctx, h)

    def alignments_collapsed(self, table: DevicePathTable, groups: NameGroups) -> "hip.DeviceAlignments":
        """The resident alignment batch with the groups as its output columns (rpvg_hip_align_index_alignments_collapsed)."""
        h = C.c_void_p()
        hip._check(hip.lib().rpvg_hip_align_index_alignments_collapsed(self.ctx.handle, self.handle, table.handle, groups.handle, C.byref(h)),
                   "rpvg_hip_align_index_alignments_collapsed")
        return hip.DeviceAlignments.from_handle(self.ctx, h, self.params.num_paths)

    def free(self):
        if self.handle:
            hip.lib().rpvg_hip_align_index_free(self.ctx.handle, self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def build_index(ctx: "hip.Context", params: IndexParams, chunks: Sequence[FragmentLists], extra_sets=None) -> AlignmentIndex:
    index = AlignmentIndex(ctx, params)
    for chunk in chunks:
        index.add(chunk)
    index.finish(extra_sets)
    return index
