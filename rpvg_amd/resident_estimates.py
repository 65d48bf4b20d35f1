"""Resident estimates (include/rpvg_table.h, rpvg_amd/csrc/estimates_gather.hip): the merged sets the nested calls leave on the GPU,
gathered there into the flat form the estimates table and the text builders take with on_device = 1.

  EstimatesPart       the merged sets of some clusters: from host arrays, or pointing into the kept device block of a nested call
  gather              parts + batch + effective lengths -> ResidentEstimates
  ResidentEstimates   the flat estimates on the device: view() (device pointers), get() (a host FlatEstimates), free()
  nested_*_kept       the three nested calls with their device block kept: (host view, EstimatesPart)
  run_resident        the harness: a prepared batch through the estimator's resident route (None when it is not taken)
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import hip
from ._flat import HandleOwner, ctx_handle
from .estimates_table import CEstimatesFlat, FlatEstimates, HarnessTable

u32p, u64p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)


class CEstimatesPart(C.Structure):
    """rpvg_estimates_part"""
    _fields_ = [("num_units", C.c_uint32), ("num_subsets", C.c_uint64), ("num_slots", C.c_uint64), ("width", C.c_uint32),
                ("unit_cluster", C.c_void_p), ("subset_off", C.c_void_p), ("path_off", C.c_void_p), ("set_count", C.c_void_p),
                ("cluster_noise_count", C.c_void_p), ("set_posterior", C.c_void_p), ("set_first", C.c_void_p), ("set_second", C.c_void_p),
                ("set_size", C.c_void_p), ("set_member", C.c_void_p), ("set_abundance", C.c_void_p), ("on_device", C.c_int32)]


class CSubsetEmView(C.Structure):
    """rpvg_hip_subset_em_view"""
    _fields_ = [("num_matrices", C.c_uint32), ("subset_off", u64p), ("weight", f64p), ("path_off", u64p), ("path", u32p), ("col_off", u64p),
                ("col_path", u32p), ("abundances", f64p), ("noise_count", f64p), ("total_count", f64p), ("iterations", u32p),
                ("set_count", u32p), ("cluster_noise_count", f64p), ("set_first", u32p), ("set_second", u32p), ("set_posterior", f64p),
                ("set_abundance", f64p)]


_PART_ARRAYS = (("subset_off", np.uint64), ("path_off", np.uint64), ("set_count", np.uint32), ("cluster_noise_count", np.float64),
                ("set_posterior", np.float64), ("set_first", np.uint32), ("set_second", np.uint32), ("set_size", np.uint32),
                ("set_member", np.uint32), ("set_abundance", np.float64))


class EstimatesPart:
    """A rpvg_estimates_part and what keeps its memory alive: numpy arrays (on_device = 0), device pointers the caller owns
    (from_device), or the kept block of a nested call's result (from_result: freed with the part)."""

    def __init__(self, c_part: CEstimatesPart, keep=(), result_handle=None):
        self.c, self._keep, self._result = c_part, list(keep), result_handle
        self.unit_cluster = None

    @classmethod
    def from_arrays(cls, width: int, unit_cluster, num_slots: Optional[int] = None, num_subsets: Optional[int] = None, **arrays) -> "EstimatesPart":
        """Host arrays by the names of rpvg_estimates_part (set_member and set_abundance may be [slots, cells]); num_slots and
        num_subsets default to what path_off and set_posterior say."""
        part = CEstimatesPart()
        keep = []
        for name, dtype in _PART_ARRAYS:
            if arrays.get(name) is None:
                continue
            a = np.ascontiguousarray(arrays[name], dtype=dtype)
            keep.append(a)
            setattr(part, name, a.ctypes.data if a.size else None)
        part.width = width
        part.num_subsets = len(arrays["path_off"]) - 1 if num_subsets is None else num_subsets
        part.num_slots = len(arrays["set_posterior"]) if num_slots is None else num_slots
        part.on_device = 0
        self = cls(part, keep)
        self.set_unit_cluster(unit_cluster)
        return self

    @classmethod
    def from_device(cls, width: int, unit_cluster, num_subsets: int, num_slots: int, **pointers) -> "EstimatesPart":
        """Device pointers (ints) by the names of rpvg_estimates_part; the caller keeps the memory alive."""
        part = CEstimatesPart()
        for name, _ in _PART_ARRAYS:
            setattr(part, name, pointers.get(name) or None)
        part.width, part.num_subsets, part.num_slots, part.on_device = width, num_subsets, num_slots, 1
        self = cls(part)
        self.set_unit_cluster(unit_cluster)
        return self

    @classmethod
    def from_result(cls, result_handle, unit_cluster, own: bool = True) -> "EstimatesPart":
        """rpvg_hip_subset_em_part of a nested call's result whose block was kept; raises EngineError (-5) when it was not.  own: the
        part frees the result."""
        part = CEstimatesPart()
        hip._check(hip.lib().rpvg_hip_subset_em_part(result_handle, C.byref(part)), "rpvg_hip_subset_em_part")
        self = cls(part, result_handle=result_handle if own else None)
        self.set_unit_cluster(unit_cluster)
        return self

    def set_unit_cluster(self, unit_cluster):
        self.unit_cluster = np.ascontiguousarray(unit_cluster, dtype=np.uint32)
        self.c.num_units = len(self.unit_cluster)
        self.c.unit_cluster = self.unit_cluster.ctypes.data if len(self.unit_cluster) else None

    def free(self):
        if self._result is not None:
            hip.lib().rpvg_hip_subset_em_free(self._result)
            self._result = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _batch_handle(batch):
    return batch.handle if hasattr(batch, "handle") else batch


class ResidentEstimates(HandleOwner):
    """The flat estimates of a batch on the GPU (rpvg_hip_flat_estimates).  The batch must outlive it."""

    def __init__(self, ctx, handle, keep=()):
        self.ctx_handle, self.handle, self._keep = ctx, handle, list(keep)

    def view(self) -> CEstimatesFlat:
        """rpvg_estimates_flat with on_device = 1: device pointers, host sizes."""
        flat = CEstimatesFlat()
        hip._check(hip.lib().rpvg_hip_flat_estimates_view(self.handle, C.byref(flat)), "rpvg_hip_flat_estimates_view")
        return flat

    def get(self) -> FlatEstimates:
        """A host copy of every array (one packed copy to page-locked memory behind it)."""
        flat = CEstimatesFlat()
        hip._check(hip.lib().rpvg_hip_flat_estimates_get(self.ctx_handle, self.handle, C.byref(flat)), "rpvg_hip_flat_estimates_get")
        return flat_from_c(flat)

    def _release(self):
        hip.lib().rpvg_hip_flat_estimates_free(self.ctx_handle, self.handle)


def flat_from_c(flat: CEstimatesFlat) -> FlatEstimates:
    """Copies of the host arrays a rpvg_estimates_flat with on_device = 0 points to."""
    K, S, M, A, P = (int(flat.num_clusters), int(flat.num_sets), int(flat.num_members), int(flat.num_abundances), int(flat.num_paths))

    def take(address, n, dtype):
        if n == 0 or not address:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(address), dtype=dtype).copy()

    return FlatEstimates(take(flat.set_off, K + 1, np.uint64), take(flat.member_off, S + 1, np.uint64), take(flat.members, M, np.uint32),
                         take(flat.posteriors, S, np.float64), take(flat.abund_off, K + 1, np.uint64), take(flat.abundances, A, np.float64),
                         take(flat.noise_count, K, np.float64), take(flat.cluster_path_off, K + 1, np.uint64),
                         take(flat.path_effective_length, P, np.float64))


def gather(ctx_or_engine, batch, parts: Sequence[EstimatesPart], eff, eff_on_device: bool = False) -> ResidentEstimates:
    """rpvg_hip_flat_estimates_gather: batch a hip.DeviceBatch (or its handle); eff the effective length of every path of the batch,
    a numpy array, or a device pointer (int) with eff_on_device.  Raises EngineError; a refusal carries "(-3)" and names the part
    and the unit."""
    ctx = ctx_handle(ctx_or_engine)
    c_parts = (CEstimatesPart * max(len(parts), 1))(*[p.c for p in parts])
    keep = []
    if eff_on_device:
        eff_pointer = C.c_void_p(int(eff))
    else:
        eff_host = np.ascontiguousarray(eff, dtype=np.float64)
        keep.append(eff_host)
        eff_pointer = C.c_void_p(eff_host.ctypes.data if eff_host.size else None)
    handle = C.c_void_p()
    hip._check(hip.lib().rpvg_hip_flat_estimates_gather(ctx, _batch_handle(batch), c_parts if parts else None, C.c_uint32(len(parts)), eff_pointer,
                                                        C.c_int32(1 if eff_on_device else 0), C.byref(handle)), "rpvg_hip_flat_estimates_gather")
    return ResidentEstimates(ctx, handle)


# ---- the three nested calls with their device block kept -----------------------------------------------------------------------

class _Kept:
    """rpvg_hip_subset_em_keep_device for the length of a call"""

    def __init__(self, ctx, keep: bool):
        self.ctx, self.keep = ctx, keep

    def __enter__(self):
        hip._check(hip.lib().rpvg_hip_subset_em_keep_device(self.ctx.handle, C.c_int32(1 if self.keep else 0)), "rpvg_hip_subset_em_keep_device")

    def __exit__(self, *exc):
        hip.lib().rpvg_hip_subset_em_keep_device(self.ctx.handle, C.c_int32(0))
        return False


def _take(pointer, n, dtype, shape=None):
    if n == 0 or not pointer:
        return np.zeros(shape if shape is not None else (0,), dtype=dtype)
    a = np.ctypeslib.as_array(pointer, shape=(n,)).copy()
    return a.reshape(shape) if shape is not None else a


def nested_subset_em(groups, column_counts, min_rel_likelihood: float, min_hap_prob: float, max_em_its: int = 10000,
                     max_rel_em_conv: float = 1e-3, collapse_precision: float = 0.0, keep: bool = False):
    """rpvg_hip_nested_subset_em (the diploid call) on every matrix of a hip.DeviceGroups: column_counts the multiplicity of every
    column, matrices back to back (None: the matrices were built from the batch's source columns).  Returns (view, handle): the
    fields of rpvg_hip_subset_em_view as numpy arrays (copies; set_abundance as [slots, 2]; the set_* fields None when the call did
    no merge) and the rpvg_hip_subset_em handle, which the caller frees (rpvg_hip_subset_em_free).  keep: with the device block kept."""
    cc = None if column_counts is None else np.ascontiguousarray(column_counts, dtype=np.uint32)
    h = C.c_void_p()
    with _Kept(groups.ctx, keep):
        hip._check(hip.lib().rpvg_hip_nested_subset_em(groups.ctx.handle, groups.batch.handle, groups.handle,
                                                       C.c_void_p(cc.ctypes.data if cc is not None and cc.size else None),
                                                       C.c_double(float(min_rel_likelihood)), C.c_double(float(min_hap_prob)), C.c_uint32(max_em_its),
                                                       C.c_double(float(max_rel_em_conv)), C.c_double(float(collapse_precision)), C.byref(h)),
                   "rpvg_hip_nested_subset_em")
    try:
        v = CSubsetEmView()
        hip._check(hip.lib().rpvg_hip_subset_em_get(h, C.byref(v)), "rpvg_hip_subset_em_get")
        M = int(v.num_matrices)
        out = {"num_matrices": M}
        out["subset_off"] = _take(v.subset_off, M + 1, np.uint64) if M and v.subset_off else np.zeros(1, np.uint64)
        S = int(out["subset_off"][-1])
        out["path_off"] = _take(v.path_off, S + 1, np.uint64) if M and v.path_off else np.zeros(1, np.uint64)
        out["col_off"] = _take(v.col_off, S + 1, np.uint64) if M and v.col_off else np.zeros(1, np.uint64)
        L, Cn = int(out["path_off"][-1]), int(out["col_off"][-1])
        for name, n, dtype in (("weight", S, np.float64), ("path", L, np.uint32), ("col_path", Cn, np.uint32), ("abundances", Cn, np.float64),
                               ("noise_count", S, np.float64), ("total_count", S, np.float64), ("iterations", S, np.uint32)):
            out[name] = _take(getattr(v, name), n, dtype)
        if v.set_count:
            out["set_count"] = _take(v.set_count, M, np.uint32)
            out["cluster_noise_count"] = _take(v.cluster_noise_count, M, np.float64)
            out["set_first"] = _take(v.set_first, L, np.uint32)
            out["set_second"] = _take(v.set_second, L, np.uint32)
            out["set_posterior"] = _take(v.set_posterior, L, np.float64)
            out["set_abundance"] = _take(v.set_abundance, 2 * L, np.float64, (L, 2))
        else:
            for name in ("set_count", "cluster_noise_count", "set_first", "set_second", "set_posterior", "set_abundance"):
                out[name] = None
        return out, h
    except BaseException:
        hip.lib().rpvg_hip_subset_em_free(h)
        raise


def nested_subset_em_kept(groups, unit_cluster, column_counts, min_rel_likelihood: float, min_hap_prob: float, **kwargs):
    """The diploid call with its device block kept: (host view, EstimatesPart that owns the result)."""
    view, h = nested_subset_em(groups, column_counts, min_rel_likelihood, min_hap_prob, keep=True, **kwargs)
    return view, _part_or_free(h, unit_cluster)


def nested_full_subset_em_kept(groups, unit_cluster, group_size: int, log_freq, min_hap_prob: float, **kwargs):
    """rpvg_hip_nested_full_subset_em with its device block kept: (host view, EstimatesPart that owns the result)."""
    with _Kept(groups.ctx, True):
        view, h = groups.nested_full_subset_em(group_size, log_freq, min_hap_prob, keep_handle=True, **kwargs)
    return view, _part_or_free(h, unit_cluster)


def nested_independent_subset_em_kept(groups, unit_cluster, matrix_off, group_size: int, min_hap_prob: float, generator_words, **kwargs):
    """rpvg_hip_nested_independent_subset_em with its device block kept: (host view, EstimatesPart that owns the result)."""
    with _Kept(groups.ctx, True):
        view, h = groups.nested_independent_subset_em(matrix_off, group_size, min_hap_prob, generator_words, keep_handle=True, **kwargs)
    return view, _part_or_free(h, unit_cluster)


def _part_or_free(h, unit_cluster):
    try:
        return EstimatesPart.from_result(h, unit_cluster)
    except BaseException:
        hip.lib().rpvg_hip_subset_em_free(h)
        raise


# ---- the harness: the estimator's resident route --------------------------------------------------------------------------------

def _harness():
    from . import engine
    L = engine.lib()
    L.rpvg_amd_run_resident.restype = C.c_void_p
    L.rpvg_amd_run_resident.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p]
    L.rpvg_amd_resident_estimates_get.argtypes = [C.c_void_p, C.POINTER(CEstimatesFlat)]
    L.rpvg_amd_resident_estimates_free.argtypes = [C.c_void_p]
    L.rpvg_amd_resident_estimates_kept_bytes.restype = C.c_uint32
    L.rpvg_amd_resident_estimates_kept_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
    L.rpvg_amd_estimates_table_build_resident.restype = C.c_void_p
    L.rpvg_amd_estimates_table_build_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    return L, engine


class HarnessResidentEstimates(HandleOwner):
    """What run_resident returns: the host class ResidentEstimates (rpvg_amd/host/estimates_table.hpp) behind a handle."""

    def __init__(self, handle):
        self.handle = handle

    def get(self) -> FlatEstimates:
        L, eng = _harness()
        flat = CEstimatesFlat()
        if L.rpvg_amd_resident_estimates_get(self.handle, C.byref(flat)) != 0:
            raise hip.EngineError(f"resident estimates get failed: {eng._err()}")
        return flat_from_c(flat)

    def table(self, engine, prepared, ploidy: int) -> HarnessTable:
        """The estimates table built from the resident estimates with on_device = 1 (no flattening); a HarnessTable like the one of
        the containers: view(), tpm(), write() and the text entry points take it."""
        L, eng = _harness()
        handle = L.rpvg_amd_estimates_table_build_resident(engine.handle, self.handle, prepared.handle, ploidy)
        if not handle:
            raise hip.EngineError(f"resident estimates table failed: {eng._err()}")
        return HarnessTable.from_handle(handle)

    def kept_block_bytes(self):
        """The device memory the kept block of every lane's nested call held (the calls' capacities), in bytes."""
        L, _ = _harness()
        out = (C.c_uint64 * 64)()
        n = L.rpvg_amd_resident_estimates_kept_bytes(self.handle, out, 64)
        return [int(out[i]) for i in range(min(n, 64))]

    def _release(self):
        _harness()[0].rpvg_amd_resident_estimates_free(self.handle)


def run_resident(engine, model: str, params, prepared) -> Optional[HarnessResidentEstimates]:
    """NestedPathAbundanceEstimator::estimateBatchResident on a prepared batch: the resident estimates, or None when the route is not
    taken (the caller then runs the engine as before).  Raises EngineError when the route fails."""
    L, eng = _harness()
    handle = L.rpvg_amd_run_resident(engine.handle, model.encode(), C.byref(params), prepared.handle)
    if not handle:
        message = eng._err()
        if message:
            raise hip.EngineError(f"run_resident failed: {message}")
        return None
    return HarnessResidentEstimates(handle)
