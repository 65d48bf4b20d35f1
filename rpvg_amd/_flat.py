"""What the Python sides of the device tables share (estimates_table.py, gibbs_table.py): a dataclass of named numpy arrays that
becomes a ctypes struct of pointers and sizes, the context handle of a Context or an Engine, and the owner of a native handle."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import hip


class FlatArrays:
    """Base of a dataclass whose fields are the arrays of a flat C input.  The subclass names them in _FIELDS ((name, dtype), ...),
    gives the ctypes struct in _C_STRUCT (pointer fields of the same names, the sizes of sizes() and on_device) and defines sizes()."""
    _FIELDS = ()
    _C_STRUCT = None

    def __post_init__(self):
        for name, dt in self._FIELDS:
            setattr(self, name, np.ascontiguousarray(getattr(self, name), dtype=dt))

    def as_c(self, device_pointers: Optional[dict] = None, **sizes):
        """Host pointers into the arrays (which must outlive the call), or the given device pointers.  sizes: num_* overrides."""
        flat = self._C_STRUCT()
        for name, value in {**self.sizes(), **sizes}.items():
            setattr(flat, name, value)
        for name, _ in self._FIELDS:
            if device_pointers is not None:
                setattr(flat, name, device_pointers[name])
            else:
                a = getattr(self, name)
                setattr(flat, name, a.ctypes.data if len(a) else None)
        flat.on_device = 0 if device_pointers is None else 1
        return flat


def ctx_handle(ctx_or_engine):
    return ctx_or_engine.handle if isinstance(ctx_or_engine, hip.Context) else ctx_or_engine._ctx()


class HandleOwner:
    """An object that owns the native object behind self.handle: free() gives it back once through the subclass's _release(),
    and so does the end of the Python object."""
    handle = None

    def _release(self):
        raise NotImplementedError

    def free(self):
        if self.handle:
            self._release()
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
