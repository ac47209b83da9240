"""Querying a trained RMI on the device (include/rmi_hip.h, "querying a trained RMI on the device").

``DeviceIndex`` holds a copy of a two-layer model in device memory and answers, for a batch of query keys:

* ``lookup(q)``  -> ``(guess, err)``, bit-identical to the emitted C++ ``lookup(key, &err)`` (rmi_amd/codegen.py);
* ``search(q)``  -> ``pos = lower_bound(keys, q)`` over the trainer's resident keys (``np.searchsorted(keys, q, "left")``);
* ``verify()``   -> ``(checked, outside)``: the reference's acceptance loop over every resident key.

``search`` compares with ``<``, as ``std::lower_bound`` over the emitted code's keys would: ``pos = (keys < q).sum()``.  That is
``np.searchsorted`` for every query but a NaN: no key is ``< NaN``, so a NaN query answers 0 (numpy sorts NaN behind every key and
answers n); it reads leaf 0, guesses 0, and counts as one ``root_oob`` and no fallback.

Queries are a numpy array (staged to the device through the trainer's context) or a torch tensor on the trainer's device
(used in place through ``data_ptr()``); the outputs come back in the same kind (torch outputs as int64 tensors on the device;
torch brings a HIP runtime of its own, which must be the first one the process initialises).  The
counters of the last call are in ``last_stats``: queries, fallbacks (lower bound outside ``[guess - err, guess + err]``),
root_oob (raw root prediction outside ``[0, L)`` or NaN, see the header) and the kernel's device time.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .train import KEY_F64, KEY_U32, KEY_U64, Model, RMIError, Trainer, TrainedRMI, _check

RMI_ERR_BAD_ARG = -6
RMI_ERR_UNSUPPORTED_MODEL = -11
VARIANTS = {"lane": 0, "coop": 1}
_NP = {KEY_U64: np.dtype(np.uint64), KEY_U32: np.dtype(np.uint32), KEY_F64: np.dtype(np.float64)}
_NP_DT = {v: k for k, v in _NP.items()}


def _torch_key_dtype(t) -> int:
    import torch
    m = {torch.int64: KEY_U64, torch.int32: KEY_U32, torch.float64: KEY_F64}
    for name, dt in (("uint64", KEY_U64), ("uint32", KEY_U32)):
        if hasattr(torch, name):
            m[getattr(torch, name)] = dt
    if t.dtype not in m:
        raise TypeError(f"query tensor of dtype {t.dtype}: expected 64-bit or 32-bit integers or float64")
    return m[t.dtype]


def _ctx_dtype(trainer: Trainer) -> int:
    trainer.wait_keys()
    ptr, n, dt = C.c_void_p(), C.c_uint64(), C.c_int()
    _check(trainer._lib.rmi_hip_key_buffer(trainer._h, C.byref(ptr), C.byref(n), C.byref(dt)), trainer._h)
    return int(dt.value)


class DeviceIndex:
    """A device index over the resident keys of ``trainer`` (see the module docstring).  Build it with
    ``from_trained`` or ``from_arrays``; ``close()`` frees it (closing the trainer frees it too)."""

    def __init__(self, trainer: Trainer, handle: C.c_void_p, dtype: int, num_rows: int, has_errors: bool):
        self._trainer = trainer
        self._lib = trainer._lib
        self._h = handle
        self.dtype = dtype
        self.num_rows = int(num_rows)
        self.has_errors = bool(has_errors)
        self.last_stats = None

    # ---- construction ----
    @classmethod
    def from_trained(cls, rmi: TrainedRMI) -> "DeviceIndex":
        """From a training result whose trainer is still open.  The rows are copied device to device while the trainer's
        arrays are the result's; after a later training, from the arrays the result has downloaded (``materialize()``)."""
        if getattr(rmi, "cache_fix", None) is not None:
            raise RMIError(RMI_ERR_UNSUPPORTED_MODEL, "bounded RMIs (cache_fix) are not indexed")
        tr = rmi._trainer
        if tr is None or tr._h is None:
            raise RuntimeError("the trainer of this result is closed or unknown: use DeviceIndex.from_arrays with a trainer")
        h = C.c_void_p()
        with tr._ctx_lock:
            rc = tr._lib.rmi_hip_index_from_result(tr._h, C.byref(rmi.root._c()), int(rmi.generation), C.byref(h))
        if rc == RMI_ERR_BAD_ARG and "params" in rmi._cache and "errors" in rmi._cache:
            return cls.from_arrays(tr, rmi.root, rmi.leaf_kind, rmi.leaf_params, rmi.last_layer_max_l1s, rmi.num_rmi_rows)
        _check(rc, tr._h)
        return cls(tr, h, _ctx_dtype(tr), rmi.num_rmi_rows, True)

    @classmethod
    def from_arrays(cls, trainer: Trainer, root: Model, leaf_kind: int, params, errors, num_rows: int,
                    dtype=None) -> "DeviceIndex":
        """From host arrays: ``params`` [L, ppl] f64, ``errors`` [L] u64 or None (a model without error rows: its search
        gallops from the guess), ``num_rows`` the key count the model was trained on.  dtype: the key dtype (default: the
        trainer's)."""
        params = np.ascontiguousarray(params, dtype=np.float64)
        L = params.shape[0]
        if errors is not None:
            errors = np.ascontiguousarray(errors, dtype=np.uint64)
            if errors.shape != (L,):
                raise ValueError("errors must have one entry per leaf")
        dt = _NP_DT[np.dtype(dtype)] if dtype is not None else _ctx_dtype(trainer)
        table = None
        if root.is_radix_table:
            if root.table is None:
                raise ValueError("a radix-table root needs its hint table (Model.table)")
            table = np.ascontiguousarray(root.table, dtype=np.uint32)
        h = C.c_void_p()
        with trainer._ctx_lock:
            rc = trainer._lib.rmi_hip_index_from_arrays(
                trainer._h, C.byref(root._c()), int(leaf_kind), L, int(num_rows), dt, params.ctypes.data,
                None if errors is None else errors.ctypes.data, None if table is None else table.ctypes.data,
                0 if table is None else table.size, C.byref(h))
        _check(rc, trainer._h)
        return cls(trainer, h, dt, num_rows, errors is not None)

    # ---- queries ----
    def _alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _check(self._lib.rmi_hip_device_alloc(self._trainer._h, int(nbytes), C.byref(p)), self._trainer._h)
        return int(p.value)

    def _call(self, q, outputs: int, fn):
        """Runs fn(query pointer, count, dtype, output pointers) and returns the outputs in the kind of q: a numpy array is
        staged through the context (device buffers of its own HIP runtime), a torch tensor on the device is used in place
        and gets torch int64 tensors back (torch must then be the first to have initialised the device in the process)."""
        try:
            import torch
        except ImportError:                                           # (numpy callers need no torch)
            torch = None
        if torch is not None and isinstance(q, torch.Tensor):
            if not q.is_cuda or not q.is_contiguous():
                raise TypeError("query tensors must be contiguous and on the device")
            torch.cuda.current_stream(q.device).synchronize()       # (the context runs on its own stream)
            n = q.numel()
            outs = [torch.empty(max(n, 1), dtype=torch.int64, device=q.device) for _ in range(outputs)]
            fn(q.data_ptr(), n, _torch_key_dtype(q), [o.data_ptr() for o in outs])
            return [o[:n] for o in outs]
        a = np.ascontiguousarray(q)
        if a.dtype not in _NP_DT:
            raise TypeError(f"queries of dtype {a.dtype}: expected uint64, uint32 or float64")
        n = a.size
        bufs = []
        try:
            dq = self._alloc(a.nbytes)
            bufs.append(dq)
            _check(self._lib.rmi_hip_copy(self._trainer._h, dq, a.ctypes.data, a.nbytes), self._trainer._h)
            douts = [self._alloc(8 * n) for _ in range(outputs)]
            bufs += douts
            fn(dq, n, _NP_DT[a.dtype], douts)
            res = []
            for d in douts:
                h = np.empty(n, dtype=np.uint64)
                _check(self._lib.rmi_hip_copy(self._trainer._h, h.ctypes.data, d, 8 * n), self._trainer._h)
                res.append(h)
            return res
        finally:
            for b in bufs:
                self._lib.rmi_hip_device_free(self._trainer._h, b)

    def _live(self):
        if self._h is None or self._trainer._h is None:
            raise RuntimeError("this index is closed (or its trainer is)")

    def lookup(self, q):
        """-> (guess, err): err is None for a model without error rows."""
        self._live()
        st = _lib.SearchStats()

        def fn(ptr, n, dt, outs):
            with self._trainer._ctx_lock:
                rc = self._lib.rmi_hip_index_lookup(self._trainer._h, self._h, ptr, n, dt, outs[0],
                                                    outs[1] if self.has_errors else None, C.byref(st))
            _check(rc, self._trainer._h)
        res = self._call(q, 2 if self.has_errors else 1, fn)
        self.last_stats = st
        return res[0], (res[1] if self.has_errors else None)

    def search(self, q, positions: bool = True):
        """-> lower bounds of the queries among the resident keys (None with positions=False: counters only)."""
        self._live()
        st = _lib.SearchStats()

        def fn(ptr, n, dt, outs):
            with self._trainer._ctx_lock:
                rc = self._lib.rmi_hip_index_search(self._trainer._h, self._h, ptr, n, dt, outs[0] if outs else None, C.byref(st))
            _check(rc, self._trainer._h)
        res = self._call(q, 1 if positions else 0, fn)
        self.last_stats = st
        return res[0] if positions else None

    def verify(self):
        """-> (checked, outside): the reference's acceptance loop over every resident key, on the device."""
        self._live()
        checked, outside = C.c_uint64(), C.c_uint64()
        with self._trainer._ctx_lock:
            rc = self._lib.rmi_hip_index_verify(self._trainer._h, self._h, C.byref(checked), C.byref(outside))
        _check(rc, self._trainer._h)
        return int(checked.value), int(outside.value)

    def set_variant(self, variant: str):
        """"lane" (default: one query per lane) or "coop" (eight lanes per query)."""
        self._live()
        _check(self._lib.rmi_hip_index_set_variant(self._h, VARIANTS[variant]))

    def close(self):
        if getattr(self, "_h", None) is not None:
            if self._trainer._h is not None:              # (rmi_hip_destroy has freed it otherwise)
                self._lib.rmi_hip_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
