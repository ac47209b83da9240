"""CPU side of the device index (no GPU): the new entry points resolve against the built library with the declared ctypes
signatures, and the batch driver of the emitted C++ that the GPU tests compare the device lookup with meets the reference's
acceptance property (|lookup(key) - lower_bound(key)| <= err) on the codegen fixtures."""
import ctypes as C

import numpy as np
import pytest

from rmi_amd import datagen as dg

from . import lookup_driver as ld

INDEX_SYMBOLS = ["rmi_hip_index_from_result", "rmi_hip_index_from_arrays", "rmi_hip_index_lookup", "rmi_hip_index_search",
                 "rmi_hip_device_alloc", "rmi_hip_device_free", "rmi_hip_copy",
                 "rmi_hip_index_verify", "rmi_hip_index_set_variant", "rmi_hip_index_destroy"]


def test_index_symbols_resolve():
    from rmi_amd import build, _lib
    build.build_hip()
    lib = _lib.load()
    decl = {s[0]: s for s in _lib.SYMBOLS}
    for name in INDEX_SYMBOLS:
        assert name in decl
        fn = getattr(lib, name)
        assert fn.argtypes == decl[name][2] and fn.restype == decl[name][1]
    assert C.sizeof(_lib.SearchStats) == 32
    from rmi_amd import index, train
    assert hasattr(train.TrainedRMI, "index") and hasattr(index.DeviceIndex, "from_arrays")


def test_index_rejects_bad_arguments_without_a_device():
    """Argument checks come before any device work: a null context or index is RMI_ERR_BAD_ARG."""
    from rmi_amd import _lib
    lib = _lib.load()
    st = _lib.SearchStats()
    assert lib.rmi_hip_index_lookup(None, None, None, 0, 0, None, None, C.byref(st)) == -6
    assert lib.rmi_hip_index_search(None, None, None, 0, 0, None, C.byref(st)) == -6
    a, b = C.c_uint64(), C.c_uint64()
    assert lib.rmi_hip_index_verify(None, None, C.byref(a), C.byref(b)) == -6
    assert lib.rmi_hip_index_set_variant(None, 0) == -6
    lib.rmi_hip_index_destroy(None)


@pytest.mark.parametrize("gen,root,leaf,L", [
    ("books_u64", "linear", "linear", 1024),
    ("dups_u64", "cubic", "linear", 4096),
    ("uniform_u32", "radix", "linear_spline", 1024),
    ("uniform_f64", "linear", "cubic", 512),
    ("books_u64", "radix18", "linear", 2048),
    ("uniform_u64", "bradix", "linear", 1024),
    ("uniform_u64", "normal", "linear_spline", 1024),
    ("books_u64", "loglinear", "linear", 512),
])
def test_driver_meets_the_acceptance_property(oracle, tmp_path, gen, root, leaf, L):
    keys = dg.GENERATORS[gen](60_000)
    o = oracle.train_two_layer(root, leaf, keys, L)
    rmi = ld.as_rmi(o.root, o.leaf_kind, o.params_per_leaf, L, len(keys), o.leaf_params, o.leaf_err)
    drv = ld.Driver(rmi, keys.dtype, tmp_path)
    g, e, undef = drv.run(keys)
    assert not undef.any()                       # the training set maps into [0, L) (else the training would have failed)
    lb = np.searchsorted(keys, keys, side="left").astype(np.int64)
    diff = np.abs(g.astype(np.int64) - lb)
    assert int((diff > e.astype(np.int64)).sum()) == 0
    # a model emitted without error rows compiles and answers the same guesses
    drv2 = ld.Driver(rmi, keys.dtype, tmp_path / "noerr", with_errors=False) if (tmp_path / "noerr").mkdir() is None else None
    g2, _, _ = drv2.run(keys)
    assert np.array_equal(g, g2)
