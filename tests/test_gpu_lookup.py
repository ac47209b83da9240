"""The device index (rmi_amd/index.py, rmi_lookup.hip): lookup bit-identical to the emitted C++, search equal to
np.searchsorted for every query, verify equal to the reference's acceptance loop, index lifetime, full-size runs, interfaces."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from rmi_amd import cli, datagen as dg, train
from rmi_amd.index import DeviceIndex

from . import lookup_driver as ld

pytestmark = pytest.mark.gpu


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch():
    import torch
    return torch


def _isolated(body: str):
    """Runs _body_<body>() in a process of its own: torch brings its own HIP runtime, which must be the first one the
    process initialises (the tests before this one have initialised the library's)."""
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); import torch; torch.cuda.init(); "
            f"from tests import test_gpu_lookup as m; m._body_{body}(); print('body ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "body ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# root x leaf x dtype, with and without error rows (radix26/28 tables are 256 MB / 1 GB on the host: left out)
SWEEP = [
    ("uniform_u64", "linear", "linear", 1024, True),
    ("books_u64", "linear_spline", "cubic", 512, False),
    ("dups_u64", "cubic", "linear", 4096, True),
    ("uniform_u32", "radix", "linear_spline", 1024, True),
    ("uniform_u64", "radix", "linear", 1024, False),
    ("uniform_f64", "linear", "linear", 512, True),
    ("uniform_f64", "normal", "linear_spline", 256, True),
    ("uniform_f64", "loglinear", "cubic", 256, False),
    ("books_u64", "radix18", "linear", 4096, True),
    ("dups_u32", "radix8", "linear_spline", 256, True),
    ("uniform_u64", "radix22", "cubic", 512, True),
    ("uniform_u64", "bradix", "linear", 1024, True),
    ("dups_u32", "bradix", "linear_spline", 300, False),
    ("uniform_u64", "normal", "linear", 1024, True),
    ("books_u64", "loglinear", "linear", 512, True),
    ("uniform_u64", "robust_linear", "robust_linear", 2048, True),
    ("uniform_u32", "cubic", "cubic", 256, True),
    ("uniform_u32", "linear", "robust_linear", 1024, False),
    ("clustered_u64", "linear", "linear_spline", 2048, True),
]


def _driver_rmi(rmi):
    root = rmi.root
    return ld.as_rmi(root, rmi.leaf_kind, rmi.params_per_leaf, rmi.branching_factor, rmi.num_rmi_rows,
                     rmi.leaf_params, rmi.last_layer_max_l1s)


@pytest.mark.parametrize("gen,root,leaf,L,with_err", SWEEP)
def test_lookup_matches_emitted_cpp_and_search_is_exact(tmp_path, gen, root, leaf, L, with_err):
    keys = dg.GENERATORS[gen](200_000)
    tr = train.Trainer(keys)
    rmi = tr.train(f"{root},{leaf}", L)
    rmi.materialize()
    if with_err:
        ix = rmi.index()
    else:
        ix = DeviceIndex.from_arrays(tr, rmi.root, rmi.leaf_kind, rmi.leaf_params, None, len(keys))
    drv = ld.Driver(_driver_rmi(rmi), keys.dtype, tmp_path, with_errors=with_err)
    for name, q in ld.query_sets(keys, seed=L).items():
        g_ref, e_ref, undef = drv.run(q)
        g, e = ix.lookup(q)
        assert ix.last_stats.root_oob == int(undef.sum()), name
        ok = ~undef
        assert np.array_equal(g[ok], g_ref[ok]), (name, np.flatnonzero(g[ok] != g_ref[ok])[:5])
        if with_err:
            assert np.array_equal(e[ok], e_ref[ok]), name
        else:
            assert e is None
        pos = ix.search(q)
        assert np.array_equal(pos, np.searchsorted(keys, q, side="left").astype(np.uint64)), name
        if name == "keys" and with_err:
            assert ix.last_stats.fallbacks == 0
            perm = np.random.default_rng(1).permutation(keys)
            pos = ix.search(perm)
            assert ix.last_stats.fallbacks == 0
            assert np.array_equal(pos, np.searchsorted(keys, perm, side="left").astype(np.uint64))
    # the cooperative variant answers the same
    q = np.concatenate(list(ld.query_sets(keys, seed=3).values()))
    ix.search(q, positions=False)
    lane_fallbacks = ix.last_stats.fallbacks
    ix.set_variant("coop")
    assert np.array_equal(ix.search(q), np.searchsorted(keys, q, side="left").astype(np.uint64))
    assert ix.last_stats.fallbacks == lane_fallbacks
    ix.close()
    tr.close()


@pytest.mark.parametrize("gen,spec,L", [("books_u64", "linear,linear", 1024), ("dups_u32", "cubic,linear_spline", 512),
                                        ("uniform_f64", "linear,cubic", 256)])
def test_verify_agrees_with_the_oracle_and_finds_violations(oracle, tmp_path, gen, spec, L):
    keys = dg.GENERATORS[gen](150_000)
    tr = train.Trainer(keys)
    rmi = tr.train(spec, L).materialize()
    o = oracle.train_two_layer(*spec.split(","), keys, L)
    assert oracle.check_lookup_property(o, keys)[0] == 0
    ix = rmi.index()
    assert ix.verify() == (len(keys), 0)
    # the bound of some leaves lowered to one below the largest |guess - lower_bound| of their keys (the trained bounds
    # can be wider than that: lower-bound widening), exactly the keys the emitted C++ then misses
    r = _driver_rmi(rmi)
    g, _, undef = ld.Driver(r, keys.dtype, tmp_path / "a").run(keys) if (tmp_path / "a").mkdir() is None else None
    assert not undef.any()
    lb = np.searchsorted(keys, keys, side="left").astype(np.int64)
    diff = np.abs(g.astype(np.int64) - lb)
    starts = rmi.leaf_starts.astype(np.int64)
    nonempty = np.flatnonzero(starts[1:] > starts[:-1])
    tight = np.maximum.reduceat(diff, starts[nonempty])
    err = rmi.last_layer_max_l1s.copy()
    sel = nonempty[tight > 0][::3]
    err[sel] = tight[tight > 0][::3] - 1
    bad_ix = DeviceIndex.from_arrays(tr, rmi.root, rmi.leaf_kind, rmi.leaf_params, err, len(keys))
    r.last_layer_max_l1s = err
    g2, e, _ = ld.Driver(r, keys.dtype, tmp_path / "b").run(keys) if (tmp_path / "b").mkdir() is None else None
    assert np.array_equal(g, g2)
    expect = int((diff > e.astype(np.int64)).sum())
    assert expect > 0
    assert bad_ix.verify() == (len(keys), expect)
    bad_ix.search(keys, positions=False)
    assert bad_ix.last_stats.fallbacks == expect
    tr.close()


def test_index_lifetime():
    keys = dg.uniform_u64(300_000)
    tr = train.Trainer(keys)
    a = tr.train("linear,linear", 2048).materialize()
    ix = a.index()
    q = np.concatenate(list(ld.query_sets(keys, seed=5).values()))
    g0, e0 = ix.lookup(q)
    p0 = ix.search(q)
    rows = a.rows.copy()
    ix2 = DeviceIndex.from_arrays(tr, a.root, a.leaf_kind, a.leaf_params, a.last_layer_max_l1s, len(keys))
    g2, e2 = ix2.lookup(q)
    assert np.array_equal(g0, g2) and np.array_equal(e0, e2) and np.array_equal(ix2.search(q), p0)
    # search leaves the context's arrays alone
    got = np.empty_like(rows)
    assert tr._lib.rmi_hip_download_rows(tr._h, got.ctypes.data) == 0
    assert np.array_equal(got, rows)
    b = tr.train("cubic,linear_spline", 512)                       # another configuration on the same context
    g1, e1 = ix.lookup(q)
    assert np.array_equal(g0, g1) and np.array_equal(e0, e1) and np.array_equal(ix.search(q), p0)
    got = np.empty(512 * 24, dtype=np.uint8)
    assert tr._lib.rmi_hip_download_rows(tr._h, got.ctypes.data) == 0
    assert np.array_equal(got, b.rows)
    # the result of the first training is still indexable from its downloaded arrays
    ix3 = a.index()
    assert np.array_equal(ix3.lookup(q)[0], g0)
    tr.close()                                                     # frees the indexes still alive
    ix.close(); ix2.close(); ix3.close()


class _DevArray:
    """A device buffer of the context as a torch tensor (no copy)."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def _key_tensor(tr):
    import ctypes as C
    torch = _torch()
    ptr, n, dt = C.c_void_p(), C.c_uint64(), C.c_int()
    assert tr._lib.rmi_hip_key_buffer(tr._h, C.byref(ptr), C.byref(n), C.byref(dt)) == 0
    return torch.as_tensor(_DevArray(ptr.value, n.value, "<i8" if dt.value != 1 else "<i4"), device="cuda:0")


def test_full_size_m():
    _isolated("full_size_m")


def _body_full_size_m():
    torch = _torch()
    n = 200_000_000
    tr = train.Trainer()
    tr.generate_keys("uniform", np.uint64, n)
    rmi = tr.train("linear,linear", 1 << 20)
    ix = rmi.index()
    assert ix.verify() == (n, 0)
    kt = _key_tensor(tr)
    pos = ix.search(kt)
    assert ix.last_stats.fallbacks == 0 and ix.last_stats.queries == n
    assert bool((pos == torch.arange(n, device="cuda:0")).all())
    del pos, kt
    ix.close()
    tr.close()
    torch.cuda.empty_cache()


def test_full_size_duplicates():
    _isolated("full_size_duplicates")


def _body_full_size_duplicates():
    torch = _torch()
    n = 1 << 25
    tr = train.Trainer()
    tr.generate_keys("dups", np.uint64, n)
    rmi = tr.train("linear,linear", 1 << 18)
    ix = rmi.index()
    assert ix.verify() == (n, 0)
    kt = _key_tensor(tr)
    pos = ix.search(kt)
    assert ix.last_stats.fallbacks == 0
    s = kt ^ torch.iinfo(torch.int64).min                       # u64 order as int64 order
    first = torch.searchsorted(s, s, side="left")
    assert bool((pos == first).all())
    assert int((first != torch.arange(n, device="cuda:0")).sum()) > 0   # there are duplicates
    tr.close()


def test_torch_in_torch_out():
    _isolated("torch_in_torch_out")


def _body_torch_in_torch_out():
    torch = _torch()
    keys = dg.uniform_u64(100_000)
    tr = train.Trainer(keys)
    ix = tr.train("linear,linear", 512).index()
    q = np.concatenate(list(ld.query_sets(keys, seed=9).values()))
    want = np.searchsorted(keys, q, side="left").astype(np.uint64)
    qt = torch.from_numpy(q.view(np.int64)).to("cuda:0")
    pt = ix.search(qt)
    assert isinstance(pt, torch.Tensor) and pt.device == qt.device
    assert np.array_equal(pt.cpu().numpy().view(np.uint64), want)
    g, e = ix.lookup(qt)
    gn, en = ix.lookup(q)
    assert np.array_equal(g.cpu().numpy().view(np.uint64), gn) and np.array_equal(e.cpu().numpy().view(np.uint64), en)
    assert ix.search(qt[:0]).numel() == 0
    tr.close()


def test_interfaces_and_errors():
    keys = dg.uniform_u64(100_000)
    tr = train.Trainer(keys)
    rmi = tr.train("linear,linear", 512)
    ix = rmi.index()
    q = np.concatenate(list(ld.query_sets(keys, seed=9).values()))
    want = np.searchsorted(keys, q, side="left").astype(np.uint64)
    # numpy in, numpy out
    p = ix.search(q)
    assert isinstance(p, np.ndarray) and np.array_equal(p, want)
    # nq == 0
    assert ix.search(np.array([], dtype=np.uint64)).size == 0
    assert ix.lookup(np.array([], dtype=np.uint64))[0].size == 0
    # dtype mismatch
    with pytest.raises(train.RMIError) as ei:
        ix.search(q.astype(np.uint32))
    assert ei.value.code == -6
    with pytest.raises(train.RMIError) as ei:
        ix.lookup(q.astype(np.float64))
    assert ei.value.code == -6
    # key-count mismatch
    other = DeviceIndex.from_arrays(tr, rmi.root, rmi.leaf_kind, rmi.leaf_params, rmi.last_layer_max_l1s, len(keys) + 1)
    with pytest.raises(train.RMIError) as ei:
        other.search(q)
    assert ei.value.code == -6
    with pytest.raises(train.RMIError) as ei:
        other.verify()
    assert ei.value.code == -6
    # bounded RMIs are not indexed
    bounded = tr.train_bounded("linear,linear", 64, 8)
    with pytest.raises(train.RMIError) as ei:
        bounded.index()
    assert ei.value.code == -11
    tr.close()


def test_cli_verify(tmp_path):
    keys = dg.books_u64(200_000)
    kfile = str(tmp_path / "books_200k_uint64")
    dg.write_keys(kfile, keys)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = cli.main([kfile, "rmi", "linear,linear", "1024", "--no-code", "--verify"])
    assert rc == 0
    assert f"checked {len(keys)} keys, 0 outside the bound" in out.getvalue()
    out2 = io.StringIO()
    with contextlib.redirect_stdout(out2):
        assert cli.main([kfile, "rmi", "linear,linear", "1024", "--no-code"]) == 0
    assert "outside the bound" not in out2.getvalue()
