"""The device index (rmi_lookup.hip) on the hand-built models of tests/designed_index.py: rows that force every search path --
window edges, gallops of every length in both directions and into both ends of the key array, clamped windows, the last line of
keys, runs of equal keys, key sets shorter than a line, keys above 2^63, f64 keys around zero, NaN and infinite queries -- and
hand-set roots for every root function.  Both search variants, every query, bit-exact integers:

  search(q)            == (keys < q).sum()
  last_stats.fallbacks == the count of |guess - lower bound| > err, guess and err from the emitted C++ (tests/lookup_driver.py)
  last_stats.root_oob  == the designed count of queries the emitted C++ leaves undefined
  lookup(q)            == the emitted C++ wherever it is defined, the documented clamp (include/rmi_hip.h) where it is not

tests/test_designed_index_cpu.py holds the census: that the sets reach the classes they were built for."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from rmi_amd import train
from rmi_amd.index import DeviceIndex

from tests import designed_index as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KTS = X.KTS
VARIANTS = ("lane", "coop")


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """key type -> {case name: (case, (guess, err, undefined) of the emitted C++)}; one driver a model"""
    cache = {}

    def get(kt):
        if kt not in cache:
            cases = X.driver_cases(kt)
            drv = X.compile_drivers(cases, tmp_path_factory.mktemp(f"drv_{kt}"))
            cache[kt] = {c.name: (c, drv[c.name].run(c.queries)) for c in cases}
        return cache[kt]
    return get


def _index(tr, c):
    return DeviceIndex.from_arrays(tr, c.root, c.leaf_kind, c.params, c.errors, c.n, dtype=c.dtype)


def _reference(c, ref):
    """(guess, err, undefined) per query: the emitted C++; on the queries it leaves undefined the clamped leaf the header documents,
    from the hand-set rows"""
    g, e, undef = ref
    assert np.array_equal(undef, c.oob), c.name
    g = np.where(undef, X.design_guess(c), g)
    e = np.where(undef, X.design_err(c), e) if c.errors is not None else np.zeros(len(g), dtype=np.uint64)
    return g, e, undef


def _check_lookup(ix, c, ref):
    g, e, undef = _reference(c, ref)
    gl, el = ix.lookup(c.queries)
    assert ix.last_stats.root_oob == int(c.oob.sum()) and ix.last_stats.queries == len(c.queries), c.name
    bad = np.flatnonzero(gl != g)
    assert bad.size == 0, (c.name, bad.size, c.queries[bad[:5]], gl[bad[:5]], g[bad[:5]], undef[bad[:5]])
    if c.errors is None:
        assert el is None
    else:
        assert np.array_equal(el, e), c.name


def _check_search(ix, c, keys, ref):
    g, e, undef = _reference(c, ref)
    lb = X.lower_bound(keys, c.queries)
    want_fb = int(X.expected_fallbacks(g, e, lb).sum())
    for variant in VARIANTS:
        ix.set_variant(variant)
        pos = ix.search(c.queries)
        st = ix.last_stats
        bad = np.flatnonzero(pos != lb)
        assert bad.size == 0, (c.name, variant, bad.size, c.queries[bad[:5]], pos[bad[:5]], lb[bad[:5]], g[bad[:5]], e[bad[:5]])
        assert (st.queries, st.fallbacks, st.root_oob) == (len(c.queries), want_fb, int(c.oob.sum())), (c.name, variant)
        assert ix.search(c.queries, positions=False) is None
        st = ix.last_stats
        assert (st.queries, st.fallbacks, st.root_oob) == (len(c.queries), want_fb, int(c.oob.sum())), (c.name, variant, "count only")
    ix.set_variant("lane")
    return want_fb


@pytest.mark.parametrize("kt", KTS)
def test_search_sets(drivers, kt):
    """main A / B / C / N, the high keys (u64, u32), the f64 keys around zero (with the NaN query: position 0, one root_oob, no
    fallback)"""
    dr = drivers(kt)
    tr = train.Trainer()
    resident = None
    for c in X.search_cases(kt):
        if resident is not c.keys and (resident is None or not np.array_equal(resident, c.keys)):
            tr.set_keys(c.keys)
            resident = c.keys
        ix = _index(tr, c)
        fb = _check_search(ix, c, c.keys, dr[c.name][1])
        assert 0 < fb < len(c.queries)
        _check_lookup(ix, c, dr[c.name][1])
        ix.close()
    tr.close()


@pytest.mark.parametrize("kt", KTS)
def test_short_key_sets(drivers, kt):
    """n = 1, 2, LN - 1 .. 2 LN + 1 keys: one trainer, set_keys per n and rotation; guesses 0, n / 2, n - 1 and the sweep, err 0, 1, LN,
    n and 2^64 - 1 (the leaf is the query's low byte)"""
    dr = drivers(kt)
    tr = train.Trainer()
    for n in X.short_ns(kt):
        c, ref = dr[f"short-{n}-{kt}"]
        ix = None
        for rot in range(X.SHORT_COMBOS):
            keys = X.short_keys(kt, n, rot)
            tr.set_keys(keys)
            ix = ix or _index(tr, c)
            _check_search(ix, c, keys, ref)
        _check_lookup(ix, c, ref)
        assert ix.verify()[0] == n
        ix.close()
    tr.close()


@pytest.mark.parametrize("kt", KTS)
def test_lookup_sets(drivers, kt):
    """every root function on hand-set parameters: guess and err bit-identical to the emitted C++ wherever it is defined; exactly
    the designed queries are undefined, and there the leaf is the documented clamp"""
    dr = drivers(kt)
    tr = train.Trainer(np.arange(1, 100, dtype=X.DT[kt]))
    for c in X.lookup_sets(kt):
        ix = _index(tr, c)
        _check_lookup(ix, c, dr[c.name][1])
        ix.close()
    tr.close()


def test_nan_predictions_have_the_documented_result():
    """NaN leaf predictions give guess 0 and are not counted; a NaN root prediction is leaf 0 and one root_oob.  The emitted FCLAMP
    is undefined on a NaN: there is no driver here."""
    tr = train.Trainer(np.arange(1000, dtype=np.float64))
    for c in X.nan_cases():
        ix = _index(tr, c)
        g, e = ix.lookup(c.queries)
        assert np.array_equal(g, X.design_guess(c)) and np.array_equal(e, X.design_err(c)), c.name
        assert ix.last_stats.root_oob == int(c.oob.sum()), c.name
        assert np.all(g[np.isnan(X.leaf_pred(c))] == 0)
        # search: the lower bound all the same, and a NaN query answers 0 (no key is < NaN)
        lb = X.lower_bound(np.arange(1000, dtype=np.float64), c.queries)
        for variant in VARIANTS:
            ix.set_variant(variant)
            assert np.array_equal(ix.search(c.queries), lb), (c.name, variant)
            assert ix.last_stats.fallbacks == int(X.expected_fallbacks(g, e, lb).sum()) and ix.last_stats.root_oob == int(c.oob.sum())
        ix.close()
    tr.close()


@pytest.mark.parametrize("kt", KTS)
def test_verify_counts_the_designed_outside_keys(kt):
    tr = train.Trainer(X.main_keys(kt).keys)
    for outside in ("0", "1", "n"):
        c = X.verify_case(kt, outside)
        ix = _index(tr, c)
        for variant in VARIANTS:
            ix.set_variant(variant)
            assert ix.verify() == (c.n, {"0": 0, "1": 1, "n": c.n}[outside]), (outside, variant)
        ix.close()
    tr.close()


@functools.lru_cache(maxsize=None)
def _cu_count() -> int:
    """the device's, from a process of its own (torch brings a HIP runtime of its own)"""
    r = subprocess.run([sys.executable, "-c", "import torch; print('CUS', torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CUS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return int(r.stdout.split("CUS")[1].split()[0])


@pytest.mark.parametrize("kt", KTS)
def test_batch_shapes(drivers, kt):
    """batches of 1 .. 257 queries, and one of more than two trips of the grid-stride loop, fallbacks spread through it"""
    c, (g, e, undef) = drivers(kt)[f"main-C-{kt}"]
    tr = train.Trainer(c.keys)
    ix = _index(tr, c)
    for k, nq in enumerate(X.BATCH_SIZES):
        at = slice(1000 * k, 1000 * k + nq)
        _check_search(ix, c.with_queries(c.queries[at], c.qleaf[at], c.oob[at]), c.keys, (g[at], e[at], undef[at]))
    nq = X.big_batch_size(_cu_count())
    assert nq % 8 != 0
    big = X.tiled(c, nq)
    reps = -(-nq // len(g))
    fb = _check_search(ix, big, c.keys, (np.tile(g, reps)[:nq], np.tile(e, reps)[:nq], np.tile(undef, reps)[:nq]))
    assert fb > nq // 100
    ix.close()
    tr.close()


def test_torch_entry():
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); import torch; torch.cuda.init(); "
            f"from tests import test_gpu_index_designed as m; m._body_torch_entry(); print('body ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "body ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _body_torch_entry():
    """torch tensors in, torch tensors out, on the f64 keys around zero (NaN and infinite queries) and the high u64 keys"""
    import torch
    for c in (X.f64_case(), X.high_case("u64")):
        tr = train.Trainer(c.keys)
        ix = _index(tr, c)
        lb = X.lower_bound(c.keys, c.queries)
        want_fb = int(X.expected_fallbacks(X.design_guess(c), X.design_err(c), lb).sum())
        qt = torch.from_numpy(c.queries if c.kt == "f64" else c.queries.view(np.int64)).to("cuda:0")
        for variant in VARIANTS:
            ix.set_variant(variant)
            pt = ix.search(qt)
            assert isinstance(pt, torch.Tensor) and pt.device == qt.device
            assert np.array_equal(pt.cpu().numpy().view(np.uint64), lb), (c.name, variant)
            assert (ix.last_stats.fallbacks, ix.last_stats.root_oob) == (want_fb, int(c.oob.sum()))
        gt, et = ix.lookup(qt)
        assert np.array_equal(gt.cpu().numpy().view(np.uint64), X.design_guess(c)) and np.array_equal(et.cpu().numpy().view(np.uint64), X.design_err(c))
        tr.close()
