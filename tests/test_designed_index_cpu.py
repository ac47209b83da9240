"""The hand-built index models of tests/designed_index.py, without a GPU: the emitted C++ (tests/lookup_driver.py) answers every
query of every set as it was designed -- guess the hand-set G of the query's leaf, err the row's, undefined exactly the designed
queries --, and the census: from (guess, err, lower bound), reference quantities only, every class of search path a set was built
for is present, per key type and direction.  A set that stops reaching a class fails here, not on the GPU."""
import os
import re

import numpy as np
import pytest

from tests import designed as D
from tests import designed_index as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KTS = X.KTS


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


def test_the_source_still_has_the_line_and_the_group_the_sets_were_built_for():
    src = open(os.path.join(ROOT, "rmi_amd", "csrc", "rmi_lookup.hip")).read()
    for name, (rx, value) in X.SOURCE_CONSTANTS.items():
        m = set(re.findall(rx, src))
        assert m == {str(value)}, f"{name}: /{rx}/ gives {m}; the designed sets were built for {value}"
    assert D.line_keys(np.uint64) == 16 and D.line_keys(np.uint32) == 32 and D.line_keys(np.float64) == 16
    # the cap of run(): 8 blocks of 256 lanes a CU
    assert re.search(r"\* 8;\s+// 8 blocks of 4 waves per CU", src) and "dim3(256)" in src


def test_the_lower_bound_reference_is_the_count_of_smaller_keys():
    """lower_bound() is (keys < q).sum() for every query: counted for the whole f64 set around zero (NaN, +-inf, +-0.0)"""
    c = X.f64_case()
    want = np.array([(c.keys < q).sum() for q in c.queries], dtype=np.uint64)
    fast = np.searchsorted(c.keys, c.queries, side="left").astype(np.uint64)
    fast[np.isnan(c.queries)] = 0
    assert np.array_equal(X.lower_bound(c.keys, c.queries), want) and np.array_equal(fast, want)
    assert want[np.isnan(c.queries)].tolist() == [0]
    assert np.searchsorted(c.keys, np.nan) == c.n               # (numpy's own answer for NaN, which the index does not give)


@pytest.mark.parametrize("kt", KTS)
def test_design_is_what_the_emitted_code_computes(drivers, kt):
    """guess = the row of the designed leaf at the query, err = that row's, undefined = the designed queries; at least 90 % of every
    set is defined."""
    for name, (c, (g, e, undef)) in drivers(kt).items():
        assert np.array_equal(undef, c.oob), (name, np.flatnonzero(undef != c.oob)[:5], c.queries[undef != c.oob][:5])
        assert int(undef.sum()) == int(c.oob.sum())
        ok = ~undef
        assert ok.sum() >= 0.9 * len(ok), name
        want = X.design_guess(c)
        bad = np.flatnonzero(g[ok] != want[ok])
        assert bad.size == 0, (name, c.queries[ok][bad[:5]], g[ok][bad[:5]], want[ok][bad[:5]])
        if c.errors is not None:
            assert np.array_equal(e[ok], X.design_err(c)[ok]), name
    for c in X.nan_cases():
        assert np.isnan(X.leaf_pred(c)).sum() >= 2 and c.oob.sum() == (3 if "root" in c.name else 0)
        assert np.all(X.design_guess(c)[np.isnan(X.leaf_pred(c))] == 0)


def _census(c, g, e, undef):
    ok = ~undef
    q, g, e = c.queries[ok], g[ok].astype(np.int64), e[ok]
    lb = X.lower_bound(c.keys, q).astype(np.int64)
    d = lb - g
    return q, g, e, lb, d, X.expected_fallbacks(g, e, lb)


@pytest.mark.parametrize("kt", KTS)
def test_census_of_the_main_search_sets(drivers, kt):
    dt, LN = X.DT[kt], D.line_keys(X.DT[kt])
    dr = drivers(kt)
    cen = {v: _census(*((dr[f"main-{v}-{kt}"][0],) + dr[f"main-{v}-{kt}"][1])) for v in "ABCN"}
    keys = dr[f"main-A-{kt}"][0].keys
    n = len(keys)
    q, g, e, lb, d, fb = cen["A"]
    assert not dr[f"main-A-{kt}"][1][2].any()
    assert 0 < fb.sum() < len(fb) // 2 and len(q) % 8 != 0
    # window edges: the last positions that are not a fallback; the first steps out; both directions
    for ee in X.search_edges(kt):
        at = e == np.uint64(ee)
        for dd in {dd for dd in (-ee, -ee + 1, 0, ee - 1, ee) if abs(dd) <= ee}:
            assert (at & (d == dd) & ~fb).any(), ("edge", ee, dd)
        for dd in (ee + 1, ee + 2, -ee - 1, -ee - 2):
            assert (at & (d == dd) & fb).any(), ("first step out", ee, dd)
    # gallop lengths |d| - e = 2^k - 1, 2^k, 2^k + 1
    over = np.abs(d) - e.astype(np.int64)
    for k in range(1, 18):
        for x in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            assert (fb & (over == x) & (d > 0)).any() and (fb & (over == x) & (d < 0)).any(), ("gallop", k, x)
    # clamped windows
    assert (g == 0).sum() > 100 and (g == n - 1).sum() > 100
    assert len(set(e[g == 0].tolist())) >= 5 and len(set(e[g == n - 1].tolist())) >= 5
    assert ((g > 0) & (e.astype(np.float64) > g) & (e < 1000)).any() and ((g < n - 1) & (g + np.minimum(e, 1000).astype(np.int64) >= n) & (e < 1000)).any()
    for ee in (n - 1, n, n + 1, 1 << 63, X.U64MAX):
        assert (e == np.uint64(ee)).sum() >= 100 and not fb[e == np.uint64(ee)].any(), ee
    assert (fb & (g == 0) & (lb > n // 3)).any() and (fb & (g == n - 1) & (lb < 2 * n // 3)).any()     # from a clamped guess far into the array
    # the last line of keys: every lower bound n - LN + r from windows of at most LN keys (A) and of more (B)
    for v, small in (("A", True), ("B", False)):
        qv, gv, ev, lbv, dv, fbv = cen[v]
        for r in range(LN + 1):
            at = np.flatnonzero((lbv == n - LN + r) & ~fbv)
            assert at.size, (v, r)
            wl = []
            for i in at[:4]:
                gi, ei = int(gv[i]), int(ev[i])
                a, b = (gi - ei if gi > ei else 0), (n if ei >= n - gi else gi + ei)
                wl.append((b + 1 if b < n else n) - (a - 1 if a > 0 else 0))
            assert all(w <= LN for w in wl) if small else all(w > LN for w in wl), (v, r, wl)
    # ... and the batch of loads moved left, counted from the restatement of the kernel's control flow
    qv, gv, ev, lbv, dv, fbv = cen["A"]
    moved = 0
    kl = keys.tolist()
    for i in np.flatnonzero(lbv > n - LN)[:200]:
        for coop in (False, True):
            p, out, info = X.py_window_search(kl, int(gv[i]), int(ev[i]), qv[i].item(), LN, coop)
            assert p == lbv[i] and out == fbv[i]
            moved += info["moved_left"]
    assert moved >= LN
    # gallop into the ends (C with error rows, N without): lower bound 0 and n from a guess at least 2^17 keys away
    top = np.finfo(dt).max if kt == "f64" else np.iinfo(dt).max
    for v in "CN":
        qv, gv, ev, lbv, dv, fbv = cen[v]
        left = fbv & (lbv == 0) & (gv >= 1 << 17)
        right = fbv & (lbv == n) & (gv <= n - (1 << 17))
        assert (left & (qv == keys[0])).any() and (left & (qv < keys[0])).any() and (left & (qv == 0)).any(), v
        assert (right & (qv > keys[-1])).any() and ((lbv == n) & (qv == top)).any(), v
        if kt != "f64":                                           # (f64: TINY x the largest double moves that query's guess to n - 1)
            assert (right & (qv == top)).any(), v
        assert (fbv & (lbv == n - 1) & (gv <= n - (1 << 17))).any()
    assert (cen["N"][2] == 0).all() and dr[f"main-N-{kt}"][0].errors is None
    # duplicates: the run's key, the key below, the key above; the guess at the run's first, middle and last position; e < run
    vals, first, counts = np.unique(keys, return_index=True, return_counts=True)
    for run in X.dup_runs(kt):
        runs = np.flatnonzero(counts == run) if run > 2 else np.flatnonzero(counts == 2)
        assert len(runs) == 3, run
        offs = set()
        for r in runs:
            s, kv = int(first[r]), vals[r]
            on, below, above = (q == kv), (lb == s) & (q < kv) & (q > keys[s - 1]), (lb == s + run) & (q > kv) & (q < keys[s + run])
            assert on.sum() >= run and below.any() and above.any(), run
            assert np.all(lb[on] == s) and len(set(g[on].tolist())) == 1 and int(e[on][0]) < run
            offs.add(int(g[on][0]) - s)
        assert offs == {0, run // 2, run - 1}, (run, offs)


@pytest.mark.parametrize("kt", ["u64", "u32"])
def test_census_of_the_high_keys(drivers, kt):
    """keys and queries on both sides of 2^63 (u32: 2^31), up to the type's maximum"""
    c, (g, e, undef) = drivers(kt)[f"high-{kt}"]
    assert not undef.any()
    q, g, e, lb, d, fb = _census(c, g, e, undef)
    top = np.iinfo(c.dtype).max
    half = c.dtype(top // 2 + 1)
    assert c.keys[0] == 0 and c.keys[-1] == top and (c.keys < half).sum() == c.n // 2
    for side in (q < half, q >= half):
        assert (side & fb & (d > 0)).sum() > 1000 and (side & fb & (d < 0)).sum() > 1000 and (side & ~fb).sum() > 1000
    assert (q == top).any() and (q == half).any() and (q == half - c.dtype(1)).any() and (q == 0).any()
    assert (fb & (lb == 0) & (g >= 1 << 17)).any() and (fb & (lb == c.n - 1) & (g <= c.n - (1 << 17))).any()
    assert {1 << 63, X.U64MAX} <= set(e.tolist())


def test_census_of_the_f64_keys_around_zero(drivers):
    c, (g, e, undef) = drivers("f64")["signed-f64"]
    k = c.keys
    assert (k < 0).sum() > 1000 and (k > 0).sum() > 1000
    z = np.flatnonzero(k == 0.0)
    assert len(z) == 2 and np.signbit(k[z[0]]) and not np.signbit(k[z[1]])           # -0.0 and 0.0 both resident, equal keys
    tiny = np.finfo(np.float64).tiny
    assert ((k > 0) & (k < tiny)).sum() >= 2 and ((k < 0) & (k > -tiny)).sum() >= 2   # denormals
    qq = c.queries
    assert np.isnan(qq).sum() == 1 and undef.sum() == 1 and np.isposinf(qq).any() and np.isneginf(qq).any()
    assert ((qq == 0.0) & np.signbit(qq)).any() and ((qq == 0.0) & ~np.signbit(qq)).any()
    q, g, e, lb, d, fb = _census(c, g, e, undef)
    assert (fb & (d > 0)).any() and (fb & (d < 0)).any() and (~fb).sum() > 1000
    assert lb[np.isposinf(q)].tolist() == [c.n] and lb[np.isneginf(q)].tolist() == [0]
    assert g[np.isposinf(q)].tolist() == [c.n - 1] and g[np.isneginf(q)].tolist() == [0]
    # the NaN query: leaf 0, guess 0, lower bound 0 (no key is < NaN): no fallback whatever the error
    i = np.flatnonzero(np.isnan(qq))
    assert c.qleaf[i].tolist() == [0] and X.design_guess(c)[i].tolist() == [0] and X.lower_bound(k, qq[i]).tolist() == [0]


@pytest.mark.parametrize("kt", KTS)
def test_census_of_the_short_key_sets_and_the_restatement(drivers, kt):
    """The short sets, and the Python restatement of the window search against the count of smaller keys on all of them: which form
    of the last line of keys runs is counted from a model of the kernel's own control flow."""
    LN = D.line_keys(X.DT[kt])
    dr = drivers(kt)
    assert X.short_ns(kt) == [1, 2, LN - 1, LN, LN + 1, 2 * LN - 1, 2 * LN, 2 * LN + 1]
    for n in X.short_ns(kt):
        c, (g, e, undef) = dr[f"short-{n}-{kt}"]
        assert not undef.any() and c.L == 256
        assert set(e.tolist()) == {0, 1, LN, n, X.U64MAX}
        forms = {"at_base": 0, "moved_left": 0, "short_form": 0}
        seen = set()
        for rot in (0, 7, 19):
            keys = X.short_keys(kt, n, rot)
            assert len(keys) == n and np.all(keys[1:] > keys[:-1])
            lb = X.lower_bound(keys, c.queries)
            assert np.array_equal(lb, np.searchsorted(keys, c.queries, side="left").astype(np.uint64))
            fb = X.expected_fallbacks(g, e, lb)
            kl = keys.tolist()
            for i in range(0, len(c.queries), 1 if rot == 0 else 5):
                for coop in (False, True):
                    p, out, info = X.py_window_search(kl, int(g[i]), int(e[i]), c.queries[i].item(), LN, coop)
                    assert p == lb[i] and out == fb[i], (n, rot, i, coop)
                    for f in forms:
                        forms[f] += info[f]
            # every key: a query below, on and above it with every guess kind and every error
            on = np.isin(c.queries, keys)
            for i in np.flatnonzero(on):
                seen.add((int(lb[i]), int(c.qleaf[i]) % X.SHORT_COMBOS))
            assert on.sum() == n
            if n >= 2:
                assert fb.any() and (~fb).any()
        if n < LN:
            assert forms["short_form"] > 0 and forms["moved_left"] == forms["at_base"] == 0
        else:
            assert forms["short_form"] == 0 and forms["moved_left"] > 0 and forms["at_base"] > 0
        # guesses 0, n / 2, n - 1 and the sweep against the lower bound
        assert {0, n // 2, n - 1} <= set(g.tolist())
        sweep = c.qleaf % 4 == 3
        assert set(g[sweep].tolist()) == set(range(n))
    # over the 20 rotations every key is a present query of every one of the 20 scenarios
    n = X.short_ns(kt)[-1]
    c = dr[f"short-{n}-{kt}"][0]
    seen = set()
    for rot in range(X.SHORT_COMBOS):
        keys = X.short_keys(kt, n, rot)
        on = np.flatnonzero(np.isin(c.queries, keys))
        seen |= {(int(p), int(t) % X.SHORT_COMBOS) for p, t in zip(np.searchsorted(keys, c.queries[on]), c.qleaf[on])}
    assert len(seen) == n * X.SHORT_COMBOS


@pytest.mark.parametrize("kt", KTS)
def test_census_of_the_lookup_sets(drivers, kt):
    dr = drivers(kt)
    names = [nm for nm in dr if not nm.startswith(("main-", "short-", "high-", "signed-"))]
    fam = {nm.split("-")[0] for nm in names}
    assert fam >= {"linear", "cubic", "loglinear", "normal", "radix", "bradix", "table"}
    assert {nm.split("-")[1] for nm in names if nm.startswith("bradix")} == {"high", "low"}
    L, n = X.LK_L, X.LK_N
    for nm in names:
        c, (g, e, undef) = dr[nm]
        if nm.startswith("precision"):
            continue
        m = re.match(r"bradix-(high|low)-c(\d+)", nm)                         # (a bradix root reaches the leaves its clamp leaves it)
        reach = L if not m else int(m.group(2)) + 1 if m.group(1) == "high" else min(L, 16 - int(m.group(2)))
        assert set(c.qleaf.tolist()) == set(range(reach)), nm                  # every leaf, so every class of leaf prediction
        assert (c.errors is None) == ("noerr" in nm)
        if nm.startswith(("cubic", "radix", "table", "bradix-low-c2")):
            assert undef.sum() > 0, nm
        if nm.startswith("bradix-high"):
            assert undef.sum() == 0
    for f in fam - {"precision"}:                                             # both leaf kinds and both error modes per family
        mine = [nm for nm in names if nm.startswith(f)]
        assert any("-linear-" in nm[len(f):] for nm in mine) and any("-cubic-" in nm[len(f):] for nm in mine)
        assert any(nm.endswith(f"-err-{kt}") for nm in mine) and any(nm.endswith(f"-noerr-{kt}") for nm in mine)
    # leaf predictions: negative, in (-1, 0), in (n - 2, n - 1), n - 1, above n - 1, above 2^64, -inf, +inf
    G = X.lookup_G()
    assert (G < -1).any() and ((G > -1) & (G < 0)).any() and ((G > n - 2) & (G < n - 1)).any() and (G == n - 1).any()
    assert ((G > n - 1) & (G < 2.0 ** 64)).any() and ((G > 2.0 ** 64) & np.isfinite(G)).any() and np.isneginf(G).any() and np.isposinf(G).any()
    # raw predictions of the float roots: -1, just above -1, -0.0, L - 1, just below L, L, far above, NaN
    for f in ("linear", "cubic"):
        c = dr[[nm for nm in names if nm.startswith(f + "-")][0]][0]
        raw = X.float_root_raw(c.root, X.as_float(c.queries))
        assert (raw == -1.0).any() and ((raw > -1.0) & (raw < -0.99)).any() and (raw == L - 1.0).any()
        assert ((raw < L) & (raw > L - 0.01)).any() and (raw == float(L)).any() and (raw > 1e6).any()
        if kt == "f64":
            assert ((raw == 0.0) & np.signbit(raw)).any() and np.isnan(raw).any() and np.isinf(raw).any() == (f == "linear")
        if f == "cubic":                                                      # (-1, 0) is defined: leaf 0; -1 is not
            assert not c.oob[(raw > -1.0) & (raw < 0.0)].any() and c.oob[raw == -1.0].all() and c.oob[raw >= L].all()
            assert c.oob.sum() == ((raw <= -1.0) | (raw >= L) | np.isnan(raw)).sum()
    if kt == "u64":
        c, (g, e, undef) = dr["precision-linear-u64"]
        for v in ((1 << 53) - 1, (1 << 53) + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1025, X.U64MAX):
            assert (c.queries == np.uint64(v)).any()
        # one ulp of (double) key is one unit of the guess
        i, j = np.flatnonzero(c.queries == np.uint64((1 << 63) + 1023))[0], np.flatnonzero(c.queries == np.uint64((1 << 63) + 1025))[0]
        assert g[j] == g[i] + 1 and g[i] == 1 << 52
        i, j = np.flatnonzero(c.queries == np.uint64(1 << 53))[0], np.flatnonzero(c.queries == np.uint64((1 << 53) + 3))[0]
        assert g[j] == g[i] + 2 and g[i] == 1 << 52
    if kt == "u32":
        for nm in names:
            if nm.startswith(("linear", "loglinear", "normal")):
                qq = dr[nm][0].queries
                assert (qq == 0).any() and (qq == 0xFFFFFFFF).any(), nm


@pytest.mark.parametrize("kt", KTS)
def test_verify_sets_have_their_designed_outside_count(kt):
    for outside, want in (("0", 0), ("1", 1), ("n", None)):
        c = X.verify_case(kt, outside)
        fb = X.expected_fallbacks(X.design_guess(c), X.design_err(c), X.lower_bound(c.keys, c.queries))
        assert int(fb.sum()) == (c.n if want is None else want)
        assert np.array_equal(c.qleaf, np.minimum(c.keys.astype(np.float64) * c.root.p[1], c.L - 1).astype(np.int64))


def test_batch_shapes():
    assert X.BATCH_SIZES == (1, 7, 8, 9, 63, 64, 65, 255, 256, 257)
    for cus in (64, 256, 304):
        nq = X.big_batch_size(cus)
        assert nq > 2 * cus * 8 * 256 and nq % 8 != 0
    c = X.tiled(X.main_case("u32", "A"), 1000)
    assert len(c.queries) == len(c.qleaf) == len(c.oob) == 1000
