"""The exact leaf kernels (k_leaf_regs, k_leaf_lanes, k_spline_scan) on key sets DESIGNED to sit on their size limits
(tests/designed.py): leaves of exactly T - 2 .. T + 2 keys for every limit T, at chosen lanes of a group, offsets inside a line and
inside a scan tile, beside runs of empty leaves, with duplicate pairs and runs at chosen steps.  The bar is the suite's: bucket
table, error integers, counts and coefficients bit-identical to the oracle, aggregates as in test_gpu_lanes._check, rows equal to
parameters + error.  On top of it every case reads the route and a counter back (rmi_hip_last_route_info, TrainedRMI.route) and
asserts that the input reached the branch it was built for.  A designed set always trains: an OracleError fails the test."""
import numpy as np
import pytest

from tests import designed as D
from tests import lookup_driver as ld

pytestmark = pytest.mark.gpu

KTS = ("u64", "u32", "f64")
KT_ROOTS = [(kt, r) for kt in KTS for r in ("linear", "radix", "cubic") if not (kt == "f64" and r == "radix")]   # (f64 keys have no radix root)
REGS_ENV = {"RMI_HIP_REGS": "1"}
# key type, environment and the k_leaf_regs variant of a set of short leaves (4-byte keys: at two waves per SIMD and at one)
KT_ENVS = [("u64", {}, 0), ("f64", {}, 0), ("u32", {"RMI_HIP_REGS_U32": "2"}, 2), ("u32", {"RMI_HIP_REGS_U32": "1"}, 0)]
LANES_ENV = {"RMI_HIP_REGS": "0"}


def _roots(oracle, d, rname, tr):
    from rmi_amd import train
    rp = d.roots()[rname]
    if rp is None:
        return tr.fit_root(rname, d.L), None
    return train.Model(rp[0], rp[1]), oracle.Model(rp[0], rp[1], (0, 0, 0, 0))


def _same(g, o, d, coef_exact=True):
    L = d.L
    assert np.array_equal(g.leaf_starts, d.starts), "bucket table is not the design's"
    assert np.array_equal(g.leaf_starts, o.leaf_start), "bucket assignment differs"
    bad = np.flatnonzero(g.last_layer_max_l1s != o.leaf_err)
    assert bad.size == 0, f"{bad.size} error integers differ, first at leaves {bad[:8].tolist()} of {d.counts[bad[:8]].tolist()} keys"
    assert np.array_equal(g.leaf_counts, o.leaf_count)
    if coef_exact:
        bad = np.flatnonzero((g.leaf_params.view(np.uint64) != o.leaf_params.view(np.uint64)).any(axis=1))
        assert bad.size == 0, f"{bad.size} coefficient rows differ, first at leaves {bad[:8].tolist()} of {d.counts[bad[:8]].tolist()} keys"
    assert g.model_max_error == o.model_max_error and g.model_max_error_idx == o.model_max_error_idx
    assert g.model_avg_error == o.model_avg_error
    assert abs(g.model_avg_l2_error - o.model_avg_l2_error) <= 1e-9 * max(1.0, abs(o.model_avg_l2_error))
    assert abs(g.model_avg_log2_error - o.model_avg_log2_error) <= 1e-9 * max(1.0, abs(o.model_avg_log2_error))
    rows = g.rows.view(np.uint64).reshape(L, 3)
    assert np.array_equal(rows[:, :2], g.leaf_params.view(np.uint64)) and np.array_equal(rows[:, 2], g.last_layer_max_l1s)


def _run(monkeypatch, oracle, env, d, rname="linear", leaf="linear", mode=0, coef_exact=True, trainings=1):
    """Trains `d` on a fresh context under `env`, `trainings` times; every result equal to the oracle's.  Returns the results."""
    from rmi_amd import train
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tr = train.Trainer(d.keys)
    tr.set_fit_mode(mode)
    g_root, o_root = _roots(oracle, d, rname, tr)
    o = oracle.train_two_layer(rname, leaf, d.keys, d.L, root=o_root)
    out = []
    for _ in range(trainings):
        g = tr.train_leaves(g_root, leaf, d.L)
        assert g.route is not None and g.route["pipeline"] == g.pipeline
        _same(g, o, d, coef_exact)
        out.append(g.materialize())
    tr.close()
    return out[0] if trainings == 1 else out


def _listed_band(d):
    must, may = D.expected_listed_groups(d)
    return len(must), len(may)


# ---- case 1: the size census --------------------------------------------------------------------------------------------------
# (key type, the LONG set, environment, the k_leaf_regs variant the route must name)
REGS_CASES = [("u64", False, {}, 0), ("f64", False, {}, 0), ("u64", True, {}, 1), ("f64", True, {}, 1),
              ("u32", False, {"RMI_HIP_REGS_U32": "2"}, 2), ("u32", True, {"RMI_HIP_REGS_U32": "2"}, 2),
              ("u32", False, {"RMI_HIP_REGS_U32": "1"}, 0), ("u32", True, {"RMI_HIP_REGS_U32": "1"}, 1)]


@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("kt,long_variant,env,variant", REGS_CASES)
def test_census_k_leaf_regs(monkeypatch, oracle, kt, long_variant, env, variant, second):
    """Under the linear root, and under the second exact root of the key type: radix (f64 keys, which have none: cubic by its margin)."""
    d = D.regs_set(kt, long_variant=long_variant)
    rname = "linear" if not second else ("cubic" if kt == "f64" else "radix")
    g = _run(monkeypatch, oracle, dict(REGS_ENV, **env), d, rname)
    r = g.route
    assert (r["pipeline"], r["regs"], r["search"]) == (4, variant, True)
    lo, hi = _listed_band(d)
    assert lo <= r["regs_listed"] <= hi and hi * 4 < d.L // 64, (r["regs_listed"], lo, hi)
    assert r["regs_dups"] == 0


# ---- case 2: sparse duplicates ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt,long_variant,env,variant", REGS_CASES)
def test_sparse_duplicates_k_leaf_regs(monkeypatch, oracle, kt, long_variant, env, variant):
    """Duplicate pairs and runs in eight leaves, one group each, outside the stretches the boundary search samples: the walk itself
    has to find them, list those groups and only those, and keep the rest on the register path."""
    d = D.regs_set(kt, long_variant=long_variant, dups=True)
    g = _run(monkeypatch, oracle, dict(REGS_ENV, **env), d)
    r = g.route
    assert r["regs_dups"] == 0, "the duplicates lie outside the sampled stretches"
    assert (r["pipeline"], r["regs"]) == (4, variant), "pipeline 4 is kept"
    lo, hi = _listed_band(d)
    assert lo >= len(D.dup_specs()) + 1 and lo <= r["regs_listed"] <= hi, (r["regs_listed"], lo, hi)


def test_distinct_keys_with_equal_low_words(monkeypatch, oracle):
    """Two distinct u64 keys 2^32 apart: the in-walk test (XOR of the low words) takes them for a duplicate -- the group is listed and
    its results are the oracle's."""
    clean, d = D.regs_set("u64"), D.regs_set("u64", wide=True)
    g0 = _run(monkeypatch, oracle, REGS_ENV, clean)
    g = _run(monkeypatch, oracle, REGS_ENV, d)
    (leaf, _), = d.wide.items()
    assert leaf // 64 not in D.expected_listed_groups(clean)[1]
    lo, hi = _listed_band(d)
    assert g.route["pipeline"] == 4 and lo <= g.route["regs_listed"] <= hi
    assert g.route["regs_listed"] == g0.route["regs_listed"] + 1


@pytest.mark.parametrize("kt,env,variant", KT_ENVS)
def test_give_up_rule(monkeypatch, oracle, kt, env, variant):
    """1 .. 64 duplicate pairs at leaf borders inside the sampled stretch: whatever the boundary search counted, the route is the one
    the rule gives for it (regs_dups * 1024 > L: every group listed at once, reported as 3), the rule goes both ways over the six
    sets, and every one equals the oracle."""
    went = set()
    for pairs in (1, 2, 4, 8, 16, 64):
        d = D.giveup_set(pairs, kt)
        r = _run(monkeypatch, oracle, dict(REGS_ENV, **env), d).route
        groups = d.L // 64
        assert r["regs"] == variant, r
        if r["regs_dups"] * 1024 > d.L:
            assert (r["pipeline"], r["regs_listed"]) == (3, groups), (pairs, r)
            went.add("all")
        else:
            lo, hi = _listed_band(d)
            assert r["pipeline"] == 4 and lo <= r["regs_listed"] <= hi, (pairs, r, lo, hi)
            went.add("some")
    assert went == {"all", "some"}


@pytest.mark.parametrize("search", ["1", "0"])
@pytest.mark.parametrize("dups", [False, True])
@pytest.mark.parametrize("kt", KTS)
def test_census_k_leaf_lanes(monkeypatch, oracle, kt, dups, search):
    """Panel rows, long_min, LN_LONG_MAX, SG_SEG and SG_ERR_LONG of the list tail; the same with the sparse duplicates and a run
    longer than LN_LONG_MAX."""
    d = D.lanes_set(kt, dups=dups)
    g = _run(monkeypatch, oracle, dict(LANES_ENV, RMI_HIP_LANES_SEARCH=search), d)
    r = g.route
    assert (r["pipeline"], r["regs"], r["search"]) == (3, -1, search == "1")
    # a container holds the leaf's keys and up to two borrowed points: longer than long_min for sure from long_min + 1 keys on, never below long_min - 2
    lm = D.C["long_min"]
    lo, hi = int((d.counts >= lm + 1).sum()), int((d.counts >= lm - 3).sum())
    hi += len(d.dups)                                        # (a leaf with a duplicate may be handed over as well; its neighbours hold one of the keys only)
    assert lo >= 20 and lo <= r["flag_count"] <= hi, (r["flag_count"], lo, hi)
    assert g.long_leaves == r["flag_count"] and r["giant_count"] == 0


@pytest.mark.parametrize("kt", KTS)
def test_k_leaf_lanes_host_threshold_lowered(monkeypatch, oracle, kt):
    d = D.lanes_set(kt, dups=True)
    hm = 6000
    g = _run(monkeypatch, oracle, dict(LANES_ENV, RMI_HIP_HOST_MIN=str(hm)), d)
    lo, hi = int((d.counts >= hm + 1).sum()), int((d.counts >= hm - 1).sum())
    assert g.route["giants"] and lo >= 20 and lo <= g.route["giant_count"] <= hi


@pytest.mark.parametrize("delta", [-2, -1, 0, 1, 2])
@pytest.mark.parametrize("kt", KTS)
def test_one_leaf_on_the_host_threshold(monkeypatch, oracle, kt, delta):
    """One real leaf of host_min +- 2 keys: fitted on a host core when its container holds more than host_min points -- for certain
    from host_min + 1 keys on, never up to host_min - 2; in between it depends on the points the container borrows (0 or 1 accepted)."""
    d = D.lanes_set(kt, giant=delta)
    g = _run(monkeypatch, oracle, LANES_ENV, d)
    r = g.route
    assert r["pipeline"] == 3 and r["giants"]
    assert (1 if delta >= 1 else 0) <= r["giant_count"] <= (1 if delta >= -1 else 0), (delta, r["giant_count"])


@pytest.mark.parametrize("kt,rname", KT_ROOTS)
def test_census_k_spline_scan(monkeypatch, oracle, kt, rname):
    """Leaves on the first / last key of a tile, on the last key of the look-ahead and one either side, tiles of 63 .. 66 leaf starts,
    sizes around EXTN, TILE and long_min; then the same layout with duplicate runs across a tile border and across the keys in front
    of it (the FixDups offsets are the oracle's: every coefficient and error integer depends on them).  scan_listed is above 0 on both
    (the leaves that end behind the look-ahead), and the same on both: see below."""
    listed = {}
    for dups in (False, True):
        d = D.scan_set(kt, dups=dups)
        r = _run(monkeypatch, oracle, {}, d, rname, leaf="linear_spline").route
        assert r["pipeline"] == 5 and r["scan_mono"] == (rname != "cubic"), r
        listed[dups] = r["scan_listed"]
        if rname != "cubic":
            assert r["scan_listed"] > 0, "tiles with a leaf open beyond the look-ahead go to the general form"
            assert r["scan_listed"] < d.n // D.tile_keys(d.keys.dtype), "most tiles take the short form"
    # RMI_SC_FAST_DUPS = 1: the short form keeps a tile with duplicate keys (its error pass then carries y and the run lengths), so the
    # runs send no further tile to the general form -- the tiles with a run across their border were worked by the short form
    assert D.C["RMI_SC_FAST_DUPS"] == 1 and listed[True] == listed[False], listed


@pytest.mark.parametrize("avg", [19, 20, 21, 39, 40, 41])
def test_scan_average_around_the_row_rule(monkeypatch, oracle, avg):
    """Exactly 19 / 20 / 21 (8-byte keys) and 39 / 40 / 41 (4-byte keys) keys a leaf on average, with one leaf that is open at a tile's
    end and runs on behind the look-ahead: from 1.25 rows of a lane a leaf on the short form runs and has to list that tile; below, the
    general form takes every tile and there is no list."""
    d = D.scan_set("u64" if avg < 30 else "u32", avg=avg)
    for rname in ("linear", "radix"):
        r = _run(monkeypatch, oracle, {}, d, rname, leaf="linear_spline").route
        assert r["pipeline"] == 5 and r["scan_mono"], r
        assert (r["scan_listed"] == 0) if avg in (19, 39) else (r["scan_listed"] > 0), (avg, r)


@pytest.mark.parametrize("kt", KTS)
def test_scan_one_leaf_on_the_far_limit(monkeypatch, oracle, kt):
    """Among leaves longer than a tile (the long-leaf instance of the short form, FAR = 2) one leaf whose end lies RMI_SC_FAR_MAX - 2 .. + 2
    keys behind the end of the tile it starts in: the search for an open leaf's end covers RMI_SC_FAR_MAX - 1 keys behind the tile, so the
    leaf's tile is kept up to there and listed from RMI_SC_FAR_MAX on; nothing else differs between the five sets.  Trained twice each (the
    second training sizes its launch by the first one's count)."""
    listed = {}
    for delta in (-2, -1, 0, 1, 2):
        d = D.scan_set(kt, far=delta)
        g1, g2 = _run(monkeypatch, oracle, {}, d, "linear", leaf="linear_spline", trainings=2)
        assert g1.route["pipeline"] == 5 and g1.route["scan_mono"] and g1.route["scan_listed"] == g2.route["scan_listed"]
        listed[delta] = g1.route["scan_listed"]
    assert listed[-2] == listed[-1] and listed[0] == listed[1] == listed[2] == listed[-1] + 1, listed


# ---- case 3: predictions that land on an integer ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kt,rname", KT_ROOTS)
def test_integer_valued_predictions(monkeypatch, oracle, kt, rname):
    """Every leaf's first key is exactly j << s (the root predicts exactly j), its last ((j + 1) << s) - 1."""
    d = D.regs_set(kt, edge_keys=True)
    assert d.edge_keys and int(d.keys[int(d.starts[5])]) == 5 << d.shift
    g = _run(monkeypatch, oracle, REGS_ENV, d, rname)
    r = g.route
    assert r["pipeline"] == 4 and r["search"]
    if rname == "cubic":
        assert r["cubic_margin"] and not r["verify"]
        monkeypatch.setenv("RMI_HIP_CUBIC_MARGIN", "0")
        r = _run(monkeypatch, oracle, REGS_ENV, d, rname).route
        assert r["verify"] and not r["cubic_margin"] and r["pipeline"] == 3
    _run(monkeypatch, oracle, LANES_ENV, d, rname)
    g = _run(monkeypatch, oracle, {}, d, rname, leaf="linear_spline")
    assert g.route["pipeline"] == 5


# ---- case 4: history on one context ------------------------------------------------------------------------------------------------
def _arrays(g):
    return [g.rows.tobytes(), g.leaf_params.tobytes(), g.last_layer_max_l1s.tobytes(), g.leaf_counts.tobytes(), g.leaf_starts.tobytes()]


@pytest.mark.parametrize("leaf", ["linear", "linear_spline"])
@pytest.mark.parametrize("kt,env,variant", KT_ENVS)
def test_history_on_one_context(monkeypatch, oracle, kt, env, variant, leaf):
    """Census, sparse duplicates, a key set that ARMS the context's memory, census again, another leaf count, all on one context: what
    the context remembers of a key set (regs_off, scan_hint, scan_skew of RouteMemory) must not leak into the next one.  The arming set
    is trained twice -- linear leaves: 64 duplicate pairs in the sampled stretch, every group listed, the second training does not
    launch k_leaf_regs any more (regs_off); linear_spline leaves: every tile listed, the second training takes the long-leaf instance
    (scan_skew) -- and the census behind it must run as on a fresh context.  Every training equals the oracle; the first training of
    every key set equals the same training on a fresh context, byte for byte in every array, and in its route."""
    from rmi_amd import train
    if leaf == "linear_spline" and env.get("RMI_HIP_REGS_U32") == "1":
        env = {}                                             # (k_spline_scan has one form for 4-byte keys: the case runs once more, plainly)
    for k, v in dict(REGS_ENV if leaf == "linear" else {}, **env).items():
        monkeypatch.setenv(k, v)
    if leaf == "linear":
        census, sparse, arming = D.regs_set(kt), D.regs_set(kt, dups=True), D.giveup_set(64, kt)
    else:
        census, sparse, arming = D.scan_set(kt), D.scan_set(kt, dups=True), D.scan_set(kt, skew=True)
    L = census.L
    assert arming.L == L
    steps = [(census, L, 1), (sparse, L, 1), (arming, L, 2), (census, L, 1), (census, L // 2, 1)]
    tr = train.Trainer(census.keys)
    last = None
    for step, (d, Ls, times) in enumerate(steps):
        if d is not last:
            tr.set_keys(d.keys)
            last = d
        w = 2.0 ** -(d.shift + (1 if Ls != L else 0))
        o = oracle.train_two_layer("linear", leaf, d.keys, Ls, root=oracle.Model(0, (0.0, w, 0.0, 0.0), (0, 0, 0, 0)))
        routes = []
        for t in range(times):
            g = tr.train_leaves(train.Model(0, (0.0, w, 0.0, 0.0)), leaf, Ls).materialize()
            routes.append(g.route)
            assert np.array_equal(g.last_layer_max_l1s, o.leaf_err) and np.array_equal(g.leaf_params.view(np.uint64), o.leaf_params.view(np.uint64)), (step, t)
            assert np.array_equal(g.leaf_counts, o.leaf_count) and np.array_equal(g.leaf_starts, o.leaf_start), (step, t)
            if t == 0:
                fresh_tr = train.Trainer(d.keys)
                f = fresh_tr.train_leaves(train.Model(0, (0.0, w, 0.0, 0.0)), leaf, Ls).materialize()
                fresh_tr.close()
                assert _arrays(g) == _arrays(f), step
                assert g.route == f.route, (step, g.route, f.route)
        if d is arming and leaf == "linear":                 # the memory is armed: the second training went to k_leaf_lanes
            assert routes[0]["regs_listed"] * 4 > L // 64 and (routes[1]["pipeline"], routes[1]["regs"]) == (3, -1), routes
        elif d is arming:
            assert routes[0]["scan_listed"] > 512 and not routes[0]["long_leaves"] and routes[1]["long_leaves"], routes
        elif leaf == "linear":
            assert (routes[0]["pipeline"], routes[0]["regs"]) == (4, variant), (step, routes)
        else:
            assert routes[0]["pipeline"] == 5 and not routes[0]["long_leaves"], (step, routes)
    tr.close()


# ---- case 5: the guarded one-pass mode -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dups", [False, True])
@pytest.mark.parametrize("kt", KTS)
def test_guarded_one_pass_mode(monkeypatch, oracle, kt, dups):
    """set_fit_mode(1) on the census of 300 keys a leaf (the one-pass kernel takes averages of 32 keys and more): error integers,
    counts and bucket table bit-identical; every leaf with a duplicate is re-fitted by the exact kernels."""
    d = D.regs_set(kt, long_variant=True, dups=dups)
    g = _run(monkeypatch, oracle, {}, d, mode=1, coef_exact=False)
    assert g.route["sigma"] and g.fit_mode_used == 1
    assert g.route["flag_count"] >= len(d.dups) and g.exact_leaves >= len(d.dups)


# ---- case 6: the device index on a designed model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf,env", [("linear", REGS_ENV), ("linear_spline", {})])
@pytest.mark.parametrize("kt", KTS)
def test_device_index_on_the_sparse_duplicate_sets(monkeypatch, kt, leaf, env):
    """The lower bound of a run of equal keys at a leaf's first and last position, of absent keys and of keys outside the range."""
    from rmi_amd import train
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = D.regs_set(kt, dups=True) if leaf == "linear" else D.scan_set(kt, dups=True)
    tr = train.Trainer(d.keys)
    rp = d.roots()["linear"]
    rmi = tr.train_leaves(train.Model(rp[0], rp[1]), leaf, d.L).materialize()
    ix = rmi.index()
    assert ix.verify() == (d.n, 0)
    for name, q in ld.query_sets(d.keys, seed=7).items():
        assert np.array_equal(ix.search(q), np.searchsorted(d.keys, q, side="left").astype(np.uint64)), name
    runs = np.concatenate([d.keys[int(d.starts[j]) + p:int(d.starts[j]) + p + r] for j, (p, r) in d.dups.items()])
    assert np.array_equal(ix.search(runs), np.searchsorted(d.keys, runs, side="left").astype(np.uint64))
    ix.close()
    tr.close()
