"""The designed key sets of tests/designed.py, without a GPU: every set the GPU module trains is bucketed by the oracle exactly as
it was designed (so a designed set must train: an OracleError is a failure), its census of leaf sizes and placements is what the
GPU tests rely on, and the size limits it was built around still have the values the kernels' sources give them."""
import os
import re

import numpy as np
import pytest

from tests import designed as D
from tests import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KTS = ("u64", "u32", "f64")

# every set tests/test_gpu_designed.py trains: id -> (factory, leaf kinds, roots it is trained under there -- None: all it has)
SETS = {}
ALL = None
for _kt in KTS:
    SETS[f"regs-{_kt}"] = (lambda kt=_kt: D.regs_set(kt), ("linear",), ALL)
    SETS[f"regs-dups-{_kt}"] = (lambda kt=_kt: D.regs_set(kt, dups=True), ("linear",), ALL)
    SETS[f"regs-long-{_kt}"] = (lambda kt=_kt: D.regs_set(kt, long_variant=True), ("linear",), ALL)
    SETS[f"regs-long-dups-{_kt}"] = (lambda kt=_kt: D.regs_set(kt, long_variant=True, dups=True), ("linear",), ALL)
    SETS[f"regs-edge-{_kt}"] = (lambda kt=_kt: D.regs_set(kt, edge_keys=True), ("linear", "linear_spline"), ALL)
    SETS[f"lanes-{_kt}"] = (lambda kt=_kt: D.lanes_set(kt), ("linear",), ALL)
    SETS[f"lanes-dups-{_kt}"] = (lambda kt=_kt: D.lanes_set(kt, dups=True), ("linear",), ALL)
    SETS[f"scan-{_kt}"] = (lambda kt=_kt: D.scan_set(kt), ("linear_spline",), ALL)
    SETS[f"scan-dups-{_kt}"] = (lambda kt=_kt: D.scan_set(kt, dups=True), ("linear_spline",), ALL)
    for _d in (-2, -1, 0, 1, 2):
        SETS[f"lanes-giant{_d:+d}-{_kt}"] = (lambda kt=_kt, d=_d: D.lanes_set(kt, giant=d), ("linear",), ("linear",))
        SETS[f"scan-far{_d:+d}-{_kt}"] = (lambda kt=_kt, d=_d: D.scan_set(kt, far=d), ("linear_spline",), ("linear",))
    SETS[f"scan-skew-{_kt}"] = (lambda kt=_kt: D.scan_set(kt, skew=True), ("linear_spline",), ("linear",))
    for _p in (1, 2, 4, 8, 16, 64):
        SETS[f"giveup-{_p}-{_kt}"] = (lambda p=_p, kt=_kt: D.giveup_set(p, kt), ("linear",), ("linear",))
for _a in (19, 20, 21, 39, 40, 41):
    SETS[f"scan-avg{_a}"] = (lambda a=_a: D.scan_set("u64" if a < 30 else "u32", avg=a), ("linear_spline",), ALL)
SETS["regs-wide-u64"] = (lambda: D.regs_set("u64", wide=True), ("linear",), ALL)


def test_limits_in_the_source_are_the_ones_the_sets_were_built_for():
    """Every limit by its name in the source: a kernel change that moves one fails here, and the sets move with it."""
    for name, (fname, rx, value) in D.SOURCE_CONSTANTS.items():
        src = open(os.path.join(ROOT, "rmi_amd", "csrc", fname)).read()
        m = re.findall(rx, src)
        assert len(m) == 1, f"{name}: {len(m)} matches of /{rx}/ in {fname}"
        assert int(m[0]) == value, f"{name} is {m[0]} in {fname}; the designed sets were built for {value}"
    assert D.RG_MAXPTS == 240 and D.tile_keys(np.uint64) == 1024 and D.tile_keys(np.uint32) == 2048


@pytest.mark.parametrize("name", sorted(SETS))
def test_oracle_buckets_a_designed_set_as_designed(oracle, name):
    factory, leaves, roots = SETS[name]
    d = factory()
    assert np.all(d.keys[1:] >= d.keys[:-1])
    for rname, rp in d.roots().items():
        if roots is not None and rname not in roots:
            continue
        for leaf in leaves:
            root = None if rp is None else oracle.Model(rp[0], rp[1], (0, 0, 0, 0))
            o = oracle.train_two_layer(rname, leaf, d.keys, d.L, root=root)          # (an OracleError fails the test)
            assert np.array_equal(o.leaf_start, d.starts), (rname, leaf)
            assert np.array_equal(o.leaf_count, d.expected_counts), (rname, leaf)
            assert oracle.check_lookup_property(o, d.keys)[0] == 0, (rname, leaf)
            if rp is None:                                   # the fitted radix root is key >> shift
                bits = d.L.bit_length() - 1
                assert tuple(o.root.ip[:2]) == (64 - d.shift - bits, bits)


def test_python_restatement_agrees_on_the_smallest_gpu_set(oracle):
    """The smallest set the GPU module trains (19 keys a leaf on average, one leaf behind the look-ahead) under the fitted radix root:
    the oracle and the independent Python restatement agree on every output."""
    d = D.scan_set("u64", avg=19)
    assert d.n == 19 * 4096                                  # (77 824 keys: every other set of the GPU module holds more)
    ref = pyref.train_two_layer([int(k) for k in d.keys], "radix", "linear_spline", d.L)
    o = oracle.train_two_layer("radix", "linear_spline", d.keys, d.L)
    assert np.array_equal(o.leaf_start, d.starts)
    assert [[float(v) for v in row] for row in o.leaf_params] == [m.params() for m in ref["leaves"]]
    assert [int(v) for v in o.leaf_err] == ref["errs"] and [int(v) for v in o.leaf_count] == ref["counts"]


def test_python_restatement_agrees_on_a_small_set_with_duplicates(oracle):
    """A small set of the same make (threshold sizes of the first rows, empty leaves, a duplicate pair and a run) under the
    fitted radix root: the oracle and the independent Python restatement agree on every output."""
    lay = D.Layout(64, 5)
    for leaf, size in ((0, 16), (1, 17), (7, 15), (31, 33), (32, 31), (33, 32), (40, 18), (50, 14), (63, 16)):
        lay.place(leaf, size)
    lay.empty_run(10, 6)
    d = D.build(lay.counts, 30, np.uint64, dups={7: (13, 2), 40: (0, 18), 31: (3, 9)})
    for leaf in ("linear", "linear_spline"):
        ref = pyref.train_two_layer([int(k) for k in d.keys], "radix", leaf, d.L)
        o = oracle.train_two_layer("radix", leaf, d.keys, d.L)
        assert np.array_equal(o.leaf_start, d.starts)
        assert [[float(v) for v in row] for row in o.leaf_params] == [m.params() for m in ref["leaves"]]
        assert [int(v) for v in o.leaf_err] == ref["errs"] and [int(v) for v in o.leaf_count] == ref["counts"]


def _assert_census(d, thresholds):
    cen = D.census_of(d)
    for t in thresholds:
        for sz in range(t - 2, t + 3):
            assert sz in cen, f"no leaf of {sz} keys (limit {t})"
            assert len(cen[sz]) >= 2, f"leaves of {sz} keys (limit {t}) start at one offset inside a line only: {cen[sz]}"


def _assert_placements(d, sizes):
    L, c = d.L, d.counts
    sizes = set(sizes)
    for leaf in (0, L - 1, L // 2 - 1, L // 2, L // 2 + 1):
        assert int(c[leaf]) in sizes, (leaf, int(c[leaf]))
    lanes = np.arange(L) % 64
    special = np.isin(c, sorted(sizes))
    assert np.any(special & (lanes == 0) & (np.arange(L) > 0)) and np.any(special & (lanes == 63) & (np.arange(L) < L - 1))
    # a leaf of a census size with a run of empty leaves on either side, a run in front of the last leaf, a run in the second half
    around = [j for j in np.flatnonzero(special).tolist() if 5 <= j < L - 6 and not c[j - 5:j].any() and not c[j + 1:j + 6].any()]
    assert around, "no census leaf between two runs of empty leaves"
    assert not c[L - 6:L - 1].any() and int((c == 0).sum()) >= 30


@pytest.mark.parametrize("kt", KTS)
@pytest.mark.parametrize("long_variant", [False, True])
def test_census_of_the_register_kernel_sets(kt, long_variant):
    d = D.regs_set(kt, long_variant=long_variant, dups=True)
    _assert_census(d, D.T_REGS)
    assert {16 * m for m in range(1, 10)} | {64, 160, 192, 240, 1008, 1024} == set(D.T_REGS)
    _assert_placements(d, D.band(D.T_REGS))
    avg = d.n / d.L
    assert (D.C["regs_max_avg"] < avg <= D.C["regs_long_max_avg"]) if long_variant else (avg <= D.C["regs_max_avg"])
    if long_variant:                                         # groups whose every container is longer than the stash
        assert any(d.counts[g * 64:(g + 1) * 64].min() > D.C["RG_STASH"] for g in range(d.L // 64))
    # the duplicates: every placement once, in a group of its own, away from lanes 0 and 63 and from the stretches k_leaf_search samples
    assert len(d.dups) == len(D.dup_specs()) and len({j // 64 for j in d.dups}) == len(d.dups)
    for j, (pos, run) in d.dups.items():
        assert 1 <= j % 64 <= 62 and not D.in_sampled_stretch(j) and not D.in_sampled_stretch(j + 1)
        assert (int(d.counts[j]), pos, run) in [(s, p, r) for s, p, r, _ in D.dup_specs()]
        a = int(d.starts[j]) + pos
        assert np.all(d.keys[a:a + run] == d.keys[a]) and (pos == 0 or d.keys[a - 1] != d.keys[a])
    must, may = D.expected_listed_groups(d)
    assert len(may) * 4 < d.L // 64, "the census runs on the register path: most groups stay"
    if kt == "u64":                                          # in-walk duplicate test: XOR of the low words of neighbouring keys
        k = d.keys
        assert not np.any((k[1:] != k[:-1]) & (((k[1:] ^ k[:-1]) & np.uint64(0xFFFFFFFF)) == 0))
        w = D.regs_set("u64", wide=True)
        (leaf, pos), = w.wide.items()
        a = int(w.starts[leaf]) + pos
        assert int(w.keys[a + 1]) - int(w.keys[a]) == 1 << 32 and not w.dups


@pytest.mark.parametrize("kt", KTS)
def test_census_of_the_lane_kernel_sets(kt):
    d = D.lanes_set(kt, dups=True)
    _assert_census(d, D.T_LANES)
    _assert_placements(d, D.band(D.T_LANES))
    for delta in (-2, 2):
        g = D.lanes_set(kt, giant=delta)
        assert int(g.counts.max()) == D.C["host_min"] + delta and g.n < 300_000


@pytest.mark.parametrize("kt", KTS)
def test_census_of_the_scan_sets(kt):
    d = D.scan_set(kt, dups=True)
    _assert_census(d, D.T_SCAN)
    assert np.array_equal(d.counts, D.scan_set(kt).counts), "the same layout with and without the runs"
    L = d.L                                                  # sizes on the look-ahead and the row at leaf 0, L - 1 and around the split
    assert [int(d.counts[j]) for j in (0, L - 1, L // 2 - 1, L // 2, L // 2 + 1)] == [17, 33, 65, 129, 63]
    sk = D.scan_set(kt, skew=True)                           # every row of nine holds two leaf starts, in more than 512 tiles
    row = D.tile_keys(sk.keys.dtype) // 64
    st = sk.starts[:-1].astype(np.int64)
    assert sk.L == L and sk.n // (64 * row) > 512 and np.all(np.bincount(st // (9 * row)) == 2) and np.all((st[1::2] // row) == (st[0::2] // row))
    tk, dt = D.tile_keys(d.keys.dtype), d.keys.dtype
    extn, fhn = D.C["SC_EXTC"] * (16 // dt.itemsize), D.C["SC_FHC"] * (16 // dt.itemsize)
    assert (tk, extn, fhn) == ((2048, 128, 16) if kt == "u32" else (1024, 64, 8))
    st, en = d.starts[:-1].astype(np.int64), d.starts[1:].astype(np.int64)
    live = d.counts > 0
    assert np.any(live & (st % tk == 0) & (st > 0)) and np.any(live & (st % tk == tk - 1))
    # a leaf that starts inside a tile and ends on the last key of that tile's look-ahead, and one key either side
    tile_end = (st // tk + 1) * tk
    for off in (-1, 0, 1):
        assert np.any(live & (en == tile_end + extn + off)), off
    # tiles with 63 .. 66 leaf starts
    per_tile = np.bincount((st[live] // tk), minlength=d.n // tk + 1)
    assert {63, 64, 65, 66} <= set(per_tile.tolist()) and {64, 65} <= set(D.band([D.C["SC_SLOTS"]], 1))
    # duplicate runs: across a tile border, and across the FHN keys in front of one
    k = d.keys
    borders = np.arange(tk, d.n, tk)
    assert np.any(k[borders] == k[borders - 1])
    assert np.any((k[borders - fhn] == k[borders - fhn - 1]) & (k[borders - 1] == k[borders - fhn]))
    for a in (19, 20, 21) if kt != "u32" else (39, 40, 41):
        av = D.scan_set(kt, avg=a)
        j = int(np.argmax(av.counts))
        s0, e0 = int(av.starts[j]), int(av.starts[j + 1])
        assert av.n == a * av.L and s0 % tk == tk - 10 and e0 > (s0 // tk + 1) * tk + extn
    # the plain instance of the short form: at least 1.25 rows of a lane a leaf on average (else the general form over all tiles), at most EXTN
    assert 5 * (tk // 64) * d.L <= 4 * d.n and d.n <= extn * d.L
    for far in (-2, 2):                                      # the long-leaf instance: above 384 keys a leaf
        f = D.scan_set(kt, far=far)
        j = int(np.argmax(f.counts))
        s0, e0 = int(f.starts[j]), int(f.starts[j + 1])
        assert e0 - (s0 // tk + 1) * tk == D.C["RMI_SC_FAR_MAX"] + far and f.n > 384 * f.L and np.median(f.counts) > tk + extn
        assert f.n == D.scan_set(kt, far=0).n


@pytest.mark.parametrize("kt", KTS)
def test_give_up_sets(kt):
    for pairs in (1, 2, 4, 8, 16, 64):
        d = D.giveup_set(pairs, kt)
        assert len(d.dups) == pairs and all(j < D.C["LS_BLOCK"] - 1 and 1 <= j % 64 <= 62 and d.counts[j] == 2 for j in d.dups)
    # the rule of k_leaf_regs: regs_dups * 1024 > L -- the sets reach both sides of it if every pair is seen once
    assert 16 * 1024 <= 16384 < 64 * 1024


def test_builder_rejects_what_it_cannot_keep_exact():
    with pytest.raises(AssertionError):
        D.build(np.full(16384, 4), 40)                       # keys beyond 2^53 are not exact doubles
    with pytest.raises(AssertionError):
        D.build(np.full(8192, 4), 20, np.uint32)             # beyond 2^32
    with pytest.raises(AssertionError):
        D.build([4, 4], 8, dups={0: (3, 2)})                 # a run that leaves its leaf
    d = D.build([3, 0, 2, 1], 8, edge_keys=True)
    assert d.keys.tolist() == [0, 127, 255, 512, 767, 768]
