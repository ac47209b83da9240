"""Designed key sets: per-leaf key counts chosen by the test, not by a random generator.

Given counts c[0..L) and a shift s, leaf j gets c[j] keys inside [j << s, (j + 1) << s).  Under a root that is exact arithmetic
on such keys -- the caller-provided `linear` root (0, 2^-s), the `cubic` root (0, 0, 2^-s, 0), the fitted `radix` root when L is
a power of two -- the bucketing is known by construction: leaf_start is the cumulative sum of the counts, whatever the oracle
or a kernel says.  The tests put leaves of chosen sizes (the size limits of the leaf kernels, two either side) at chosen leaves,
lanes of a group of 64 leaves, offsets inside a 128-byte line and inside a scan tile, with duplicate runs at chosen steps.

numpy only; no GPU, no oracle."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

# The size limits the designed sets were built for, by the name the source gives them: (file under rmi_amd/csrc, regular
# expression with one group, value).  tests/test_designed_cpu.py reads every one back from the source.
SOURCE_CONSTANTS = {
    "RG_ROW": ("rmi_regs.hip.h", r"constexpr int RG_ROW = (\d+);", 16),
    "RG_UBLK": ("rmi_regs.hip.h", r"#define RG_UBLK (\d+)", 9),
    "RG_PRE": ("rmi_regs.hip.h", r"#define RG_PRE (\d+)", 3),
    "RG_STASH": ("rmi_regs.hip.h", r"#define RG_STASH_N (\d+)", 192),
    "RG_STASH2": ("rmi_regs.hip.h", r"#define RG_STASH2_N (\d+)", 160),
    "RG_BEHIND_STASH": ("rmi_regs.hip.h", r"constexpr int RG_MAXPTS = RG_STASH_N \+ (\d+);", 48),   # (RG_MAXPTS = 192 + 48 = 240)
    "RG_FARPTS": ("rmi_regs.hip.h", r"constexpr int RG_FARPTS = (\d+);", 1008),
    "RG_TMAX": ("rmi_regs.hip.h", r"constexpr int RG_TMAX = (\d+);", 1024),
    "LN_LONG_MAX": ("rmi_lanes.hip.h", r"constexpr int LN_LONG_MAX = (\d+);", 8192),
    "LS_BLOCK": ("rmi_lanes.hip.h", r"#define RMI_LS_BLOCK (\d+)", 512),
    "SG_SEG": ("rmi_sigma.hip.h", r"constexpr int SG_SEG = (\d+);", 2048),
    "SG_ERR_LONG": ("rmi_sigma.hip.h", r"constexpr int SG_ERR_LONG = (\d+);", 16384),
    "SC_TILE_ROWS": ("rmi_scan.hip.h", r"static constexpr int TILE = (\d+) \* V;", 64),        # (V = 16 / 32 keys a lane: 1 024 / 2 048)
    "SC_EXTC": ("rmi_scan.hip.h", r"static constexpr int EXTC = (\d+);", 32),                  # (x 2 / 4 keys a chunk: 64 / 128)
    "SC_FHC": ("rmi_scan.hip.h", r"static constexpr int FHC = (\d+);", 4),                     # (8 / 16 keys)
    "SC_SLOTS": ("rmi_scan.hip.h", r"constexpr int SC_SLOTS = (\d+);", 64),
    "RMI_SC_FAST_DUPS": ("rmi_scan.hip.h", r"#define RMI_SC_FAST_DUPS (\d+)", 1),             # (the short form keeps tiles with duplicate keys)
    "RMI_SC_FAR_MAX": ("rmi_scan.hip.h", r"#define RMI_SC_FAR_MAX (\d+)", 262144),
    "long_min": ("rmi_route.h", r"unsigned int long_min = (\d+);", 4096),
    "host_min": ("rmi_route.h", r"uint64_t host_min = (\d+);", 262144),
    "regs_max_avg": ("rmi_route.h", r"unsigned int regs_max_avg = (\d+);", 208),
    "regs_long_max_avg": ("rmi_route.h", r"unsigned int regs_long_max_avg = (\d+);", 640),
}
C = {k: v[2] for k, v in SOURCE_CONSTANTS.items()}
RG_MAXPTS = C["RG_STASH"] + C["RG_BEHIND_STASH"]          # 240
LINE_BYTES = 128

# thresholds (in keys of a leaf) by kernel: the census of a set holds T - 2 .. T + 2 for each
T_REGS = sorted({C["RG_ROW"] * m for m in range(1, C["RG_UBLK"] + 1)} | {(C["RG_PRE"] + 1) * C["RG_ROW"], C["RG_STASH2"], C["RG_STASH"],
                                                                        RG_MAXPTS, C["RG_FARPTS"], C["RG_TMAX"]})
T_LANES = sorted({16, 32, C["SG_SEG"], C["long_min"], C["LN_LONG_MAX"], C["SG_ERR_LONG"]})
T_SCAN = sorted({C["SC_EXTC"] * 2, C["SC_EXTC"] * 4, C["SC_TILE_ROWS"] * 16, C["SC_TILE_ROWS"] * 32, C["long_min"]})


def band(thresholds, width=2):
    """T - width .. T + width for every T: a leaf's container holds up to two borrowed points beside the leaf's own keys, so the
    band covers the container sitting on T whichever way it is counted."""
    return sorted({t + d for t in thresholds for d in range(-width, width + 1) if t + d >= 1})


def line_keys(dtype) -> int:
    return LINE_BYTES // np.dtype(dtype).itemsize


def tile_keys(dtype) -> int:
    return C["SC_TILE_ROWS"] * (128 // np.dtype(dtype).itemsize)


@dataclass
class Designed:
    keys: np.ndarray
    counts: np.ndarray                 # int64 [L]
    shift: int
    dups: dict = field(default_factory=dict)
    wide: dict = field(default_factory=dict)
    edge_keys: bool = False

    @property
    def L(self) -> int:
        return len(self.counts)

    @property
    def n(self) -> int:
        return len(self.keys)

    @property
    def starts(self) -> np.ndarray:
        """leaf_start by construction: [L + 1] uint64."""
        return np.concatenate([[0], np.cumsum(self.counts)]).astype(np.uint64)

    @property
    def expected_counts(self) -> np.ndarray:
        """leaf_count of the reference: the design, and one more for the leaf of the last key (two_layer.rs:226-232)."""
        c = self.counts.astype(np.uint64).copy()
        c[np.flatnonzero(self.counts)[-1]] += 1
        return c

    def roots(self):
        """The roots under which the bucketing is the design's, as (name, p, ip): `linear` and `cubic` caller-provided; `radix`
        is fitted by the trainer (None) and only offered where its fit reproduces key >> shift."""
        w = 2.0 ** -self.shift
        out = {"linear": (0, (0.0, w, 0.0, 0.0)), "cubic": (2, (0.0, 0.0, w, 0.0))}
        L = self.L
        nz = np.flatnonzero(self.counts)
        if L & (L - 1) == 0 and nz[-1] >= L // 2 and nz[0] < L // 2 and self.keys.dtype != np.float64:
            out["radix"] = None
        return out


def build(counts, shift: int, dtype=np.uint64, dups=None, wide=None, edge_keys=False) -> Designed:
    """counts[j] keys in [j << shift, (j + 1) << shift), evenly spread (edge_keys: the first exactly j << shift, the last exactly
    ((j + 1) << shift) - 1).  dups = {leaf: (position, run)}: keys position .. position + run - 1 of the leaf equal the key at
    `position`.  wide = {leaf: position} (u64, shift > 33): key position + 1 is key position + 2^32, two distinct keys with the same
    low word.  Neighbouring distinct integer keys otherwise differ in their low 32-bit words."""
    counts = np.asarray(counts, dtype=np.int64)
    L, s = len(counts), int(shift)
    dt = np.dtype(dtype)
    assert counts.min() >= 0 and counts.sum() > 0 and counts.max() <= (1 << s), "a leaf holds at most 2^shift distinct keys"
    assert (L << s) <= (1 << 53), "keys stay exact as doubles: 2^-shift * key is the leaf, with no rounding"
    if dt == np.uint32:
        assert (L << s) <= (1 << 32)
    assert (int(counts.max()) * 2 + 1) << s < (1 << 63)
    starts = np.concatenate([[0], np.cumsum(counts)])
    n = int(starts[-1])
    j = np.repeat(np.arange(L, dtype=np.uint64), counts)
    i = np.arange(n, dtype=np.uint64) - starts[:-1].astype(np.uint64)[j.astype(np.int64)]
    c = counts.astype(np.uint64)[j.astype(np.int64)]
    one = np.uint64(1)
    if edge_keys:
        span = np.uint64((1 << s) - 1)
        off = np.where(c > one, (i * span) // np.maximum(c - one, one), np.uint64(0))
    else:
        off = ((np.uint64(2) * i + one) << np.uint64(s)) // (np.uint64(2) * c)
    keys = (j << np.uint64(s)) + off
    # distinct neighbours with equal low words (possible across a leaf border when shift >= 32): move the upper key by one
    if dt == np.uint64 and s >= 32 and not edge_keys:
        keys += i % np.uint64(1024)                          # (evenly spread keys of a leaf of 2^k keys are multiples of 2^32 apart)
        bad = np.flatnonzero(((keys[1:] ^ keys[:-1]) & np.uint64(0xFFFFFFFF)) == 0) + 1
        keys[bad] += one
    for leaf, (pos, run) in (dups or {}).items():
        a = int(starts[leaf]) + pos
        assert 0 <= pos and run >= 2 and pos + run <= counts[leaf], (leaf, pos, run, counts[leaf])
        keys[a:a + run] = keys[a]
    for leaf, pos in (wide or {}).items():
        a = int(starts[leaf]) + pos
        assert dt == np.uint64 and pos + 2 < counts[leaf] and keys[a] + np.uint64(1 << 32) < keys[a + 2]
        keys[a + 1] = keys[a] + np.uint64(1 << 32)
    assert np.all(keys[1:] >= keys[:-1])
    if dt == np.uint64:
        same_low = np.count_nonzero((keys[1:] != keys[:-1]) & (((keys[1:] ^ keys[:-1]) & np.uint64(0xFFFFFFFF)) == 0))
        assert same_low == len(wide or {}), "distinct neighbours with equal low words: only where `wide` asks for them"
    assert np.array_equal((keys >> np.uint64(s)).astype(np.int64), j.astype(np.int64)), "every key lies in its leaf's interval"
    out = keys.astype(dt)                                    # (f64: exact below 2^53)
    return Designed(np.ascontiguousarray(out), counts, s, dict(dups or {}), dict(wide or {}), edge_keys)


class Layout:
    """Per-leaf counts under construction: a filler size everywhere, then chosen sizes at chosen leaves.  Leaves that were placed
    are fixed; `align` moves a leaf's start index to a residue by resizing filler leaves in front of it."""

    def __init__(self, L: int, filler):
        self.L = L
        f = np.asarray(filler, dtype=np.int64)
        self.counts = np.resize(f, L).astype(np.int64) if f.ndim else np.full(L, int(f), dtype=np.int64)
        self.fixed = np.zeros(L, dtype=bool)
        self.placed = []                                     # (leaf, size, tag)
        self._aligned_upto = 0

    def place(self, leaf: int, size: int, tag: str = ""):
        assert 0 <= leaf < self.L and not self.fixed[leaf], (leaf, size, tag)
        self.counts[leaf] = size
        self.fixed[leaf] = True
        self.placed.append((leaf, size, tag))
        return leaf

    def empty_run(self, first: int, length: int, tag: str = "empty"):
        for q in range(first, first + length):
            self.place(q, 0, tag)

    def free_leaf(self, at: int, lanes=range(1, 63)) -> int:
        """The first leaf >= at that is not fixed, whose neighbours are not fixed either, at one of `lanes` of its group."""
        q = at
        while self.fixed[q] or self.fixed[q - 1] or self.fixed[q + 1] or (q % 64) not in lanes:
            q += 1
        return q

    def start(self, leaf: int) -> int:
        return int(self.counts[:leaf].sum())

    def align(self, leaf: int, modulus: int, residue: int, per_leaf: int = 8):
        """start(leaf) % modulus == residue, by adding up to `per_leaf` keys to each of the filler leaves in front of `leaf` (behind
        the leaf aligned last: alignments are made in increasing leaf order)."""
        assert leaf >= self._aligned_upto
        need = (residue - self.start(leaf)) % modulus
        q = leaf - 1
        while need > 0:
            assert q >= self._aligned_upto, "not enough filler leaves in front"
            if not self.fixed[q]:
                d = min(per_leaf, need)
                self.counts[q] += d
                self.fixed[q] = True
                need -= d
            q -= 1
        self._aligned_upto = leaf
        assert self.start(leaf) % modulus == residue


def census_layout(L: int, sizes, filler, dtype, repeats: int = 2, first: int = 600, stride: int = 5, edge_sizes=None, empties: int = 50):
    """Every size of `sizes` `repeats` times at leaves first, first + stride, ... (lanes 1 .. 62), each repeat at another start offset
    inside a line; `edge_sizes` (six of them) at leaf 0, L - 1, L/2 - 1, L/2, L/2 + 1 and at lanes 0 and 63 of one group; runs of
    empty leaves in front of and behind one placed leaf, at the head of the second half and in front of the last leaf."""
    lay = Layout(L, filler)
    es = list(edge_sizes or sizes[:7])
    lay.place(0, es[0], "leaf0")
    lay.place(L - 1, es[1], "last")
    lay.place(L // 2 - 1, es[2], "split-1")
    lay.place(L // 2, es[3], "split")
    lay.place(L // 2 + 1, es[4], "split+1")
    g = (first // 64 + 1) * 64
    lay.place(g, es[5], "lane0")
    lay.place(g + 63, es[6 % len(es)], "lane63")
    lk = line_keys(dtype)
    q = g + 64
    todo = []
    for r in range(repeats):
        for k, sz in enumerate(sizes):
            q = lay.free_leaf(q)
            lay.place(q, sz, f"census{r}")
            todo.append((q, (3 + 5 * k + 7 * r) % lk))
            q += stride
    # runs of empty leaves: around one census leaf, and two long ones
    q = lay.free_leaf(q + 8)
    lay.empty_run(q - 5, 5)
    lay.place(q, es[5], "between-empties")
    lay.empty_run(q + 1, 7)
    rest = max(0, empties - 12)
    lay.empty_run(L // 2 + 70, rest // 2)
    lay.empty_run(L - 1 - (rest - rest // 2), rest - rest // 2)
    for leaf, res in sorted(todo):
        lay.align(leaf, lk, res, per_leaf=lk)
    return lay


def census_of(d: Designed, dtype=None):
    """{size: set of start offsets inside a line} over the leaves of a designed set."""
    lk = line_keys(d.keys.dtype if dtype is None else dtype)
    st = d.starts[:-1].astype(np.int64)
    out = {}
    for sz, a in zip(d.counts.tolist(), (st % lk).tolist()):
        out.setdefault(sz, set()).add(a)
    return out


def expected_listed_groups(d: Designed, long_min: int = C["long_min"]):
    """(must, may): groups of 64 leaves k_leaf_regs has to leave to k_leaf_lanes_listed, and those it may leave beside them.
    must: a leaf of at least RG_FARPTS + 3 keys (its container of >= RG_FARPTS + 1 points fails the test of make_tile whichever
    points it borrows), or a duplicate inside a leaf (both keys in the leaf's container).  may: a leaf within 2 of RG_FARPTS, and the
    group of leaf L/2 (the container behind the split does not cover the leaf's first key)."""
    far = C["RG_FARPTS"]
    must = {j // 64 for j in np.flatnonzero(d.counts >= far + 3).tolist()} | {j // 64 for j in d.dups} | {j // 64 for j in d.wide}
    may = {j // 64 for j in np.flatnonzero((d.counts >= far - 2) & (d.counts < far + 3)).tolist()} | {d.L // 2 // 64}
    return must, (may | must)


# ---------------------------------------------------------------------------------------------------------------------------
# The named sets of tests/test_gpu_designed.py (tests/test_designed_cpu.py checks every one against the oracle and the census)
# ---------------------------------------------------------------------------------------------------------------------------
# k_leaf_search samples regs_dups in every 16th stretch of LS_BLOCK leaves: leaves [0, 512), [8 192, 8 704), ...
def in_sampled_stretch(leaf: int) -> bool:
    return (leaf // C["LS_BLOCK"]) % 16 == 0


# duplicate placements of the sparse sets: (leaf size, position, run, what)
def dup_specs():
    return [(300, 0, 2, "steps 0/1"), (300, 15, 2, "steps 15/16"), (300, 159, 2, "steps 159/160"), (300, 191, 2, "steps 191/192"),
            (300, 239, 2, "steps 239/240"), (300, 298, 2, "the last two keys"), (40, 0, 40, "a whole leaf of one value"),
            (1000, 350, 300, "300 equal keys in a leaf of 1 000")]


_SHIFT = {("u64", 16384): 38, ("f64", 16384): 36, ("u32", 16384): 18, ("u64", 4096): 40, ("f64", 4096): 40, ("u32", 4096): 20,
          ("u64", 8192): 40, ("f64", 8192): 40, ("u32", 8192): 19, ("u64", 2048): 40, ("f64", 2048): 40, ("u32", 2048): 21, ("u64", 1024): 40, ("f64", 1024): 40, ("u32", 1024): 22}
DTYPES = {"u64": np.uint64, "u32": np.uint32, "f64": np.float64}
_EDGE_REGS = [RG_MAXPTS, RG_MAXPTS + 1, RG_MAXPTS, RG_MAXPTS + 1, RG_MAXPTS - 1, C["RG_FARPTS"], C["RG_FARPTS"] + 1]


def regs_set(kt: str, long_variant: bool = False, dups: bool = False, wide: bool = False, edge_keys: bool = False) -> Designed:
    """The census of k_leaf_regs: every size within 2 of a limit of T_REGS twice.  Short variants: L = 16 384 with 24 keys a leaf
    beside; LONG: L = 4 096 with 300 keys a leaf beside (every container of an ordinary group is longer than the stash).  dups: the
    placements of dup_specs in leaves of their own, one group each, outside the stretches k_leaf_search samples; wide: two
    neighbouring keys 2^32 apart in a clean group."""
    L, filler = (4096, 300) if long_variant else (16384, 24)
    dt = DTYPES[kt]
    lay = census_layout(L, band(T_REGS), filler, dt, repeats=2, first=600, stride=5, edge_sizes=_EDGE_REGS)
    dd, ww = {}, {}
    q = (max(p[0] for p in lay.placed if p[2].startswith("census")) // 64 + 2) * 64
    if dups:
        for size, pos, run, what in dup_specs():
            leaf = lay.free_leaf(q + 20)
            assert not in_sampled_stretch(leaf) and not in_sampled_stretch(leaf + 1)
            lay.place(leaf, size, "dup: " + what)
            dd[leaf] = (pos, run)
            q += 64
    if wide:
        leaf = lay.free_leaf(q + 20)
        lay.place(leaf, 8, "wide")
        ww[leaf] = 3
    return build(lay.counts, 20 if edge_keys and kt == "u64" else _SHIFT[(kt, L)], dt, dups=dd, wide=ww, edge_keys=edge_keys)


def giveup_set(pairs: int, kt: str = "u64") -> Designed:
    """`pairs` leaves of two equal keys (a duplicate pair at the leaf's border on either side) inside leaves 0 .. 511, the stretch
    k_leaf_search samples; 24 keys a leaf beside them."""
    L = 16384
    lay = Layout(L, 24)
    dd = {}
    for k in range(pairs):
        leaf = 3 + 7 * k + (2 if (3 + 7 * k) % 64 in (0, 63) else 0)
        assert leaf < C["LS_BLOCK"] - 1
        lay.place(leaf, 2, "pair")
        dd[leaf] = (0, 2)
    return build(lay.counts, _SHIFT[(kt, L)], DTYPES[kt], dups=dd)


def lanes_set(kt: str, dups: bool = False, giant: int | None = None) -> Designed:
    """The census of k_leaf_lanes and its list kernels: every size within 2 of a limit of T_LANES twice, L = 2 048; giant: L = 1 024
    and one leaf of host_min + giant keys."""
    dt = DTYPES[kt]
    if giant is not None:
        lay = Layout(1024, 24)
        for leaf, size in ((0, 31), (200, C["long_min"] + 1), (511, 17), (512, 33), (700, C["host_min"] + giant), (1023, 15)):
            lay.place(leaf, size, "giant" if size > C["host_min"] // 2 else "edge")
        return build(lay.counts, _SHIFT[(kt, 1024)], dt)
    L = 2048
    es = [C["long_min"], C["long_min"] + 1, 16, 17, 15, 32, 33]
    lay = census_layout(L, band(T_LANES), 24, dt, repeats=2, first=100, stride=3, edge_sizes=es, empties=40)
    dd = {}
    if dups:
        q = (max(p[0] for p in lay.placed if p[2].startswith("census")) // 64 + 2) * 64
        for size, pos, run, what in dup_specs() + [(5000, 4094, 4, "across long_min"), (9000, 0, 8193, "a run longer than LN_LONG_MAX")]:
            leaf = lay.free_leaf(q + 5)
            lay.place(leaf, size, "dup: " + what)
            dd[leaf] = (pos, run)
            q += 16
    return build(lay.counts, _SHIFT[(kt, L)], dt, dups=dd)


def scan_set(kt: str, dups: bool = False, avg: int | None = None, far: int | None = None, skew: bool = False) -> Designed:
    """k_spline_scan: leaves that start on the first / last key of a tile, that end on the last key of the look-ahead and one key
    either side, tiles with 63 .. 66 leaf starts, every size within 2 of a limit of T_SCAN; avg: that many keys in every leaf instead
    on average (the "shorter than a row" rule); skew: every tile is listed; far: one leaf whose end lies RMI_SC_FAR_MAX + far keys
    behind the end of the tile it starts in, among leaves longer than a tile and its look-ahead (the long-leaf instance, FAR = 2); dups: runs across a tile border and across the FHN keys
    in front of it."""
    dt = DTYPES[kt]
    tk = tile_keys(dt)
    extn = C["SC_EXTC"] * (16 // np.dtype(dt).itemsize)
    fhn = C["SC_FHC"] * (16 // np.dtype(dt).itemsize)
    if avg is not None:
        # `avg` keys a leaf on average, exactly: leaves of avg keys, one leaf that starts 10 keys in front of a tile's end and runs on
        # behind the look-ahead (the short form has to list its tile; the general form over all tiles has no list), and as many leaves
        # of avg - 1 keys behind it as the long leaf and its alignment took.
        L = 4096
        lay = Layout(L, avg)
        lay.place(1000, 10 + extn + 50, "open behind the look-ahead")
        lay.align(1000, tk, tk - 10, per_leaf=2)
        excess = int(lay.counts.sum()) - avg * L
        assert 0 < excess < 3000
        lay.counts[1001:1001 + excess] -= 1
        return build(lay.counts, _SHIFT[(kt, L)], dt)
    if skew:
        # leaves of 8 keys and of nine rows of a lane less 8, in turn: every ninth row holds two leaf starts, so the short form lists
        # every tile -- 576 of them, more than the SCAN_SKEW_LISTED = 512 above which the context takes the key set for skewed
        row = tk // 64
        return build(np.resize([8, 9 * row - 8], 8192), _SHIFT[(kt, 8192)], dt)
    if far is not None:
        # The long-leaf instance of the short form (averages above 384 keys a leaf) looks for the end of the leaf that is open at a tile's
        # end in blocks of 64 keys behind the look-ahead, the last of them ending RMI_SC_FAR_MAX keys behind the tile: a leaf whose
        # successor starts RMI_SC_FAR_MAX - 1 keys behind the end of the tile it starts in stays, one key further it is listed.  The leaf
        # starts 10 keys in front of a tile's end; the leaf behind it takes up the difference, so that nothing else moves with `far`.
        lay = Layout(1024, tk + extn + 100)
        for leaf, size in ((0, 31), (300, C["long_min"] + 1), (511, 17), (512, 33), (600, C["RMI_SC_FAR_MAX"] + 10 + far), (1023, 15)):
            lay.place(leaf, size, "far" if size > C["RMI_SC_FAR_MAX"] // 2 else "edge")
        lay.place(601, tk + extn + 100 - far, "behind far")
        lay.align(600, tk, tk - 10, per_leaf=16)
        return build(lay.counts, _SHIFT[(kt, 1024)], dt)
    L = 8192
    # (the short form is taken from 1.25 rows of a lane a leaf on average -- 20 / 40 keys --, its plain instance up to EXTN keys a leaf)
    lay = Layout(L, 48 if kt == "u32" else 24)
    lay.place(0, 17, "leaf0"); lay.place(L - 1, 33, "last"); lay.place(L // 2 - 1, 65, "split-1"); lay.place(L // 2, 129, "split"); lay.place(L // 2 + 1, 63, "split+1")
    dd = {}
    q = 200
    gap = 280 if kt == "u32" else 150                                    # (filler leaves an alignment to a tile may need, at 16 keys each)
    plan = []                                                            # (leaf, size, residue of its start inside a tile, tag, dup)
    # a leaf that starts on the first / last key of a tile; one that ends on the last key of the look-ahead, one key either side
    for size, res, tag in [(40, 0, "starts on a tile's first key"), (40, tk - 1, "starts on a tile's last key"),
                           (extn + 10 - 1, tk - 10, "ends one key inside the look-ahead's end"), (extn + 10, tk - 10, "ends on the look-ahead's last key"),
                           (extn + 10 + 1, tk - 10, "ends one key behind the look-ahead")]:
        plan.append((size, res, tag, None))
    if True:                                                             # (the same layout with and without the runs)
        plan += [(40, tk - 3, "a run across the tile border", (1, 6)), (40, tk - fhn - 2, "a run across the FHN keys in front of a tile", (0, fhn + 6) if fhn + 6 <= 40 else (0, 40)),
                 (300, tk - 100, "a long run across the tile border", (50, 120))]
    for size, res, tag, dup in plan:
        leaf = lay.free_leaf(q)
        lay.place(leaf, size, tag)
        if dup and dups:
            dd[leaf] = dup
        lay.align(leaf, tk, res, per_leaf=16)
        q = leaf + gap
    # tiles with 63 / 64 / 65 / 66 leaf starts: a tile's worth of keys cut into that many leaves, the first starting on the tile's first key
    for k in (63, 64, 65, 66):
        first = lay.free_leaf(q)
        while lay.fixed[first:first + k + 1].any():
            first += 1
        sizes = np.full(k, tk // k)
        sizes[: tk - sizes.sum()] += 1
        for m in range(k):
            lay.place(first + m, int(sizes[m]), f"tile of {k} starts")
        lay.align(first, tk, 0, per_leaf=16)
        q = first + k + gap
    lk = line_keys(dt)
    for r in range(2):
        for k, sz in enumerate(band(T_SCAN)):
            leaf = lay.free_leaf(q)
            lay.place(leaf, sz, f"census{r}")
            lay.align(leaf, lk, (3 + 5 * k + 7 * r) % lk, per_leaf=lk)
            q = leaf + 4
    assert q < L - 2
    return build(lay.counts, _SHIFT[(kt, L)], dt, dups=dd)
