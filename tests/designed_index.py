"""Hand-built models for the device index (rmi_lookup.hip): no training, every search path forced by the rows.

`DeviceIndex.from_arrays` takes any root, any leaf rows and any errors, and tests/lookup_driver.py emits and compiles the C++ for
the same arrays.  A leaf row (intercept G, slope 0) makes the guess of every query of that leaf exactly G and its error whatever
the row says, while the query's lower bound is wherever the resident keys put it: d = lower_bound - guess is the builder's to
choose.  With the keys of leaf j inside [j << s, (j + 1) << s) and the root `linear (0, 2^-s)` (exact below 2^53) or
`radix (prefix 0, bits log2 L)` (exact for every integer key) the leaf of a query is known by construction.

A `Case` carries the model, the queries and the DESIGN: the leaf every query reads (after the clamp include/rmi_hip.h documents
for the queries on which the emitted C++ is undefined) and which queries those are.  tests/test_designed_index_cpu.py checks the
design against the emitted C++ and takes the census of the classes each set was built for; tests/test_gpu_index_designed.py runs
the kernels.  numpy only; no GPU, no oracle."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from rmi_amd.train import Model

from tests import designed as D

LINEAR, CUBIC, RADIX, LOGLINEAR, NORMAL, RADIX8, BRADIX = 0, 2, 3, 5, 6, 8, 13
KTS = ("u64", "u32", "f64")
DT = D.DTYPES
U64MAX = (1 << 64) - 1
TINY = 2.0 ** -1000          # a slope that leaves every finite prediction where it is and sends an infinite query to +-inf, not NaN
# what rmi_lookup.hip was read for: (regular expression with one group, value).  test_designed_index_cpu.py reads them back.
SOURCE_CONSTANTS = {
    "LINE_BYTES": (r"constexpr uint64_t LN = (\d+) / sizeof\(K\);", D.LINE_BYTES),
    "COOP_G": (r"constexpr int COOP_G = (\d+);", 8),
}
COOP_G = SOURCE_CONSTANTS["COOP_G"][1]
BLOCK, BLOCKS_PER_CU = 256, 8                    # run(): at most 8 blocks of 256 lanes a CU, striding over the queries


@dataclass
class Case:
    name: str
    kt: str
    keys: object                 # resident keys (None: a lookup set; its trainer holds any keys of the dtype)
    n: int                       # num_rows of the model
    root: Model
    leaf_kind: int
    params: np.ndarray           # [L, ppl]
    errors: object               # [L] u64 or None
    queries: np.ndarray
    qleaf: np.ndarray            # int64: the leaf every query reads, by design
    oob: np.ndarray              # bool: the emitted C++ has no defined result (the device counts the query in root_oob)
    nan_leaf: bool = False       # the leaf predictions are NaN: the emitted FCLAMP is undefined and the driver does not say so

    @property
    def L(self) -> int:
        return len(self.params)

    @property
    def dtype(self):
        return DT[self.kt]

    def rmi(self):
        """for lookup_driver.Driver"""
        from tests import lookup_driver as ld
        err = np.zeros(self.L, dtype=np.uint64) if self.errors is None else self.errors
        return ld.as_rmi(self.root, self.leaf_kind, self.params.shape[1], self.L, self.n, self.params, err)

    def with_queries(self, q, qleaf, oob=None, name=None):
        return Case(name or self.name, self.kt, self.keys, self.n, self.root, self.leaf_kind, self.params, self.errors,
                    np.ascontiguousarray(q, dtype=self.dtype), np.asarray(qleaf, dtype=np.int64),
                    np.zeros(len(q), dtype=bool) if oob is None else np.asarray(oob, dtype=bool), self.nan_leaf)


# ---------------------------------------------------------------------------------------------------------------------------
# the design's arithmetic: the operations of the emitted lookup on rows whose products are exact (powers of two, zero, TINY)
# ---------------------------------------------------------------------------------------------------------------------------
def as_float(q) -> np.ndarray:
    """`(double) key`: round to nearest even for the integers"""
    return np.asarray(q).astype(np.float64)


def fclamp(f, bound: float) -> np.ndarray:
    """FCLAMP(f, bound) as u64; NaN -> 0 (the device's documented result; the emitted code is undefined there)"""
    f = np.asarray(f, dtype=np.float64)
    out = np.zeros(f.shape, dtype=np.uint64)
    hi = f > bound
    mid = ~(f < 0.0) & ~hi & ~np.isnan(f)
    out[hi] = np.uint64(int(bound))
    out[mid] = f[mid].astype(np.uint64)
    return out


def leaf_pred(case: Case, x=None) -> np.ndarray:
    """the leaf's prediction at every query, from the row of the designed leaf"""
    x = as_float(case.queries) if x is None else x
    p = case.params[case.qleaf]
    with np.errstate(all="ignore"):
        if p.shape[1] == 2:
            return p[:, 1] * x + p[:, 0]
        return ((p[:, 0] * x + p[:, 1]) * x + p[:, 2]) * x + p[:, 3]


def design_guess(case: Case) -> np.ndarray:
    return fclamp(leaf_pred(case), float(case.n) - 1.0)


def design_err(case: Case) -> np.ndarray:
    if case.errors is None:
        return np.zeros(len(case.queries), dtype=np.uint64)
    return case.errors[case.qleaf]


def lower_bound(keys, q) -> np.ndarray:
    """(keys < q).sum() per query: np.searchsorted(side="left") for everything but NaN, which numpy sorts behind every key and
    `<` puts in front of every key (the kernel compares with `<`, as std::lower_bound over the keys would)."""
    keys, q = np.asarray(keys), np.asarray(q)
    if keys.size * q.size <= 1 << 22:
        return (keys[None, :] < q[:, None]).sum(axis=1).astype(np.uint64)
    lb = np.searchsorted(keys, q, side="left").astype(np.uint64)
    if q.dtype == np.float64:
        lb[np.isnan(q)] = 0
    return lb


def expected_fallbacks(g, e, lb) -> np.ndarray:
    """bool per query: the lower bound lies outside [g - e, g + e]"""
    g, lb = np.asarray(g, dtype=np.uint64), np.asarray(lb, dtype=np.uint64)
    dist = np.where(g > lb, g - lb, lb - g)
    return dist > np.asarray(e, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------
# the window search of rmi_lookup.hip in Python integers: a census tool (which form of the last line of keys a query meets,
# how far it gallops).  The GPU tests never compare the kernel with it.
# ---------------------------------------------------------------------------------------------------------------------------
def _line_count(keys, n, base, ln, q, LN, info):
    if n >= LN:
        s = base if base + LN <= n else n - LN
        info["moved_left" if s != base else "at_base"] += 1
        v = [keys[s + j] for j in range(LN)]
    else:
        s = 0
        info["short_form"] += 1
        v = [keys[j if j < n else n - 1] for j in range(LN)]
    return base + sum(1 for j in range(LN) if base <= s + j < base + ln and v[j] < q)


def _lb(keys, n, base, ln, q, LN, coop, info):
    while ln > LN:
        if coop:
            w = (ln + COOP_G - 1) // COOP_G
            c = sum(1 for j in range(COOP_G) if base + (j + 1) * w - 1 < base + ln and keys[base + (j + 1) * w - 1] < q)
            nb = base + c * w
            ln = min(base + ln - nb, w - 1)
            base = nb
        else:
            half = ln >> 1
            if keys[base + half] < q:
                base, ln = base + half + 1, ln - half - 1
            else:
                ln = half
    return _line_count(keys, n, base, ln, q, LN, info)


def py_window_search(keys, g: int, e: int, q, LN: int, coop: bool = False):
    """-> (position, outside, info): window_search<COOP> for one query; info counts the forms of line_count and the gallop's steps"""
    n = len(keys)
    info = {"at_base": 0, "moved_left": 0, "short_form": 0, "steps": 0}
    a = g - e if g > e else 0
    b = n if e >= n - g else g + e
    lo, hi = (a - 1 if a > 0 else 0), (b + 1 if b < n else n)
    p = _lb(keys, n, lo, hi - lo, q, LN, coop, info)
    left, right = a > 0 and p == lo, b < n and p == hi
    if not left and not right:
        return p, False, info
    step = 1
    if left:
        h, l = lo, 0
        while h > 0:
            pr = h - step if h > step else 0
            info["steps"] += 1
            if keys[pr] < q:
                l = pr + 1
                break
            h, step = pr, step << 1
    else:
        l, h = hi, n
        while l < n:
            pr = l - 1 + step if n - l > step else n - 1
            info["steps"] += 1
            if not keys[pr] < q:
                h = pr
                break
            l, step = pr + 1, step << 1
    return _lb(keys, n, l, h - l, q, LN, coop, info), True, info


# ---------------------------------------------------------------------------------------------------------------------------
# search sets
# ---------------------------------------------------------------------------------------------------------------------------
def _rows(kt, leaf_kind, G, slope=None):
    """slope-0 rows (f64 keys: TINY, so that an infinite query predicts +-inf and not NaN)"""
    G = np.asarray(G, dtype=np.float64)
    z = np.zeros(len(G))
    t = np.full(len(G), TINY if kt == "f64" and slope is None else 0.0)
    if leaf_kind == LINEAR:
        return np.stack([G, t if slope is None else np.asarray(slope, dtype=np.float64)], axis=1)
    # (cubic: TINY in the highest coefficient -- with a zero there an infinite query gives 0 x inf = NaN whatever follows)
    return np.stack([t, z, z if slope is None else np.asarray(slope, dtype=np.float64), G], axis=1)


def _leaf_queries(keys, starts, lo_of, hi_of, dt, keep=None):
    """per leaf: its keys (keep: those of them), each key -+ 1 (f64: nextafter both ways), the first and the last value of its
    range -> (q, leaf)"""
    L = len(starts) - 1
    leaf = np.repeat(np.arange(L, dtype=np.int64), np.diff(starts.astype(np.int64)))
    if keep is not None:
        keys, leaf = keys[keep], leaf[keep]
    if dt == np.float64:
        below, above = np.nextafter(keys, -np.inf), np.nextafter(keys, np.inf)
        ok_b = ok_a = np.ones(len(keys), dtype=bool)
    else:
        one = np.array(1, dtype=dt)
        below, above = keys - one, keys + one
        ok_b, ok_a = keys > 0, keys < np.iinfo(dt).max
    j = np.arange(L, dtype=np.int64)
    q = np.concatenate([keys, below[ok_b], above[ok_a], lo_of(j), hi_of(j)])
    return q.astype(dt), np.concatenate([leaf, leaf[ok_b], leaf[ok_a], j, j])


def _shuffled(case_args, q, qleaf, oob=None, seed=1, odd=True):
    """queries in a fixed random order, so that fallbacks and scenarios are spread through the batch and a wave holds queries of
    many leaves; odd: the count is no multiple of 8 (the last cooperative group of the batch is not full)"""
    if odd and len(q) % 8 == 0:
        q, qleaf = q[:-1], qleaf[:-1]
        oob = None if oob is None else oob[:-1]
    perm = np.random.default_rng(seed).permutation(len(q))
    return q[perm], qleaf[perm], (None if oob is None else np.asarray(oob)[perm])


MAIN_L, MAIN_C, MAIN_TAIL, MAIN_TAIL_C = 4096, 64, 16, 4
MAIN_SHIFT = {"u64": 40, "f64": 40, "u32": 20}
FAR = (1 << 17) + 5000
DUP_LEAF0 = 1200


def dup_runs(kt):
    LN = D.line_keys(DT[kt])
    return [2, LN, LN + 1, 3 * LN, 1000]


def main_keys(kt) -> D.Designed:
    """64 keys a leaf; 15 leaves with a run of equal keys (4 distinct keys on either side); the last 16 leaves 4 keys each, so that
    the last line of keys is spread over leaves with rows of their own."""
    counts = np.full(MAIN_L, MAIN_C, dtype=np.int64)
    counts[MAIN_L - MAIN_TAIL:] = MAIN_TAIL_C
    dups = {}
    for i, run in enumerate(np.repeat(dup_runs(kt), 3).tolist()):
        counts[DUP_LEAF0 + 2 * i] = run + 8
        dups[DUP_LEAF0 + 2 * i] = (4, run)
    return D.build(counts, MAIN_SHIFT[kt], DT[kt], dups=dups)


def search_edges(kt):
    LN = D.line_keys(DT[kt])
    return [0, 1, 2, LN - 1, LN, LN + 1, 4 * LN + 3, 100_003]


def main_case(kt: str, variant: str, leaf_kind: int = LINEAR) -> Case:
    """The main search set of a key type.  Every leaf is a scenario (G, e); its queries sweep d = lower_bound - G over the leaf's
    positions.  Variants (same keys, same root, other rows):
      A  the last 16 leaves have windows of at most a line of keys
      B  the last 16 leaves have windows of more than a line of keys, clamped at n
      C  leaf 0 guesses 2^17 + 5000 and the last leaf n - 1 - (2^17 + 5000): the gallop runs into position 0 and into n from afar
      N  the rows of C without error rows (err = 0 for every leaf)"""
    d = main_keys(kt)
    dt, LN, n, L, s = DT[kt], D.line_keys(DT[kt]), d.n, MAIN_L, MAIN_SHIFT[kt]
    S = d.starts.astype(np.int64)
    cnt = d.counts
    mid = S[:-1] + cnt // 2
    G = mid.astype(np.float64)
    E = ((np.arange(L) % 7) * 6).astype(object)                  # unplanned leaves: e in 0, 6, .. 36 against d in -32 .. 31
    free = np.ones(L, dtype=bool)
    free[0] = free[L - MAIN_TAIL:] = False
    free[list(d.dups)] = False
    nxt = {"lo": 1, "hi": L - MAIN_TAIL - 1, "mid": L // 2}

    def take(side):
        j = nxt[side]
        while not free[j]:
            j += -1 if side == "hi" else 1
        free[j] = False
        nxt[side] = j + (-1 if side == "hi" else 1)
        return j

    def rel(dm, e):
        """a leaf whose middle key has lower_bound - G = dm"""
        j = take("hi" if dm > 0 else "lo" if dm < 0 else "mid")
        G[j], E[j] = mid[j] - dm, e
        assert 0 <= G[j] <= n - 1, (dm, e, j)

    def fixed(side, g, e):
        j = take(side)
        G[j], E[j] = g, e

    for e in search_edges(kt):                                    # window edges and the first step out, both directions
        for dm in (-(e + 1), 0, e + 1):
            rel(dm, e)
    for k in range(1, 18):                                        # gallop lengths 2^k - 1, 2^k, 2^k + 1
        for sign in (-1, 1):
            rel(sign * (k + (1 << k)), k)
    for e in (0, 1, LN, 200):                                     # clamped windows
        fixed("lo", 0.0, e)
        fixed("hi", n - 1.0, e)
    fixed("lo", 3.0, 10); fixed("hi", n - 4.0, 10)
    fixed("lo", -4.0, 500); fixed("hi", n + 1000.0, 500)          # (predictions below 0 and above n - 1)
    fixed("mid", 0.0, 5); fixed("mid", n - 1.0, 5)
    for e in (n - 1, n, n + 1, 1 << 63, U64MAX):
        j = take("mid")
        E[j] = e
    fixed("mid", 0.0, U64MAX); fixed("mid", n - 1.0, 1 << 63); fixed("mid", 0.0, n); fixed("mid", n - 1.0, n - 1)
    for i, (j, (pos, run)) in enumerate(sorted(d.dups.items())):  # the guess at the run's first, middle and last position
        G[j] = S[j] + pos + (0, run // 2, run - 1)[i % 3]
        E[j] = 1 if run == 2 else run // 3
    tail = np.arange(L - MAIN_TAIL, L)
    if variant == "B":
        G[tail], E[tail] = n - 51.0, 70
    else:
        G[tail], E[tail] = mid[tail], 3
    if variant in "CN":
        G[0], E[0] = FAR, 7
        G[L - 1], E[L - 1] = n - 1 - FAR, 7
    errors = None if variant == "N" else np.array([int(v) for v in E], dtype=np.uint64)
    w = 2.0 ** -s
    root = Model(LINEAR, (0.0, w, 0.0, 0.0))

    def lo_of(j):
        return (j.astype(np.uint64) << np.uint64(s)).astype(dt)

    def hi_of(j):
        if dt == np.float64:
            return np.nextafter(((j + 1).astype(np.uint64) << np.uint64(s)).astype(dt), -np.inf)
        return (((j + 1).astype(np.uint64) << np.uint64(s)) - np.uint64(1)).astype(dt)
    # the leaves without a scenario of their own are queried at every fourth key (their part of the batch is filler)
    kleaf = np.repeat(np.arange(L), cnt)
    keep = ~free[kleaf] | ((np.arange(n) - S[kleaf]) % 4 == 0)
    q, ql = _leaf_queries(d.keys, d.starts, lo_of, hi_of, dt, keep)
    top = np.finfo(dt).max if dt == np.float64 else np.iinfo(dt).max
    extra = [0, top] + ([-0.0] if dt == np.float64 else [])
    q = np.concatenate([q, np.array(extra, dtype=dt)])
    ql = np.concatenate([ql, np.array([0, L - 1] + [0] * (len(extra) - 2), dtype=np.int64)])
    case = Case(f"main-{variant}-{kt}", kt, d.keys, n, root, leaf_kind, _rows(kt, leaf_kind, G), errors, q, ql, None)
    q, ql, _ = _shuffled(None, q, ql, seed=11)
    return case.with_queries(q, ql)


def high_case(kt: str = "u64", leaf_kind: int = LINEAR) -> Case:
    """u64 / u32 keys over the whole range of the type, on both sides of its middle (2^63 / 2^31), the first key 0 and the last the
    type's maximum; radix root (prefix 0 / 32, 12 bits): exact for every key"""
    W = {"u64": 64, "u32": 32}[kt]
    dt = DT[kt]
    L, c, s = 4096, 64, W - 12
    n = L * c
    j = np.repeat(np.arange(L, dtype=np.uint64), c)
    i = np.tile(np.arange(c, dtype=np.uint64), L)
    keys = (j << np.uint64(s)) + (((np.uint64(2) * i + np.uint64(1)) << np.uint64(s)) >> np.uint64(7)) + (i * np.uint64(37) + j) % np.uint64(1021)
    keys[0], keys[-1] = 0, np.uint64((1 << W) - 1)
    assert np.all(keys[1:] > keys[:-1]) and np.array_equal(keys >> np.uint64(s), j)
    keys = keys.astype(dt)
    LN = D.line_keys(dt)
    starts = np.arange(L + 1, dtype=np.uint64) * np.uint64(c)
    mid = starts[:-1].astype(np.int64) + c // 2
    dms = [0, 1, -1, 33, -33, 40, -40, 300, -300, 5000, -5000, 70000, -70000]
    es = [0, 1, LN, 37, 1 << 63, U64MAX, 2]
    G = np.clip(mid - np.array([dms[k % len(dms)] for k in range(L)]), 0, n - 1).astype(np.float64)
    E = [es[k % len(es)] for k in range(L)]
    G[0], E[0] = FAR, 7
    G[L - 1], E[L - 1] = n - 1 - FAR, 7
    q, ql = _leaf_queries(keys, starts, lambda t: (t.astype(np.uint64) << np.uint64(s)).astype(dt),
                          lambda t: ((t.astype(np.uint64) << np.uint64(s)) + np.uint64((1 << s) - 1)).astype(dt), dt)
    case = Case(f"high-{kt}", kt, keys, n, Model(RADIX, ip=(64 - W, 12)), leaf_kind, _rows(kt, leaf_kind, G),
                np.array([np.uint64(v) for v in E], dtype=np.uint64), q, ql, None)
    q, ql, _ = _shuffled(None, q, ql, seed=12)
    return case.with_queries(q, ql)


F64_SPECIALS = [-1e-310, -5e-324, -0.0, 0.0, 5e-324, 1e-310, 2.2250738585072014e-308]


def f64_case(leaf_kind: int = LINEAR) -> Case:
    """f64 keys on both sides of zero: negative keys, -0.0 and 0.0 both resident, denormals; queries -0.0, 0.0, +-inf, NaN.
    Root linear (32, 2^-10) over 64 leaves: leaf j holds [(j - 32) * 1024, (j - 31) * 1024)."""
    L, c, s = 64, 64, 10
    base = (np.arange(L, dtype=np.float64) - L // 2) * 1024.0
    keys = (base[:, None] + (2.0 * np.arange(c) + 1.0) * 8.0).reshape(-1)
    at = np.searchsorted(keys, 0.0)
    keys = np.concatenate([keys[:at], np.array(F64_SPECIALS), keys[at:]])
    assert np.all(keys[1:] >= keys[:-1])
    n = len(keys)
    root = Model(LINEAR, (float(L // 2), 2.0 ** -s, 0.0, 0.0))

    def leaf_of(x):
        with np.errstate(all="ignore"):
            return fclamp(2.0 ** -s * x + float(L // 2), L - 1.0).astype(np.int64)
    specials = np.array([-0.0, 0.0, -np.inf, np.inf, np.nan, np.finfo(np.float64).max, -np.finfo(np.float64).max, 1e-320, -1e-320])
    q = np.concatenate([keys, np.nextafter(keys, -np.inf), np.nextafter(keys, np.inf), base, np.nextafter(base + 1024.0, -np.inf),
                        specials])
    ql = leaf_of(q)
    kl = leaf_of(keys)
    first = np.searchsorted(kl, np.arange(L))
    cnt = np.diff(np.append(first, n))
    mid = first + cnt // 2
    dms = [0, 1, -1, 5, -5, 17, -17, 33, -33, 100, -100, 1000, -1000]
    es = [0, 1, 2, 16, 50]
    G = np.clip(mid - np.array([dms[k % len(dms)] for k in range(L)]), 0, n - 1).astype(np.float64)
    E = np.array([es[k % len(es)] for k in range(L)], dtype=np.uint64)
    case = Case("signed-f64", "f64", keys, n, root, leaf_kind, _rows("f64", leaf_kind, G), E, q, ql, None)
    q, ql, oob = _shuffled(None, q, ql, np.isnan(q), seed=13)
    return case.with_queries(q, ql, oob)


SHORT_T0, SHORT_COMBOS = 100, 20


def short_ns(kt):
    LN = D.line_keys(DT[kt])
    return [1, 2, LN - 1, LN, LN + 1, 2 * LN - 1, 2 * LN, 2 * LN + 1]


def short_keys(kt, n: int, rot: int) -> np.ndarray:
    """key i = (i + 1) * 256 + c_i with c_i = 100 + (i + rot) % 20: the low byte of a query picks the leaf -- the scenario --, so
    over the 20 rotations every key is a present query of every scenario"""
    i = np.arange(n, dtype=np.uint64)
    return (((i + np.uint64(1)) << np.uint64(8)) + np.uint64(SHORT_T0) + (i + np.uint64(rot)) % np.uint64(SHORT_COMBOS)).astype(DT[kt])


def short_case(kt: str, n: int, leaf_kind: int = LINEAR) -> Case:
    """Key sets shorter than, equal to and just longer than one and two lines of keys.  Root radix (prefix 56, 8 bits): leaf = the
    query's low byte t.  Leaf t: guess 0, n/2, n - 1 or (t % 4 == 3) a guess that sweeps against the lower bound -- the line
    n + 1/2 - q / 256 --; err 0, 1, LN, n or 2^64 - 1 by (t / 4) % 5.  Queries: every block b = 0 .. n + 1 with the low bytes 80 .. 139,
    so each key has queries below, on and above it in every one of the 20 scenarios.  keys: rotation 0 (short_keys gives the others)."""
    LN = D.line_keys(DT[kt])
    t = np.arange(256)
    G = np.select([t % 4 == 0, t % 4 == 1, t % 4 == 2], [0.0, float(n // 2), n - 1.0], n + 0.5)
    slope = np.where(t % 4 == 3, -(2.0 ** -8), 0.0)
    E = np.array([[0, 1, LN, n, U64MAX][(v // 4) % 5] for v in t.tolist()], dtype=np.uint64)
    b = np.repeat(np.arange(n + 2, dtype=np.uint64), 60)
    tt = np.tile(np.arange(80, 140, dtype=np.uint64), n + 2)
    q = ((b << np.uint64(8)) + tt).astype(DT[kt])
    case = Case(f"short-{n}-{kt}", kt, short_keys(kt, n, 0), n, Model(RADIX, ip=(56, 8)), leaf_kind, _rows(kt, leaf_kind, G, slope), E,
                q, tt.astype(np.int64), None)
    q, ql, _ = _shuffled(None, q, tt.astype(np.int64), seed=n, odd=False)
    return case.with_queries(q, ql)


def verify_case(kt: str, outside: str) -> Case:
    """rows over the main keys whose count of keys outside the bound is designed: "0", "1" or "n"; the queries are the keys"""
    d = main_keys(kt)
    S, cnt, n = d.starts.astype(np.int64), d.counts, d.n
    G = (S[:-1] + cnt // 2).astype(np.float64)
    E = cnt.astype(np.uint64)                                     # |lower bound - G| <= the leaf's key count
    if outside == "1":
        E[7] = MAIN_C // 2 - 1                                    # 64 distinct keys at d = -32 .. 31: the first one is outside
    elif outside == "n":
        G = (G + n // 2) % n
        E[:] = 0
    ql = np.repeat(np.arange(MAIN_L, dtype=np.int64), cnt)
    return Case(f"verify-{outside}-{kt}", kt, d.keys, n, Model(LINEAR, (0.0, 2.0 ** -MAIN_SHIFT[kt], 0.0, 0.0)), LINEAR,
                _rows(kt, LINEAR, G), E, d.keys.copy(), ql, np.zeros(n, dtype=bool))


# ---------------------------------------------------------------------------------------------------------------------------
# lookup sets: hand-set roots
# ---------------------------------------------------------------------------------------------------------------------------
LK_L, LK_N = 12, 1_000_003
LK_ERR = np.array([0, 1, U64MAX, 1 << 63, 17, 2, 3, 1 << 32, 5, 6, 7, LK_N], dtype=np.uint64)


def lookup_G(n=LK_N):
    """leaf predictions: negative, in (-1, 0), in (n - 2, n - 1), n - 1, above n - 1, above 2^64, -inf, +inf, -0.0 (the first and the
    last leaf, where infinite queries land, stay finite)"""
    return np.array([12345.0, -7.0, -0.5, n - 1.5, n - 1.0, n + 9.0, 2.0 ** 65, -np.inf, np.inf, -0.0, 1.0, n - 2.0])


def _lookup_rows(leaf_kind, G):
    """TINY in the highest coefficient: an infinite query gives an infinite prediction, a finite one G"""
    t, z = np.full(len(G), TINY), np.zeros(len(G))
    return np.stack([G, t], axis=1) if leaf_kind == LINEAR else np.stack([t, z, z, G], axis=1)


def exp1(v):
    v = 1.0 + v / 64.0
    for _ in range(6):
        v = v * v
    return v


def float_root_raw(root: Model, x):
    """the raw prediction of a float root, operation by operation as the emitted code has it (every product here is exact or
    the only rounding of its fma)"""
    p = root.p
    with np.errstate(all="ignore"):
        if root.kind == LINEAR:
            return p[1] * x + p[0]
        if root.kind == CUBIC:
            return ((p[0] * x + p[1]) * x + p[2]) * x + p[3]
        if root.kind == LOGLINEAR:
            return exp1(p[1] * x + p[0])
        assert root.kind == NORMAL
        return 1.0 / (1.0 + exp1(-1.65451 * ((x - p[0]) / p[1]))) * p[2]


def float_root_leaf(root: Model, f, L):
    """-> (leaf, oob): FCLAMP for the roots with a bounds check (undefined: NaN), `(uint64_t) fpred` for cubic (defined for
    -1 < fpred < L; the device clamps the rest to leaf 0 or L - 1)"""
    nan = np.isnan(f)
    if root.kind != CUBIC:
        return fclamp(f, L - 1.0).astype(np.int64), nan
    ok = (f > -1.0) & (f < float(L))
    leaf = np.where(ok, np.trunc(np.where(ok, f, 0.0)), np.where(f >= float(L), L - 1.0, 0.0)).astype(np.int64)
    return leaf, ~ok


def _float_queries(kt, root_kind, L):
    """queries whose raw prediction x / 256 + alpha sits at -1, just above -1, -0.0, every leaf, L - 1, just below L, L and far above"""
    if kt == "f64":
        xs = [-256.0, np.nextafter(-256.0, 0.0), -255.0, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1e-310, 255.0]
        for l in range(L + 1):
            xs += [256.0 * l + o for o in [0.5, 1.0, 17.25, 100.5, 127.0, 129.0, 254.0, 255.0, 255.5] + list(range(0, 256, 8))]
            xs += [np.nextafter(256.0 * l, np.inf), np.nextafter(256.0 * (l + 1), 0.0)]
        xs += [256.0 * (L + 1), 2.0 ** 40, 2.0 ** 63, 2.0 ** 64, 1e300, -1e300, -np.inf, np.inf, np.nan, -512.0]
        return np.array(xs)
    xs = [0, 1, 255]
    for l in range(L + 1):
        xs += [256 * (l + 1) + o for o in [1, 2, 17, 127, 129, 253, 254, 255] + list(range(0, 256, 8))]
    xs += [256 * (L + 2), 1 << 31, (1 << 32) - 1]
    if kt == "u64":
        xs += [1 << 40, (1 << 53) + 1, (1 << 63) - 1, 1 << 63, U64MAX]
    return np.array([np.uint64(v) for v in xs]).astype(DT[kt])


def _scan_queries(kt, hi=12000, step=7):
    if kt == "f64":
        return np.concatenate([np.arange(0, hi, step) + 0.25, [-0.0, -5e-324, 1e-310, -300.5, -1e300, 1e300, 2.0 ** 63, -np.inf, np.inf, np.nan]])
    top = [1 << 31, (1 << 32) - 1] + ([1 << 40, (1 << 53) + 1, 1 << 63, U64MAX] if kt == "u64" else [])
    return np.concatenate([np.arange(0, hi, step, dtype=DT[kt]), np.array(top, dtype=DT[kt])])


def _weighted(q, leaf, oob):
    """every defined query, and of the undefined ones so many that at least 90 % of the set is defined"""
    keep = ~oob
    und = np.flatnonzero(oob)
    k = min(len(und), max(1, int(keep.sum()) // 12))
    if len(und):
        keep[und[np.unique(np.linspace(0, len(und) - 1, k).round().astype(int))]] = True
    return q[keep], leaf[keep], oob[keep]


def _radix_queries(kt, prefix, field_bits, field_shift, variants=16):
    """queries whose bits [field_shift, field_shift + field_bits) run through every value t, with `variants` settings of the bits
    below the field and of the bits above it (which the root's prefix shifts out); every query fits the key type -> (q, t)"""
    W = {"u64": 64, "u32": 32, "f64": 53}[kt]
    hi_bits = W - (field_shift + field_bits)
    assert hi_bits >= 0 and 64 - prefix == field_shift + field_bits
    rng = np.random.default_rng(prefix * 64 + field_bits)
    qs, ts = [], []
    for t in range(1 << field_bits):
        for v in range(variants):
            # v = 0: every other bit clear; v = 1: every other bit set; else random
            lo = 0 if v == 0 else (1 << field_shift) - 1 if v == 1 else int(rng.integers(0, 1 << field_shift)) if field_shift else 0
            hi = 0 if v == 0 else (1 << hi_bits) - 1 if v == 1 else int(rng.integers(0, 1 << hi_bits)) if hi_bits else 0
            x = (hi << (field_shift + field_bits)) | (t << field_shift) | lo
            assert x < (1 << W)
            qs.append(x)
            ts.append(t)
    q = np.array([np.uint64(v) for v in qs], dtype=np.uint64)
    if kt == "f64":
        assert all(int(float(x)) == x for x in qs)
    return q.astype(DT[kt]), np.array(ts, dtype=np.int64)


def lookup_cases(kt: str) -> list:
    """Every root function of rmi_lookup.hip on hand-set parameters; linear and cubic leaf rows, with and without error rows."""
    L, n, W = LK_L, LK_N, {"u64": 64, "u32": 32, "f64": 53}[kt]
    ki = KTS.index(kt)
    out = []

    def add(name, root, q, leaf, oob, idx):
        q, leaf, oob = _weighted(np.asarray(q, dtype=DT[kt]), np.asarray(leaf, dtype=np.int64), np.asarray(oob, dtype=bool))
        flip = (idx + ki) % 2
        for leaf_kind, with_err in ((LINEAR, not flip), (CUBIC, bool(flip))):
            nm = f"{name}-{'linear' if leaf_kind == LINEAR else 'cubic'}-{'err' if with_err else 'noerr'}-{kt}"
            out.append(Case(nm, kt, None, n, root, leaf_kind, _lookup_rows(leaf_kind, lookup_G()), LK_ERR.copy() if with_err else None,
                            q, leaf, oob))

    # the float roots: raw prediction x / 256 + alpha (f64 queries: alpha = -0.0 and negative queries; integers: alpha = -1)
    alpha = -0.0 if kt == "f64" else -1.0
    roots = [("linear", Model(LINEAR, (alpha, 2.0 ** -8, 0.0, 0.0)), _float_queries(kt, LINEAR, L)),
             ("cubic", Model(CUBIC, (0.0, 0.0, 2.0 ** -8, alpha)), _float_queries(kt, CUBIC, L)),
             ("loglinear", Model(LOGLINEAR, (-16.0, 2.0 ** -12, 0.0, 0.0)), _scan_queries(kt, hi=90000, step=50)),
             ("normal", Model(NORMAL, (5000.0, 1000.0, L + 2.0, 0.0)), _scan_queries(kt, step=13))]
    for idx, (name, root, q) in enumerate(roots):
        leaf, oob = float_root_leaf(root, float_root_raw(root, as_float(q)), L)
        add(name, root, q, leaf, oob, idx)
    # the radix family: 4-bit field t right under the bits the prefix shifts out.  p0: nothing of the key type is shifted out
    # (u64: prefix 0); p0 + 4: the four high bits of the query are set and shifted out
    p0 = 64 - W
    idx = len(roots)
    for prefix in (p0, p0 + 4):
        q, t = _radix_queries(kt, prefix, 4, 64 - prefix - 4)
        add(f"radix-p{prefix}", Model(RADIX, ip=(prefix, 4)), q, np.minimum(t, L - 1), t >= L, idx)
        idx += 1
        for high, clamps in ((1, (L - 3, L - 1)), (0, (2, L - 1))):
            for cl in clamps:
                raw = np.minimum(t, cl) if high else np.where(t < cl, 0, t - cl)
                if prefix == p0 and cl == L - 1:
                    continue                                     # (each clamp with one prefix)
                if prefix != p0 and cl != L - 1:
                    continue
                add(f"bradix-{'high' if high else 'low'}-c{cl}-p{prefix}", Model(BRADIX, ip=(prefix, 4, cl, high)), q,
                    np.minimum(raw, L - 1), raw >= L, idx)
                idx += 1
    # radix tables (radix8): prefix + 8 < 64 and = 64; the table is the test's: entries 0 .. L + 3
    table = ((np.arange(256) * 7) % (L + 4)).astype(np.uint32)
    for prefix in (p0 + 4, 56):
        q, t = _radix_queries(kt, prefix, 8, 64 - prefix - 8, variants=6)
        raw = table[t].astype(np.int64)
        add(f"table-p{prefix}", Model(RADIX8, ip=(prefix, 8), table=table), q, np.minimum(raw, L - 1), raw >= L, idx)
        idx += 1
    return out


def precision_cases() -> list:
    """u64 queries around 2^53 and 2^63 under a slope that makes one ulp of `(double) key` visible in the guess: radix root
    (prefix 0, 4 bits), leaf 0 (keys below 2^60) slope 1/2, the others 2^-11; n = 2^62."""
    qs = [(1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 53) + 3]
    for k in list(range(1, 12)) + [20, 31, 32, 33, 40, 52]:
        qs += [(1 << 53) + (1 << k) - 1, (1 << 53) + (1 << k) + 1]
    for b in (1 << 63, (1 << 63) + (1 << 62), 1 << 60, (1 << 64) - (1 << 12)):
        qs += [b - 1, b, b + 1, b + 1023, b + 1024, b + 1025, b + 3071, b + 3072, b + 3073, b + (1 << 32) + 1025]
    qs += [U64MAX, U64MAX - 1023, U64MAX - 1024, 0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1]
    q = np.array([np.uint64(v) for v in qs if v <= U64MAX], dtype=np.uint64)
    leaf = (q >> np.uint64(60)).astype(np.int64)
    slope = np.full(16, 2.0 ** -11)
    slope[0] = 0.5
    z = np.zeros(16)
    out = []
    for leaf_kind, rows in ((LINEAR, np.stack([z, slope], axis=1)), (CUBIC, np.stack([z, z, slope, z], axis=1))):
        out.append(Case(f"precision-{'linear' if leaf_kind == LINEAR else 'cubic'}-u64", "u64", None, 1 << 62, Model(RADIX, ip=(0, 4)), leaf_kind,
                        rows, np.arange(16, dtype=np.uint64), q, leaf, np.zeros(len(q), dtype=bool)))
    return out


def nan_cases() -> list:
    """A set of their own: NaN leaf predictions (an infinite f64 query on a row of slope exactly 0: inf x 0), and the NaN root of
    a linear root of slope 0.  The emitted FCLAMP is undefined on a NaN and the driver does not flag a NaN leaf: these are compared
    with the documented device result only -- guess 0, a NaN root counted in root_oob, a NaN leaf not."""
    L, n = 4, 1000
    G = np.array([10.0, 20.0, 30.0, 40.0])
    z = np.zeros(L)
    out = []
    for leaf_kind, rows in ((LINEAR, np.stack([G, z], axis=1)), (CUBIC, np.stack([z, z, z, G], axis=1))):
        nm = "linear" if leaf_kind == LINEAR else "cubic"
        # root of slope 1: +-inf -> leaf L - 1 / 0 (defined), the leaf predicts inf x 0 = NaN
        q = np.array([0.5, 1.5, 2.5, 3.5, np.inf, -np.inf, 2.0, np.inf])
        out.append(Case(f"nan-leaf-{nm}", "f64", None, n, Model(LINEAR, (0.0, 1.0, 0.0, 0.0)), leaf_kind, rows, np.arange(L, dtype=np.uint64) + 5,
                        q, np.array([0, 1, 2, 3, 3, 0, 2, 3]), np.zeros(len(q), dtype=bool), nan_leaf=True))
        # root of slope 0: every finite query -> leaf 2; +-inf and NaN -> a NaN root: leaf 0, root_oob
        q = np.array([0.5, np.inf, 7.0, -np.inf, np.nan, -3.0])
        out.append(Case(f"nan-root-{nm}", "f64", None, n, Model(LINEAR, (2.0, 0.0, 0.0, 0.0)), leaf_kind, rows, np.arange(L, dtype=np.uint64) + 5,
                        q, np.array([2, 0, 2, 0, 0, 2]), np.array([False, True, False, True, True, False]), nan_leaf=True))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# batch shapes
# ---------------------------------------------------------------------------------------------------------------------------
BATCH_SIZES = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257)


def big_batch_size(cus: int) -> int:
    """more than two trips of the grid-stride loop for the one-query-per-lane variant, and no multiple of 8"""
    return 2 * cus * BLOCKS_PER_CU * BLOCK + 12345


def tiled(case: Case, nq: int) -> Case:
    reps = -(-nq // len(case.queries))
    return case.with_queries(np.tile(case.queries, reps)[:nq], np.tile(case.qleaf, reps)[:nq], np.tile(case.oob, reps)[:nq])


def compile_drivers(cases, workdir, jobs: int = 8) -> dict:
    """name -> lookup_driver.Driver, compiled `jobs` at a time"""
    import os
    from concurrent.futures import ThreadPoolExecutor
    from tests import lookup_driver as ld

    def one(c):
        p = os.path.join(str(workdir), c.name)
        os.makedirs(p, exist_ok=True)
        return c.name, ld.Driver(c.rmi(), c.dtype, p, with_errors=c.errors is not None)
    with ThreadPoolExecutor(jobs) as ex:
        return dict(ex.map(one, cases))


# ---------------------------------------------------------------------------------------------------------------------------
# the sets by key type
# ---------------------------------------------------------------------------------------------------------------------------
def search_cases(kt: str) -> list:
    """the search sets of a key type that share one key set each: main A / B / C / N (linear and cubic rows in turn), u64: the
    high keys, f64: the keys around zero"""
    out = [main_case(kt, v, (LINEAR, CUBIC)[i % 2]) for i, v in enumerate("ABCN")]
    if kt != "f64":
        out.append(high_case(kt))
    if kt == "f64":
        out.append(f64_case(CUBIC))
    return out


def short_cases(kt: str) -> list:
    return [short_case(kt, n, (LINEAR, CUBIC)[i % 2]) for i, n in enumerate(short_ns(kt))]


def lookup_sets(kt: str) -> list:
    return lookup_cases(kt) + (precision_cases() if kt == "u64" else [])


def driver_cases(kt: str) -> list:
    return search_cases(kt) + short_cases(kt) + lookup_sets(kt)
