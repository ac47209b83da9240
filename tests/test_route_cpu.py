"""The route planner on the CPU: tests/route_check.cpp includes rmi_amd/csrc/rmi_route.h (plain C++17) and prints plan_route's
decision for every line of input.  The rows of DESIGN.md §4's dispatch table, the boundaries around them, the knobs the GPU tests
set, and what RouteMemory remembers between trainings."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIM = (1 << 32) - (1 << 16)                      # the 32-bit index kernels take key sets below this


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route") / "route_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "route_check.cpp"), "-o", exe], check=True)
    return exe


def plan(driver, *lines, **env):
    """the route of every line (a dict of ints); env: RMI_HIP_* knobs without the prefix"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("RMI_HIP_")}
    e.update({"RMI_HIP_" + k: str(v) for k, v in env.items()})
    out = subprocess.run([driver], input="\n".join(lines) + "\n", env=e, check=True, capture_output=True, text=True).stdout
    return [{k: (float(v) if k == "cubic_margin_scale" else int(v)) for k, v in (w.split("=") for w in ln.split())} for ln in out.strip().split("\n")]


def one(driver, line, **env):
    return plan(driver, line, **env)[0]


M = "root=linear leaf=linear key=u64 n=200000000 L=1048576"          # 190 keys a leaf
C2 = "root=linear leaf=linear key=u64 n=200000000 L=262144"          # 763
C3 = "root=cubic leaf=linear key=u64 n=200000000 L=1048576"
C4S = "root=linear leaf=linear key=u64 n=100000000 L=262144"         # 381
C5 = "root=radix leaf=linear_spline key=u32 n=400000000 L=4194304"
MS = "root=linear leaf=linear key=u64 n=25000000 L=131072"           # 2 048 groups on 1 024 resident waves
U32 = "root=linear leaf=linear key=u32 n=400000000 L=2097152"


def test_design_table_pipeline5(driver):
    for root in ("linear", "radix", "cubic", "radix8", "bradix", "normal", "loglinear"):
        for key in ("u64", "u32", "f64"):
            for n, L in ((200_000_000, 1 << 20), (500, 64), (LIM - 1, 1 << 20)):
                r = one(driver, f"root={root} leaf=linear_spline key={key} n={n} L={L}")
                assert (r["pipeline"], r["sigma"], r["search"], r["init_arrays"], r["fused"], r["regs"]) == (5, 0, 0, 0, 1, -1), (root, key, n)
    r = one(driver, f"{C5} n_it=0")                                     # an empty shard
    assert r["pipeline"] == 5
    # the short form of a tile: roots monotone by arithmetic
    assert one(driver, C5)["scan_mono"] == 1 and one(driver, C5 + " prefix=0")["scan_mono"] == 0
    assert one(driver, "root=linear leaf=linear_spline n=1000000 L=4096")["scan_mono"] == 1
    assert one(driver, "root=linear leaf=linear_spline n=1000000 L=4096 slope_ok=0")["scan_mono"] == 0
    assert one(driver, "root=cubic leaf=linear_spline n=1000000 L=4096")["scan_mono"] == 0


def test_design_table_pipeline4(driver):
    for root, extra in (("linear", ""), ("radix", ""), ("bradix", ""), ("cubic", "")):
        r = one(driver, M.replace("root=linear", f"root={root}") + extra)
        assert (r["pipeline"], r["regs"], r["search"], r["init_folded"], r["optimistic"], r["listed_late"]) == (4, 0, 1, 1, 1, 1), root
        assert r["regs_grid"] == 1024
    assert one(driver, C3)["cubic_margin"] == 1 and one(driver, C3)["verify"] == 0
    assert one(driver, M + " key=f64")["regs"] == 0
    assert (one(driver, C4S)["pipeline"], one(driver, C4S)["regs"]) == (4, 1)          # LONG
    r = one(driver, U32)
    assert (r["pipeline"], r["regs"], r["regs_grid"]) == (4, 2, 2048)                 # two waves per SIMD
    # roots the search does not serve still take k_leaf_regs, behind the bucketing scan + fill
    for root in ("radix8", "normal", "loglinear"):
        r = one(driver, M.replace("root=linear", f"root={root}"))
        assert (r["pipeline"], r["regs"], r["search"], r["init_arrays"]) == (4, 0, 0, 1), root
    r = one(driver, M.replace("root=linear", "root=radix") + " prefix=0")
    assert (r["pipeline"], r["search"]) == (4, 0)
    r = one(driver, C3 + " cubic_finite=0")
    assert (r["pipeline"], r["search"], r["verify"]) == (4, 0, 0)


def test_design_table_pipeline3(driver):
    for line in (C2, "root=linear leaf=linear key=u64 n=1000000 L=1024", MS, U32.replace("L=2097152", "L=262144")):
        r = one(driver, line)
        assert (r["pipeline"], r["regs"], r["search"], r["fused"]) == (3, -1, 1, 1), line
    r = one(driver, C3 + " increasing=0")                              # k_leaf_lanes<.., K_CUBIC> verifies every key
    assert (r["pipeline"], r["search"], r["verify"], r["cubic_margin"]) == (3, 1, 1, 0)
    # ... as does an increasing cubic wherever k_leaf_regs is not taken: long leaves, the groups-per-wave rule, RMI_HIP_REGS=0
    for line, env in ((C3.replace("L=1048576", "L=262144"), {}), ("root=cubic leaf=linear key=u64 n=25000000 L=131072", {}), (C3, {"REGS": 0})):
        r = one(driver, line, **env)
        assert (r["pipeline"], r["search"], r["verify"], r["cubic_margin"]) == (3, 1, 1, 0), line
    r = one(driver, C2.replace("root=linear", "root=radix8"))
    assert (r["pipeline"], r["search"], r["init_arrays"]) == (3, 0, 1)


def test_design_table_pipeline2(driver):
    for leaf in ("cubic", "robust_linear"):
        for root in ("linear", "cubic", "radix", "radix8"):
            r = one(driver, f"root={root} leaf={leaf} n=200000000 L=1048576")
            assert (r["pipeline"], r["sigma"], r["fused"], r["init_arrays"], r["giants"]) == (2, 0, 0, 1, 0), (root, leaf)
            assert r["asked_prefix"] == r["asked_increasing"] == 0
    for n in (0, 1, 1023):                                               # n < 1 024: the streaming passes
        assert one(driver, f"root=linear leaf=linear n={n} L=64")["pipeline"] == 2
    assert one(driver, "root=linear leaf=linear n=1024 L=64")["pipeline"] == 4
    r = one(driver, "root=linear leaf=linear n=200000000 L=1048576 fit_mode=1")
    assert (r["pipeline"], r["sigma"], r["giants"], r["giants_early"]) == (2, 1, 1, 1)
    assert one(driver, "root=linear leaf=linear n=200000000 L=1048576 fit_mode=2")["sigma"] == 1
    assert one(driver, "root=linear leaf=linear n=200000000 L=8000000 fit_mode=1")["sigma"] == 0      # < 32 keys a leaf
    assert one(driver, "root=linear leaf=linear n=4095 L=16 fit_mode=1")["sigma"] == 0


def test_huge_key_sets(driver):
    """n >= 2^32 - 2^16: linear leaves through the unfused k_leaf_lanes (k_err_range + k_finalize behind it), pipeline 3; the others
    through the streaming passes"""
    for n in (LIM, 1 << 33):
        r = one(driver, f"root=linear leaf=linear n={n} L=16777216")
        assert (r["pipeline"], r["fused"], r["search"], r["optimistic"], r["giants"], r["regs"], r["init_arrays"]) == (3, 0, 1, 0, 0, -1, 1)
        r = one(driver, f"root=linear leaf=linear n={n} L=16777216 fit_mode=1")
        assert (r["pipeline"], r["sigma"], r["fused"]) == (3, 0, 0)
        for leaf in ("linear_spline", "cubic", "robust_linear"):
            r = one(driver, f"root=linear leaf={leaf} n={n} L=16777216")
            assert (r["pipeline"], r["fused"]) == (2, 0), leaf
    r = one(driver, f"root=cubic leaf=linear n={LIM} L=16777216")
    assert (r["pipeline"], r["search"], r["verify"]) == (3, 0, 0)
    assert one(driver, f"root=linear leaf=linear n={LIM - 1} L=16777216")["fused"] == 1


def test_groups_per_wave_rule(driver):
    """between one and two and a half groups of 64 leaves per resident wave (4 per CU) k_leaf_lanes; not for LONG leaves, not with
    RMI_HIP_REGS=1 or RMI_HIP_REGS_GRID"""
    for groups, pipe in ((1024, 4), (1025, 3), (2560, 3), (2561, 4)):
        L = groups * 64
        assert one(driver, f"root=linear leaf=linear n={L * 190} L={L}")["pipeline"] == pipe, groups
    assert one(driver, f"root=linear leaf=linear n={2048 * 64 * 190} L={2048 * 64} n_cu=512")["pipeline"] == 4
    assert one(driver, f"root=linear leaf=linear n={2048 * 64 * 381} L={2048 * 64}")["pipeline"] == 4      # LONG
    assert one(driver, MS, REGS=1)["pipeline"] == 4
    assert one(driver, MS, REGS_GRID=700)["pipeline"] == 4
    assert one(driver, M, REGS_GRID=700)["regs_grid"] == 700


def test_knob_overrides(driver):
    assert one(driver, M, PIPELINE=2)["pipeline"] == 2
    assert one(driver, C5, PIPELINE=2)["pipeline"] == 2
    assert one(driver, M, PIPELINE=3)["pipeline"] == 4
    assert (one(driver, M, REGS=0)["pipeline"], one(driver, M, REGS=1)["pipeline"]) == (3, 4)
    assert one(driver, U32, REGS_U32=0)["pipeline"] == 3
    assert (one(driver, U32, REGS_U32=1)["regs"], one(driver, U32, REGS_U32=2)["regs"]) == (0, 2)
    r = one(driver, M, OPT_TAIL=0)
    assert (r["optimistic"], r["listed_late"], r["giants_early"], r["pipeline"]) == (0, 0, 0, 4)
    r = one(driver, M, LANES_SEARCH=0)
    assert (r["search"], r["init_arrays"], r["pipeline"]) == (0, 1, 4)
    r = one(driver, M.replace("root=linear", "root=radix"), LANES_SEARCH=0)
    assert (r["search"], r["asked_prefix"]) == (0, 0)
    assert one(driver, C5, LANES_SEARCH=0)["asked_prefix"] == 1                         # (the scan asks anyway)
    r = one(driver, C3, CUBIC_MARGIN=0)
    assert (r["pipeline"], r["verify"], r["asked_increasing"]) == (3, 1, 0)
    assert (one(driver, C5, LEAN=0)["lean"], one(driver, C5)["lean"]) == (0, 1)
    for extra in (" stream=1", " defer=1", " rows_ext=1"):
        assert one(driver, C5 + extra)["lean"] == 0
    # giant leaves: only where the average leaf is far below the threshold -- or wherever RMI_HIP_HOST_MIN says
    few = "root=linear leaf=linear key=u32 n=400000000 L=1024"
    assert one(driver, few)["giants"] == 0 and one(driver, few, HOST_MIN=262144)["giants"] == 1
    assert one(driver, M, HOST_MIN=0)["giants"] == 0
    assert one(driver, M + " defer=1")["giants"] == 0 and one(driver, M + " stream=1")["giants"] == 0
    r = one(driver, M + " defer=1")
    assert (r["optimistic"], r["listed_late"]) == (1, 0)
    r = one(driver, M + " peers=3")
    assert (r["peers"], r["listed_late"]) == (1, 0)


def test_read_knobs(driver):
    k = plan(driver, "knobs", PIPELINE=5, LONG_MIN=10, HOST_MIN=1000, REGS=1, CUBIC_MARGIN_SCALE="1e13", FIT_THREADS=4096)[0]
    assert (k["pipeline"], k["long_min"], k["host_min"], k["host_min_set"], k["regs"], k["regs_forced"]) == (3, 4096, 1000, 1, 1, 1)
    assert (k["cubic_margin_scale"], k["fit_threads"]) == (1e13, 4096)
    k = plan(driver, "knobs", PIPELINE=1, LONG_MIN=100, REGS=0)[0]
    assert (k["pipeline"], k["long_min"], k["regs"], k["regs_forced"]) == (2, 100, 0, 0)
    k = plan(driver, "knobs", PIPELINE="", REGS="")[0]                                    # (empty: the default)
    assert (k["pipeline"], k["regs"], k["host_min_set"], k["long_min"]) == (3, 1, 0, 4096)


def test_edge_keys_asked_only_where_needed(driver):
    assert one(driver, M)["asked_prefix"] == 0
    assert one(driver, M.replace("root=linear", "root=radix"))["asked_prefix"] == 1
    assert one(driver, "root=radix leaf=linear n=1000 L=64")["asked_prefix"] == 0       # (the streaming passes)
    assert one(driver, C3)["asked_increasing"] == 1
    assert one(driver, C3, REGS=0)["asked_increasing"] == 0
    assert one(driver, C3 + " cubic_finite=0")["asked_increasing"] == 0


def test_memory_sigma_hint(driver):
    f1 = "root=linear leaf=linear n=200000000 L=1048576 fit_mode=1"
    r = plan(driver, f1 + " learn=1 flag_count=300000", f1, f1 + " fit_mode=2", f1 + " epoch=2", f1.replace("L=1048576", "L=524288"))
    assert [x["sigma"] for x in r] == [1, 0, 1, 1, 1]
    assert r[1]["pipeline"] == 4
    r = plan(driver, f1 + " learn=1 flag_count=300000 merged_count=100000", f1)             # (merged leaves do not count)
    assert [x["sigma"] for x in r] == [1, 1]
    # eight leaf counts per key set, the oldest forgotten first
    lines = [f1.replace("L=1048576", f"L={1000 + i}") + " learn=1 flag_count=1000000" for i in range(9)]
    r = plan(driver, *lines, f1.replace("L=1048576", "L=1000"), f1.replace("L=1048576", "L=1001"))
    assert (r[-2]["sigma"], r[-1]["sigma"]) == (1, 0)


def test_memory_regs_backoff(driver):
    r = plan(driver, M + " learn=1 regs_listed=5000", M, M + " epoch=2", C4S)
    assert [x["pipeline"] for x in r] == [4, 3, 4, 4]
    r = plan(driver, M + " learn=1 regs_listed=4096", M)                                  # a quarter of the groups: kept
    assert [x["pipeline"] for x in r] == [4, 4]
    assert [x["pipeline"] for x in plan(driver, M + " learn=1 regs_listed=5000", M, REGS_BACKOFF=0)] == [4, 4]


def test_memory_scan_skew(driver):
    r = plan(driver, C5 + " learn=1 scan_listed=300", C5, C5 + " learn=1 scan_listed=513", C5, C5 + " epoch=2")
    assert [(x["listed_hint"], x["long_leaves"]) for x in r] == [(2**32 - 1, 0), (300, 0), (300, 0), (513, 1), (2**32 - 1, 0)]
    r = plan(driver, C5 + " learn=1 scan_listed=5000 stream=1", C5)                         # (streamed chunks teach nothing)
    assert (r[1]["listed_hint"], r[1]["long_leaves"]) == (2**32 - 1, 0)
    r = plan(driver, C5 + " learn=1 scan_listed=5000", C5 + " learn=1 scan_listed=3", C5)   # (the skew is sticky)
    assert (r[2]["listed_hint"], r[2]["long_leaves"]) == (3, 1)
