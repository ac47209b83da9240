"""A batch driver for the emitted C++ (rmi_amd/codegen.py): reads query keys, writes (guess, err) per query, and marks the
queries on which the emitted lookup has no defined result (the device index counts them as root_oob): a root without a
bounds check whose raw prediction is outside [0, L), a NaN root prediction.  Shared by tests/test_lookup_cpu.py and
tests/test_gpu_lookup.py.  Compiled with strict IEEE flags: -O2 -std=c++17 -ffp-contract=off, no -ffast-math."""
import os
import re
import shutil
import subprocess
import types

import numpy as np

from rmi_amd import codegen

DRIVER_CPP = r'''
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "NS.cpp"
namespace NS {
// the root line of lookup(), then: does the emitted code define the leaf it reads?
static bool root_defined(LKEYT key) {
  double fpred = 0.0; uint64_t ipred = 0; (void)fpred; (void)ipred;
ROOT_LINE
  return CHECK;
}
}
int main(int argc, char** argv) {
  FILE* f = std::fopen(argv[1], "rb");
  uint64_t n = 0;
  if (std::fread(&n, 8, 1, f) != 1) return 3;
  std::vector<KEYT> q(n);
  if (n && std::fread(q.data(), sizeof(KEYT), n, f) != n) return 3;
  std::fclose(f);
  if (!NS::load(argv[2])) { std::printf("load failed\n"); return 2; }
  std::vector<uint64_t> out(3 * n);
  for (uint64_t i = 0; i < n; i++) {
    const LKEYT key = (LKEYT)q[i];
    if (!NS::root_defined(key)) { out[3 * i + 2] = 1; continue; }
    size_t err = 0;
    out[3 * i] = CALL;
    out[3 * i + 1] = err;
  }
  NS::cleanup();
  f = std::fopen(argv[3], "wb");
  std::fwrite(out.data(), 8, out.size(), f);
  std::fclose(f);
  return 0;
}
'''

ROOT_KINDS = {n: i for i, n in enumerate(["linear", "linear_spline", "cubic", "radix", "robust_linear", "loglinear", "normal",
                                          "lognormal", "radix8", "radix18", "radix22", "radix26", "radix28", "bradix"])}


def compiler():
    """g++, or ROCm's clang++ where there is no g++."""
    for c in ("g++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        p = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if p:
            return p
    raise RuntimeError("no C++ compiler (g++ or clang++) found")


def as_rmi(root, leaf_kind, ppl, L, n, params, errors):
    """The attributes codegen.output_rmi reads."""
    return types.SimpleNamespace(branching_factor=L, num_rmi_rows=n, root=root, leaf_kind=leaf_kind, params_per_leaf=ppl,
                                 leaf_params=np.asarray(params, dtype=np.float64).reshape(L, ppl),
                                 last_layer_max_l1s=np.asarray(errors, dtype=np.uint64), build_time=0)


class Driver:
    """Emits `rmi` into `workdir` and compiles the batch driver against it."""

    def __init__(self, rmi, key_dtype, workdir, with_errors=True):
        self.dir = str(workdir)
        self.key_dtype = np.dtype(key_dtype)
        self.with_errors = with_errors
        key_c = "double" if self.key_dtype == np.float64 else "uint64_t"
        paths = codegen.output_rmi("rmi", rmi, os.path.join(self.dir, "rmi_data"), key_type=key_c,
                                   include_errors=with_errors, out_dir=self.dir)
        src = open(paths["rmi.cpp"]).read()
        root_line = re.search(r"^  ([fi]pred = .*;)$", src, re.M).group(1)
        kind = int(rmi.root.kind)
        L = int(rmi.branching_factor)
        if kind in (codegen.RADIX, codegen.BRADIX) or kind in codegen.RADIX_TABLES:
            check = f"ipred < {L}UL"
        elif kind == codegen.CUBIC:
            check = f"fpred > -1.0 && fpred < {L}.0"
        else:
            check = "!std::isnan(fpred)"
        kt = {np.dtype(np.uint64): "uint64_t", np.dtype(np.uint32): "uint32_t", np.dtype(np.float64): "double"}[self.key_dtype]
        call = "NS::lookup(key, &err)" if with_errors else "NS::lookup(key)"
        main = (DRIVER_CPP.replace("ROOT_LINE", "  " + root_line).replace("CHECK", check).replace("CALL", call)
                .replace("LKEYT", key_c).replace("KEYT", kt).replace("NS", "rmi"))
        with open(os.path.join(self.dir, "driver.cpp"), "w") as f:
            f.write(main)
        self.exe = os.path.join(self.dir, "driver")
        subprocess.check_call([compiler(), "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-o", self.exe,
                               os.path.join(self.dir, "driver.cpp")], cwd=self.dir)

    def run(self, queries):
        """-> (guess u64[n], err u64[n], undefined bool[n])"""
        q = np.ascontiguousarray(queries, dtype=self.key_dtype)
        qf, of = os.path.join(self.dir, "q.bin"), os.path.join(self.dir, "out.bin")
        with open(qf, "wb") as f:
            f.write(np.uint64(q.size).tobytes())
            f.write(q.tobytes())
        subprocess.check_call([self.exe, qf, os.path.join(self.dir, "rmi_data"), of])
        out = np.fromfile(of, dtype=np.uint64).reshape(-1, 3)
        return out[:, 0], out[:, 1], out[:, 2].astype(bool)


def query_sets(keys, seed=0, absent=20_000):
    """all keys, random absent keys in range, keys below the minimum / above the maximum, 0 and the dtype's maximum"""
    rng = np.random.default_rng(seed)
    dt = keys.dtype
    lo, hi = keys[0], keys[-1]
    if dt == np.float64:
        inr = rng.uniform(float(lo), float(hi), absent)
        below = float(lo) - rng.uniform(0, max(1.0, abs(float(lo))), 64) if lo > 0 else np.array([], dtype=np.float64)
        above = float(hi) + rng.uniform(0, max(1.0, abs(float(hi))), 64)
        edge = np.array([0.0, np.finfo(np.float64).max])
    else:
        info = np.iinfo(dt)
        inr = rng.integers(int(lo), int(hi), absent, dtype=dt, endpoint=True)
        below = rng.integers(0, int(lo), 64, dtype=dt) if lo > 0 else np.array([], dtype=dt)
        above = rng.integers(int(hi), info.max, 64, dtype=dt, endpoint=True) if hi < info.max else np.array([], dtype=dt)
        edge = np.array([0, info.max], dtype=dt)
    inr = inr[~np.isin(inr, keys)]
    return {"keys": keys.copy(), "absent": inr.astype(dt), "outside": np.concatenate([below, above, edge]).astype(dt)}
