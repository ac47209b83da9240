#!/bin/bash
# usage: tools/build_var.sh NAME [-DMACRO=..]...  -> build_ab/var/NAME.so (an experiment build of the same ABI; RMI_HIP_LIB=... selects it)
# rmi_hip.hip is compiled with the macros; the units of pipeline 5 and of the device index are taken from the in-tree build
# (rmi_amd/build/rmi_scan.o, rmi_lookup.o).
# LOOKUP_SRC=path tools/build_var.sh NAME [-DMACRO=..]...: the device index is the unit that is compiled instead -- from `path`, with
# the macros (rmi_amd/csrc/rmi_lookup.hip itself, or a changed copy of it anywhere: the mutants of CHANGELOG.md's table are built so) --
# and rmi_hip.o and rmi_scan.o are the in-tree ones.
NAME=$1; shift
mkdir -p build_ab/var
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function"
if [ -n "$LOOKUP_SRC" ]; then
  SRC=$LOOKUP_SRC; REST="rmi_amd/build/rmi_hip.o rmi_amd/build/rmi_scan.o"
else
  SRC=rmi_amd/csrc/rmi_hip.hip; REST="rmi_amd/build/rmi_scan.o rmi_amd/build/rmi_lookup.o"
fi
/opt/rocm/bin/hipcc $FLAGS -Irmi_amd/csrc "$@" -c "$SRC" -o build_ab/var/$NAME.o 2> build_ab/var/$NAME.log || { tail -5 build_ab/var/$NAME.log; exit 1; }
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build_ab/var/$NAME.so build_ab/var/$NAME.o $REST -ldl && rm -f build_ab/var/$NAME.o
