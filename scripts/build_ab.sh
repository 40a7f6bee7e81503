#!/bin/bash
# A copy of the library for same-box A/B comparisons: scripts/build_ab.sh NAME [hipcc argument ...]  ->  scripts/ab/NAME.so
# It builds the tree as it stands with the product's flags (geobipy_amd/build.py), so `scripts/build_ab.sh parent` before a change
# keeps the parent's library for scripts/ab_bits.py and scripts/ab_rj.py (GBP_AB_LIB).  Measurement only: the product loads
# geobipy_amd/csrc/libgeobipy_amd.so.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p scripts/ab
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -pthread \
    "$@" geobipy_amd/csrc/gbp_fdem.hip -o scripts/ab/$name.so
echo built scripts/ab/$name.so
