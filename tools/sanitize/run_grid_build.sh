#!/bin/bash
# The host twin of the grid builder (host/grid_build.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: seeded random
# grids (L = 1 .. 4, D = 1 .. 49, uniform regions of every size) held to the invariants of the definition -- the field at every
# voxel, breadth-first links, no uniform node left, the counts -- in outputs of exactly the reported size, the edge cases (zero
# grids, chains, NaN records), `room` too small and the argument refusals (tools/sanitize/grid_build_fuzz.cpp, a stand-alone
# program).  CPU only, nothing preloaded.
#   tools/sanitize/run_grid_build.sh [iters] [seed]
set -e
cd "$(dirname "$0")/../.."
IT=${1:-300}
SEED=${2:-1}
T=$(mktemp -d /tmp/rto_grid_build_san.XXXXXX)
trap 'rm -rf "$T"' EXIT
S=rt-octree_amd/csrc
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$S -Iinclude \
    tools/sanitize/grid_build_fuzz.cpp $S/host/grid_build.cpp -o $T/grid_build_fuzz
UBSAN_OPTIONS=print_stacktrace=1 ASAN_OPTIONS=detect_leaks=1:allocator_may_return_null=0 $T/grid_build_fuzz $IT $SEED
