#!/bin/bash
# culling_cells (host/tree_layout.cpp: the culling cells of a tree, as the bounds of their dense leaves and as whole cubes) under
# AddressSanitizer + UndefinedBehaviorSanitizer: seeded random trees held to containment and tightness of the bounds, then the
# same trees with mutated `child` arrays (accepted or refused, never a report, bounds never outside their cell) --
# tools/sanitize/culling_fuzz.cpp, a stand-alone program.  CPU only.
#   tools/sanitize/run_culling.sh [iters] [seed]
set -e
cd "$(dirname "$0")/../.."
IT=${1:-300}
SEED=${2:-1}
T=$(mktemp -d /tmp/rto_culling_san.XXXXXX)
trap 'rm -rf "$T"' EXIT
S=rt-octree_amd/csrc
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$S -Iinclude \
    tools/sanitize/culling_fuzz.cpp $S/host/tree_layout.cpp -o $T/culling_fuzz
UBSAN_OPTIONS=print_stacktrace=1 ASAN_OPTIONS=detect_leaks=1:allocator_may_return_null=0 $T/culling_fuzz $IT $SEED
