#!/bin/bash
# The host twin of the tree refiner (host/tree_refine.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: seeded random
# trees (shuffled, padded with garbage nodes, N = 2 and 3, D = 1 .. 28) with random keys, thresholds, budgets and level bounds,
# held to the invariants of the definition -- the counts, the order of the selection, slot_src, the field along random slot
# paths -- the same trees with mutated `child` arrays (RTO_OK or RTO_E_FORMAT, never a report), the depth limit and the argument
# refusals (tools/sanitize/refine_fuzz.cpp, a stand-alone program).  CPU only.
#   tools/sanitize/run_refine.sh [iters] [seed]
set -e
cd "$(dirname "$0")/../.."
IT=${1:-300}
SEED=${2:-1}
T=$(mktemp -d /tmp/rto_refine_san.XXXXXX)
trap 'rm -rf "$T"' EXIT
S=rt-octree_amd/csrc
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$S -Iinclude \
    tools/sanitize/refine_fuzz.cpp $S/host/tree_refine.cpp -o $T/refine_fuzz
UBSAN_OPTIONS=print_stacktrace=1 ASAN_OPTIONS=detect_leaks=1:allocator_may_return_null=0 $T/refine_fuzz $IT $SEED
