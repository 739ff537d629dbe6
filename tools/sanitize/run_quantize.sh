#!/bin/bash
# The host twin of the median-cut quantiser (host/median_cut.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: seeded
# random, tie-heavy and constant-column inputs held to the invariants of the definition -- every id below 2^bits, sibling boxes
# differing by at most one row, the palette the exact mean, a one-row box's palette its row -- and the refusals
# (tools/sanitize/quantize_fuzz.cpp, a stand-alone program).  CPU only.
#   tools/sanitize/run_quantize.sh [iters] [seed]
set -e
cd "$(dirname "$0")/../.."
IT=${1:-300}
SEED=${2:-1}
T=$(mktemp -d /tmp/rto_quant_san.XXXXXX)
trap 'rm -rf "$T"' EXIT
S=rt-octree_amd/csrc
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$S \
    tools/sanitize/quantize_fuzz.cpp $S/host/median_cut.cpp -o $T/quantize_fuzz
UBSAN_OPTIONS=print_stacktrace=1 ASAN_OPTIONS=detect_leaks=1:allocator_may_return_null=0 $T/quantize_fuzz $IT $SEED
