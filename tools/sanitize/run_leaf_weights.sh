#!/bin/bash
# The host twin of the per-leaf peak weights (host/leaf_weights.cpp over rto_leaf_march.h) under AddressSanitizer +
# UndefinedBehaviorSanitizer: seeded random small trees and cameras, degenerate ones included; every call terminates, every weight
# lies in [0, 1], the thread count changes nothing, mutated child arrays are marched or refused, never a report
# (tools/sanitize/leaf_weights_fuzz.cpp, a stand-alone program).  CPU only.
#   tools/sanitize/run_leaf_weights.sh [iters] [seed]
set -e
cd "$(dirname "$0")/../.."
IT=${1:-300}
SEED=${2:-1}
T=$(mktemp -d /tmp/rto_leaf_weights_san.XXXXXX)
trap 'rm -rf "$T"' EXIT
S=rt-octree_amd/csrc
g++ -std=c++17 -O1 -g -ffp-contract=off -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$S -Iinclude \
    tools/sanitize/leaf_weights_fuzz.cpp $S/host/leaf_weights.cpp -o $T/leaf_weights_fuzz
UBSAN_OPTIONS=print_stacktrace=1 ASAN_OPTIONS=detect_leaks=1:allocator_may_return_null=0 $T/leaf_weights_fuzz $IT $SEED
