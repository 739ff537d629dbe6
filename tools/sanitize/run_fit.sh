#!/bin/bash
# The host twin of the tree fit (host/fit_grad.cpp over rto_fit_march.h) under AddressSanitizer + UndefinedBehaviorSanitizer:
# seeded random small trees, cameras and targets, masked and degenerate ones included; every call terminates, the thread count
# changes no bit, internal slots receive no gradient, mutated child arrays are marched or refused, never a report
# (tools/sanitize/fit_fuzz.cpp, a stand-alone program).  CPU only.
#   tools/sanitize/run_fit.sh [iters] [seed]
set -e
cd "$(dirname "$0")/../.."
IT=${1:-300}
SEED=${2:-1}
T=$(mktemp -d /tmp/rto_fit_san.XXXXXX)
trap 'rm -rf "$T"' EXIT
S=rt-octree_amd/csrc
g++ -std=c++17 -O1 -g -ffp-contract=off -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$S -Iinclude \
    tools/sanitize/fit_fuzz.cpp $S/host/fit_grad.cpp $S/host/leaf_weights.cpp -o $T/fit_fuzz
UBSAN_OPTIONS=print_stacktrace=1 ASAN_OPTIONS=detect_leaks=1:allocator_may_return_null=0 $T/fit_fuzz $IT $SEED
