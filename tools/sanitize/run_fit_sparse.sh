#!/bin/bash
# The host twins of the sparse step of the tree fit (rto::fit_grad_rays_touched_host, host/fit_grad.cpp; rto::fit_touched_list_host
# and rto::fit_step_sparse_host, host/fit_sparse.cpp over rto_fit_optim.h) under AddressSanitizer + UndefinedBehaviorSanitizer:
# seeded random small trees and rays; the bitmap does not depend on threads or splits and covers every non-zero grad row, the list
# is ascending, cut at its capacity and clears, the SGD step over it leaves the dense step's bytes, RMSProp and Adam change no
# row that is not listed, never a report (tools/sanitize/fit_sparse_fuzz.cpp, a stand-alone program).  CPU only.
#   tools/sanitize/run_fit_sparse.sh [iters] [seed]
set -e
cd "$(dirname "$0")/../.."
IT=${1:-300}
SEED=${2:-1}
T=$(mktemp -d /tmp/rto_fit_sparse_san.XXXXXX)
trap 'rm -rf "$T"' EXIT
S=rt-octree_amd/csrc
g++ -std=c++17 -O1 -g -ffp-contract=off -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$S -Iinclude \
    tools/sanitize/fit_sparse_fuzz.cpp $S/host/fit_grad.cpp $S/host/fit_sparse.cpp $S/host/leaf_weights.cpp -o $T/fit_sparse_fuzz
UBSAN_OPTIONS=print_stacktrace=1 ASAN_OPTIONS=detect_leaks=1:allocator_may_return_null=0 $T/fit_sparse_fuzz $IT $SEED
