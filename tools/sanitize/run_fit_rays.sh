#!/bin/bash
# The host twin of the tree fit on rays the caller supplies (rto::fit_grad_rays_host, host/fit_grad.cpp over rto_fit_march.h)
# under AddressSanitizer + UndefinedBehaviorSanitizer: seeded random small trees and rays, degenerate and masked ones included;
# every call terminates, the thread count, the order of the rays and a split over calls change no bit, internal slots receive
# no gradient, never a report (tools/sanitize/fit_rays_fuzz.cpp, a stand-alone program).  CPU only.
#   tools/sanitize/run_fit_rays.sh [iters] [seed]
set -e
cd "$(dirname "$0")/../.."
IT=${1:-300}
SEED=${2:-1}
T=$(mktemp -d /tmp/rto_fit_rays_san.XXXXXX)
trap 'rm -rf "$T"' EXIT
S=rt-octree_amd/csrc
g++ -std=c++17 -O1 -g -ffp-contract=off -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$S -Iinclude \
    tools/sanitize/fit_rays_fuzz.cpp $S/host/fit_grad.cpp $S/host/leaf_weights.cpp -o $T/fit_rays_fuzz
UBSAN_OPTIONS=print_stacktrace=1 ASAN_OPTIONS=detect_leaks=1:allocator_may_return_null=0 $T/fit_rays_fuzz $IT $SEED
