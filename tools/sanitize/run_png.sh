#!/bin/bash
# The PNG reader (host/png_read.cpp) with the project's PNG writer under AddressSanitizer + UndefinedBehaviorSanitizer: round
# trips, then mutated files, each of which must load or be refused with std::runtime_error (tools/sanitize/png_fuzz.cpp, a
# stand-alone program; it also checks the RANK_METRICS line of cli/rank_metrics.h).  CPU only.
#   tools/sanitize/run_png.sh [iters] [png]     png: a 64 x 48 image the project's writer leaves there (tests/test_png_reader.py)
set -e
cd "$(dirname "$0")/../.."
IT=${1:-3000}
T=$(mktemp -d /tmp/rto_png_san.XXXXXX)
trap 'rm -rf "$T"' EXIT
S=rt-octree_amd/csrc
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Iinclude -I$S \
    tools/sanitize/png_fuzz.cpp $S/host/png_read.cpp $S/cli/imwrite.cpp -lz -o $T/png_fuzz
UBSAN_OPTIONS=print_stacktrace=1 ASAN_OPTIONS=detect_leaks=1:allocator_may_return_null=0:max_allocation_size_mb=4096 $T/png_fuzz $T $IT $2
