#!/bin/bash
# The host code behind the C ABI (csrc/*.cpp, csrc/host/*.cpp, rto_abi_common.h) under AddressSanitizer + UBSan, driven by a
# program of its own (abi_refusals.cpp) through the refusals that are decided on the host.  CPU only: nothing is launched.
# The device code is the library's own objects, uninstrumented: build librto.so first (make -C rt-octree_amd/csrc).
set -e
cd "$(dirname "$0")/../.."
S=rt-octree_amd/csrc
O=rt-octree_amd/lib/obj
T=$(mktemp -d /tmp/rto_san_abi.XXXXXX)
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
for f in rto_abi rto_tree rto_render_abi rto_guidance_abi rto_metrics_abi rto_guidance_train_abi rto_mesh host/png_read host/mesh_build \
         host/mesh_io host/tree_layout host/npz host/n3tree_host cli/imwrite; do
    hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -fPIC -ffp-contract=off -fno-fast-math $SAN -Iinclude -I$S -c $S/$f.cpp \
        -o $T/$(basename $f).o &
done
wait
hipcc --offload-arch=gfx950 -std=c++17 -O1 -g $SAN -Iinclude -c -x c++ tools/sanitize/abi_refusals.cpp -o $T/main.o
hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o $T/abi_refusals $T/*.o $O/*_kernels.o -lz
UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 ASAN_OPTIONS=detect_leaks=0 $T/abi_refusals
rm -rf "$T"
