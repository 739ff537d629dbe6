"""Code-generation guard for the refiner's kernels (no GPU needed: hipcc cross-compiles gfx950), in the pattern of
tests/test_fit_codegen.py: refine_kernels.hip, its ABI unit and the host twin are part of the library, built with the common
flags; no kernel holds a private segment; none needs more than about 2 KB of LDS and the write pass keeps none.  The VGPR and
LDS figures are printed (DESIGN.md 7p records them)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rt-octree_amd", "csrc")
SRC = "refine_kernels.hip"
KERNELS = ("ref_links", "ref_level", "ref_hist", "ref_pick", "ref_count", "ref_tile_scan", "ref_index", "ref_slots", "ref_data16",
           "ref_data2")


def _makefile():
    return open(os.path.join(CSRC, "Makefile")).read()


def _flags():
    mk = _makefile()
    common = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split()
    common = [f for f in common if f.startswith(("-std", "-O", "-f")) and f != "-fPIC"]
    own = re.search(r"^\$\(OBJ\)/refine_kernels\.o: HIPFLAGS \+= (.*)$", mk, re.M)
    return common + (own.group(1).split() if own else [])


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("refine_codegen") / "refine_kernels.s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950"] + _flags() +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, SRC), "-o", out],
                       check=True, capture_output=True, text=True, timeout=900)
    return r.stderr


def test_the_sources_are_part_of_the_library():
    mk = _makefile()
    assert re.search(r"^HIP_SRCS := .*\brefine_kernels\.hip\b", mk, re.M)
    assert re.search(r"^CPP_SRCS := .*\brto_refine_abi\.cpp\b", mk, re.M) and re.search(r"^CPP_SRCS := .*\bhost/tree_refine\.cpp\b", mk, re.M)
    for name in ("refine_kernels.hip", "rto_refine_abi.cpp", "rto_refine_launch.h", "host/tree_refine.h", "host/tree_refine.cpp"):
        assert os.path.exists(os.path.join(CSRC, name)), name
    flags = _flags()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-O3" in flags, flags
    # the links' arithmetic is the simplifier's, included and not restated
    text = open(os.path.join(CSRC, "host", "tree_refine.h")).read()
    assert '#include "host/tree_simplify.h"' in text and "simp_link_target(" not in text


def test_no_refine_kernel_uses_scratch(remarks):
    names = re.findall(r"Function Name: (\S+)", remarks)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", remarks)]
    for row in zip(names, vgprs, scratch, lds):
        print(row)
    assert len(names) == len(scratch) == len(lds) == len(vgprs) == len(KERNELS), names
    for k in KERNELS:
        assert sum(k in n for n in names) == 1, (k, names)
    bad = [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert not bad, "refine kernels with a private segment: %s" % bad
    # a 256-bin histogram or a 256-entry scan buffer of 64-bit counts at the most: occupancy is never bounded by LDS
    assert max(lds) <= 256 * 8 + 64 and min(lds[names.index(n)] for n in names if "ref_hist" in n or "ref_index" in n) >= 1024, lds
    # the write pass keeps nothing in LDS
    assert all(l == 0 for n, l in zip(names, lds) if "ref_slots" in n or "ref_data" in n), lds
