"""Code-generation guard for the leaf-weight kernels (no GPU needed: hipcc cross-compiles gfx950), in the pattern of
tests/test_metrics_codegen.py: leaf_weight_kernels.hip is part of the library, built without contraction and without the SLP
vectoriser like the other traversal units; its three kernels (one per walk) hold no private segment, no LDS and no
v_pk_fma_f32 (the project's round-3 hazard); the update is a vector atomic max on global memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rt-octree_amd", "csrc")
SRC = "leaf_weight_kernels.hip"


def _makefile():
    return open(os.path.join(CSRC, "Makefile")).read()


def _flags():
    mk = _makefile()
    common = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split()
    common = [f for f in common if f.startswith(("-std", "-O", "-f")) and f != "-fPIC"]
    own = re.search(r"^\$\(OBJ\)/leaf_weight_kernels\.o: HIPFLAGS \+= (.*)$", mk, re.M)
    return common + (own.group(1).split() if own else [])


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("leaf_weights_codegen") / "leaf_weight_kernels.s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950"] + _flags() +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, SRC), "-o", out],
                       check=True, capture_output=True, text=True, timeout=900)
    return open(out).read(), r.stderr


def test_the_source_is_part_of_the_library_with_the_traversal_units_flags():
    mk = _makefile()
    assert re.search(r"^HIP_SRCS := .*\bleaf_weight_kernels\.hip\b", mk, re.M)
    assert re.search(r"^CPP_SRCS := .*\brto_leaf_weights_abi\.cpp\b.*\bhost/leaf_weights\.cpp\b", mk, re.M)
    flags = _flags()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-O3" in flags and "-fno-slp-vectorize" in flags, flags


def test_no_leaf_weight_kernel_uses_scratch_or_lds(compiled):
    _, remarks = compiled
    names = re.findall(r"Function Name: (\S+)", remarks)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", remarks)]
    print(list(zip(names, vgprs, scratch, lds)))
    assert len(names) == len(scratch) == len(lds) == 3, names  # one kernel per walk: child[], one-level image, two-level image
    assert all("leaf_weights_kernel" in n for n in names), names
    bad = [(n, s, l) for n, s, l in zip(names, scratch, lds) if s != 0 or l != 0]
    assert not bad, "leaf-weight kernels with a private segment or LDS: %s" % bad


def test_no_leaf_weight_kernel_holds_v_pk_fma_f32(compiled):
    text, _ = compiled
    assert text.count("s_endpgm") >= 3
    assert "v_pk_fma_f32" not in text, "%d v_pk_fma_f32" % text.count("v_pk_fma_f32")


def test_the_update_is_a_vector_atomic_max_and_the_march_is_not_contracted(compiled):
    text, _ = compiled
    bodies = re.findall(r"^(_ZN3rto\S*leaf_weights_kernel\S*):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M)
    assert len(bodies) == 3
    for name, body in bodies:
        assert re.search(r"\b(global|flat)_atomic_u?max\b", body), name
        # pos = cen + t * dir, w = T * (1 - att), t + dt: float multiplies and adds; the only v_fma_f32 left are those of the
        # IEEE division and square-root sequences (v_div_fmas_f32 / v_div_fixup_f32 close each of them)
        assert body.count("v_mul_f32") >= 12 and body.count("v_add_f32") >= 6, (name, body.count("v_mul_f32"), body.count("v_add_f32"))
