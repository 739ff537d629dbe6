"""Code-generation guard for the ray kernels of the tree fit (no GPU needed: hipcc cross-compiles gfx950), in the pattern of
tests/test_fit_codegen.py: fit_rays_kernels.hip is part of the library, built without contraction and without the SLP vectoriser
like the other traversal units; its 18 kernels (one per walk and format) hold no private segment, no LDS and no v_pk_fma_f32,
and the march is not contracted.  The VGPR counts are printed (DESIGN.md 7q records them)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rt-octree_amd", "csrc")
SRC = "fit_rays_kernels.hip"
N_KERNELS = 3 * 6  # child[], one-level image, two-level image x RGBA, SH1, SH4, SH9, SH16, SH25


def _makefile():
    return open(os.path.join(CSRC, "Makefile")).read()


def _flags():
    mk = _makefile()
    common = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split()
    common = [f for f in common if f.startswith(("-std", "-O", "-f")) and f != "-fPIC"]
    own = re.search(r"^\$\(OBJ\)/fit_rays_kernels\.o: HIPFLAGS \+= (.*)$", mk, re.M)
    return common + (own.group(1).split() if own else [])


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("fit_rays_codegen") / "fit_rays_kernels.s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950"] + _flags() +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, SRC), "-o", out],
                       check=True, capture_output=True, text=True, timeout=900)
    return open(out).read(), r.stderr


def test_the_source_is_part_of_the_library_with_the_traversal_units_flags():
    mk = _makefile()
    assert re.search(r"^HIP_SRCS := .*\bfit_rays_kernels\.hip\b", mk, re.M)
    flags = _flags()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-O3" in flags and "-fno-slp-vectorize" in flags, flags


def test_eighteen_kernels_without_a_private_segment_or_lds(compiled):
    _, remarks = compiled
    names = re.findall(r"Function Name: (\S+)", remarks)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", remarks)]
    for row in zip(names, vgprs, scratch, lds):
        print(row)
    assert len(names) == len(scratch) == len(lds) == N_KERNELS, names
    assert all("fit_grad_rays_kernel" in n for n in names), names
    bad = [(n, s, l) for n, s, l in zip(names, scratch, lds) if s != 0 or l != 0]
    assert not bad, "ray kernels with a private segment or LDS: %s" % bad


def test_no_kernel_holds_v_pk_fma_f32(compiled):
    text, _ = compiled
    assert text.count("s_endpgm") >= N_KERNELS
    assert "v_pk_fma_f32" not in text, "%d v_pk_fma_f32" % text.count("v_pk_fma_f32")


def test_the_march_is_not_contracted(compiled):
    text, _ = compiled
    bodies = re.findall(r"^(_ZN3rto\S*fit_grad_rays_kernel\S*):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M)
    assert len(bodies) == N_KERNELS
    for name, body in bodies:
        # pos = cen + t * dir, w = T * (1 - att), acc + w * c, t + dt: float multiplies and adds; the only v_fma_f32 left are
        # those of the IEEE division and square-root sequences
        assert body.count("v_mul_f32") >= 20 and body.count("v_add_f32") >= 10, (name, body.count("v_mul_f32"), body.count("v_add_f32"))
