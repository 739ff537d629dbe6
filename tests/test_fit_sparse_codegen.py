"""Code-generation guard for the sparse step of the tree fit (no GPU needed: hipcc cross-compiles gfx950), in the pattern of
tests/test_fit_rays_codegen.py: fit_sparse_kernels.hip is part of the library, built with the fit units' flags; its 18 marking
kernels (one per walk and format) hold no private segment, no LDS and no v_pk_fma_f32; the step kernels' arithmetic is not
contracted.  The VGPR counts are printed (DESIGN.md 7r records them)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rt-octree_amd", "csrc")
SRC = "fit_sparse_kernels.hip"
N_MARKING = 3 * 6  # child[], one-level image, two-level image x RGBA, SH1, SH4, SH9, SH16, SH25
N_STEP = 3 * 2  # SGD, RMSProp, Adam x 32-bit and 64-bit element index


def _makefile():
    return open(os.path.join(CSRC, "Makefile")).read()


def _flags(unit):
    mk = _makefile()
    common = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split()
    common = [f for f in common if f.startswith(("-std", "-O", "-f")) and f != "-fPIC"]
    own = re.search(r"^\$\(OBJ\)/%s\.o: HIPFLAGS \+= (.*)$" % re.escape(unit), mk, re.M)
    return common + (own.group(1).split() if own else [])


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("fit_sparse_codegen") / "fit_sparse_kernels.s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950"] + _flags("fit_sparse_kernels") +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, SRC), "-o", out],
                       check=True, capture_output=True, text=True, timeout=900)
    return open(out).read(), r.stderr


def _rows(remarks):
    names = re.findall(r"Function Name: (\S+)", remarks)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", remarks)]
    assert len(names) == len(scratch) == len(lds) == len(vgprs)
    return list(zip(names, vgprs, scratch, lds))


def test_the_source_is_part_of_the_library_with_the_fit_units_flags():
    mk = _makefile()
    assert re.search(r"^HIP_SRCS := .*\bfit_sparse_kernels\.hip\b", mk, re.M)
    assert re.search(r"^CPP_SRCS := .*\bhost/fit_sparse\.cpp\b", mk, re.M)
    flags = _flags("fit_sparse_kernels")
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-O3" in flags and "-fno-slp-vectorize" in flags, flags
    assert sorted(flags) == sorted(_flags("fit_rays_kernels")) == sorted(_flags("fit_kernels"))


def test_eighteen_marking_kernels_without_a_private_segment_or_lds(compiled):
    _, remarks = compiled
    rows = _rows(remarks)
    for row in rows:
        print(row)
    marking = [r for r in rows if "fit_grad_rays_touched_kernel" in r[0]]
    assert len(marking) == N_MARKING, [r[0] for r in rows]
    bad = [r for r in marking if r[2] != 0 or r[3] != 0]
    assert not bad, "marking kernels with a private segment or LDS: %s" % bad
    # the step kernels keep nothing in scratch or LDS either; the list's kernels use LDS for their scans, and no scratch
    step = [r for r in rows if "fit_step_sparse_kernel" in r[0]]
    assert len(step) == N_STEP and not [r for r in step if r[2] != 0 or r[3] != 0], step
    lists = [r for r in rows if "touched_s" in r[0]]
    assert len(lists) == 3 and not [r for r in lists if r[2] != 0], lists
    assert len(rows) == N_MARKING + N_STEP + 3


def _bodies(text, what):
    return re.findall(r"^(_ZN3rto\S*%s\S*):[^\n]*\n(.*?)s_endpgm" % what, text, re.S | re.M)


def test_no_marking_kernel_holds_v_pk_fma_f32(compiled):
    text, _ = compiled
    bodies = _bodies(text, "fit_grad_rays_touched_kernel")
    assert len(bodies) == N_MARKING
    for name, body in bodies:
        assert "v_pk_fma_f32" not in body, name
        # the march is not contracted (tests/test_fit_rays_codegen.py), and the lane marks with an atomic or
        assert body.count("v_mul_f32") >= 20 and body.count("v_add_f32") >= 10, (name, body.count("v_mul_f32"), body.count("v_add_f32"))
        assert "global_atomic_or" in body, name
    assert "v_pk_fma_f32" not in text


def test_the_steps_arithmetic_is_not_contracted(compiled):
    text, _ = compiled
    bodies = _bodies(text, "fit_step_sparse_kernel")
    assert len(bodies) == N_STEP
    for name, body in bodies:
        kind = int(re.search(r"fit_step_sparse_kernelILi(\d)E", name).group(1))
        # (a subtraction may appear as an addition of a negated operand -- the compiler moves the sign into from_fixed's ldexp, which
        # is exact -- so additions and subtractions are counted together)
        mul, add = body.count("v_mul_f32"), len(re.findall(r"v_(add|sub|subrev)_f32", body))
        fma, fmac = body.count("v_fma_f32"), body.count("v_fmac_f32")
        ndiv, nsqrt = body.count("v_div_fixup_f32"), body.count("v_sqrt_f32")
        print(name, "mul %d add/sub %d v_fma_f32 %d v_fmac_f32 %d divisions %d roots %d" % (mul, add, fma, fmac, ndiv, nsqrt))
        assert not re.findall(r"v_(mac|mad)_f32|v_pk_fma_f32", body), name
        # the only fused operations are those of the IEEE sequences: three v_fma_f32 and two v_fmac_f32 per division
        # (v_div_scale .. v_div_fmas, v_div_fixup), two v_fma_f32 per correctly rounded square root
        # (the instantiation with a 64-bit element index also divides 64-bit integers, through float reciprocals of its own)
        wide = "ILi%dEmE" % kind in name
        assert (fma >= 3 * ndiv + 2 * nsqrt and fmac >= 2 * ndiv) if wide else (fma == 3 * ndiv + 2 * nsqrt and fmac == 2 * ndiv), \
            (name, fma, fmac, ndiv, nsqrt)
        if kind == 0:
            # g * grad_scale, lr * g, p - s: two multiplies and a subtraction, and no fused multiply-add at all
            assert mul >= 2 and add >= 1 and ndiv == 0 and nsqrt == 0, (name, mul, add)
        else:
            # the moments: beta * v, (1 - beta) * g, (. * g), their sum; lr * r and p - s
            # RMSProp: 5 multiplies, v's sum, root + eps, p - s; Adam: 2 more multiplies and m's sum
            assert mul >= (7 if kind == 2 else 5) and add >= (4 if kind == 2 else 3), (name, mul, add)
            assert ndiv == (3 if kind == 2 else 1) and nsqrt == 1, name
