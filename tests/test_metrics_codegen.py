"""Code-generation guard for the metric kernels (no GPU needed: hipcc cross-compiles gfx950), like tests/test_codegen.py:
metrics_kernels.hip, built with the Makefile's flags, holds no private segment and no v_pk_fma_f32 (the project's round-3
hazard), and its float64 formula is not contracted into fused multiply-adds by the flags it is built with."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rt-octree_amd", "csrc")
SRC = "metrics_kernels.hip"


def _makefile():
    return open(os.path.join(CSRC, "Makefile")).read()


def _flags():
    mk = _makefile()
    common = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split()
    common = [f for f in common if f.startswith(("-std", "-O", "-f")) and f != "-fPIC"]
    own = re.search(r"^\$\(OBJ\)/metrics_kernels\.o: HIPFLAGS \+= (.*)$", mk, re.M)
    return common + (own.group(1).split() if own else [])


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("metrics_codegen") / "metrics_kernels.s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950"] + _flags() +
                       ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, SRC), "-o", out],
                       check=True, capture_output=True, text=True, timeout=900)
    return open(out).read(), r.stderr


def test_the_source_is_part_of_the_library_and_built_without_contraction():
    mk = _makefile()
    assert re.search(r"^HIP_SRCS := .*\bmetrics_kernels\.hip\b", mk, re.M)
    flags = _flags()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-O3" in flags, flags


def test_no_metric_kernel_uses_scratch(compiled):
    _, remarks = compiled
    names = re.findall(r"Function Name: (\S+)", remarks)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    assert len(names) == len(scratch) == 5, names  # metrics_tiles for the four format pairs + metrics_finish
    assert sum("metrics_tiles" in n for n in names) == 4 and sum("metrics_finish" in n for n in names) == 1
    bad = [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert not bad, "metric kernels with a private segment: %s" % bad


def test_no_metric_kernel_holds_v_pk_fma_f32(compiled):
    text, _ = compiled
    assert text.count("s_endpgm") >= 5
    assert "v_pk_fma_f32" not in text, "%d v_pk_fma_f32" % text.count("v_pk_fma_f32")


def test_the_window_sums_are_multiplies_and_adds(compiled):
    """each of the four tile kernels holds 2 passes x 5 moment planes x 11 taps of v_mul_f64 + v_add_f64 (and the squares and
    the product of the first pass): with contraction on these would be v_fma_f64, of which only the divisions' own remain"""
    text, _ = compiled
    for m in re.finditer(r"^(_ZN3rto\S*metrics_tiles\S*):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M):
        body = m.group(2)
        assert body.count("v_mul_f64") >= 110 and body.count("v_add_f64") >= 110, (m.group(1), body.count("v_mul_f64"), body.count("v_add_f64"))
        assert body.count("v_fma_f64") <= 40, (m.group(1), body.count("v_fma_f64"))  # two divisions per map value + the smape terms'
