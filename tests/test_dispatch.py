"""rto_dispatch.h: the run-time values the launchers of render_kernels.hip and depth_kernels.hip turn into template arguments.
The header is host only, so its tables are checked here by a small program of their own, without a GPU: every supported SPP
and the refusal of any other, the lobe form of each tree format, the three traversal images, the shading kernel's record
modes.  (That every kernel behind them is launched and returns the right bytes is the GPU tests' business.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rt-octree_amd", "csrc")

PROGRAM = r"""
#include <cstdio>

#include "rto_dispatch.h"
using namespace rto;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++bad; } } while (0)

int main() {
    for (int spp = -3; spp <= 70; ++spp) {
        bool in = false;
        for (int s : {SUPPORTED}) in = in || s == spp;
        int got = -1;
        const hipError_t e = with_spp(spp, [&](auto SPP) {
            constexpr int v = SPP;  // (usable as a template argument)
            got = v;
            return hipSuccess;
        });
        CHECK(in ? (e == hipSuccess && got == spp) : (e == hipErrorInvalidValue && got == -1));
    }
    TreeDev t = {};
    const auto lobes = [&] { return with_lobes(t, [](auto LOBES) { constexpr int v = LOBES; return v; }); };
    t.format = kFmtRGBA; CHECK(lobes() == 0);
    t.format = kFmtSH;   CHECK(lobes() == 0);
    t.format = kFmtSG;   CHECK(lobes() == kFmtSG);
    t.format = kFmtASG;  CHECK(lobes() == kFmtASG);

    // 10 * WIDE + STACK, and the (WIDE, STACK) pairs met
    const auto image = [&] { return with_image(t, [](auto wide, auto stack) { constexpr bool w = wide; constexpr int s = stack; return 10 * w + s; }); };
    const uint32_t words[1] = {0};
    t.top_levels = 6;
    // (max_depth -> pairs of levels below the grid: 7 -> 1, 9 and 10 -> 2, 11 -> 3, 13 -> 4, 24 -> 9)
    const int depths[] = {1, 7, 9, 10, 11, 13, 24}, want_wide[] = {11, 11, 11, 11, 10, 10, 10};
    for (int i = 0; i < 7; ++i) {
        t.max_depth = depths[i];
        t.widew = nullptr;
        CHECK(image() == 0 && !register_stack(t));
        t.widew = words;
        CHECK(image() == want_wide[i] && register_stack(t) == (want_wide[i] == 11));
        CHECK(with_wide_image(t, [](auto wide, auto stack) { return 10 * wide + stack; }) == want_wide[i]);
        CHECK(fast_lds_bytes(t) == (size_t)(depths[i] + 1) * 1024);
    }

    const auto mode = [&](bool records) { return with_record_mode(t, records, [](auto MODE) { constexpr int v = MODE; return v; }); };
    const int dims[] = {4, 13, 28, 49, 76, 77}, want_mode[] = {0, 0, 28, 49, 76, 0};
    for (int i = 0; i < 6; ++i) {
        t.data_dim = dims[i];
        CHECK(mode(true) == want_mode[i] && mode(false) == 0);
    }
    if (bad) std::printf("%d checks failed\n", bad);
    else std::printf("dispatch ok\n");
    return bad != 0;
}
"""


@pytest.mark.parametrize("define,supported", [([], "1, 2, 3, 4, 6, 8, 16, 32"), (["-DRTO_DEV_SPP6_ONLY"], "6")])
def test_dispatch_tables(tmp_path, define, supported):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc is needed to compile the host program")
    src = tmp_path / "dispatch_check.cpp"
    src.write_text(PROGRAM.replace("{SUPPORTED}", "{" + supported + "}"))
    exe = tmp_path / "dispatch_check"
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include")] + define + [str(src), "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "dispatch ok" in r.stdout, r.stdout + r.stderr
