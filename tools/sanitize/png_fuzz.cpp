// png_fuzz.cpp -- the PNG reader (host/png_read.cpp) under AddressSanitizer + UBSan, CPU only.  Build + run:
// tools/sanitize/run_png.sh.  A stand-alone program:
//   1. images of several sizes go through the project's writer (cli/imwrite.cpp) and back through the reader, byte for byte;
//   2. the same images, encoded here with every row filter and real deflate (RGB and RGBA, one and several IDAT chunks), must
//      decode to the same bytes;
//   3. `iters` mutations of those files -- byte flips, truncations, edits of a chunk's length field, half of them with every
//      chunk's CRC made right again so that the mutation reaches the code behind the CRC check -- must each either load or be
//      refused with std::runtime_error.  Anything else (a sanitizer report, a signal, another exception type) fails the run;
//   4. the RANK_METRICS line of `volrend_headless --gpus N` (cli/rank_metrics.h) is formatted, parsed and merged on hand-made
//      lines.
// usage: png_fuzz <scratch dir> <iters> [<png to write with the project's writer>]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include <zlib.h>

#include "../../rt-octree_amd/csrc/cli/imwrite.h"
#include "../../rt-octree_amd/csrc/cli/rank_metrics.h"
#include "../../rt-octree_amd/csrc/host/png_read.h"

namespace {

[[noreturn]] void die(const std::string& why) {
    std::fprintf(stderr, "png_fuzz: FAILED: %s\n", why.c_str());
    std::exit(1);
}

std::vector<uint8_t> slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    if (!f) die("cannot read " + p);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// the pattern tests/test_png_reader.py expects in the file the project's writer leaves behind
std::vector<uint8_t> pattern(int w, int h) {
    std::vector<uint8_t> px((size_t)w * h * 4);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < 4; ++c) px[((size_t)y * w + x) * 4 + c] = (uint8_t)((x * 7 + y * 13 + c * 29 + x * y) & 0xff);
    return px;
}

void put32(std::vector<uint8_t>& b, uint32_t v) {
    for (int s = 24; s >= 0; s -= 8) b.push_back((uint8_t)(v >> s));
}

void put_chunk(std::vector<uint8_t>& b, const char* type, const uint8_t* data, size_t n) {
    put32(b, (uint32_t)n);
    const size_t at = b.size();
    b.insert(b.end(), type, type + 4);
    b.insert(b.end(), data, data + n);
    put32(b, (uint32_t)crc32(crc32(0L, Z_NULL, 0), b.data() + at, (uInt)(4 + n)));
}

int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// an encoder of its own: filter type row % 5 on every row, deflate at `level`, the stream cut into `idats` chunks
std::vector<uint8_t> encode(const std::vector<uint8_t>& rgba, int w, int h, int channels, int level, int idats) {
    const size_t stride = (size_t)w * channels;
    std::vector<uint8_t> lines((size_t)h * stride), raw;
    for (size_t i = 0; i < (size_t)w * h; ++i)
        for (int c = 0; c < channels; ++c) lines[i * channels + c] = rgba[i * 4 + c];
    for (int y = 0; y < h; ++y) {
        const int ft = y % 5;
        raw.push_back((uint8_t)ft);
        for (size_t i = 0; i < stride; ++i) {
            const int a = i >= (size_t)channels ? lines[y * stride + i - channels] : 0;
            const int b = y > 0 ? lines[(y - 1) * stride + i] : 0;
            const int c = (y > 0 && i >= (size_t)channels) ? lines[(y - 1) * stride + i - channels] : 0;
            const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) / 2 : paeth(a, b, c);
            raw.push_back((uint8_t)((lines[y * stride + i] - pred) & 0xff));
        }
    }
    uLongf zn = compressBound((uLong)raw.size());
    std::vector<uint8_t> z(zn);
    if (compress2(z.data(), &zn, raw.data(), (uLong)raw.size(), level) != Z_OK) die("compress2");
    z.resize(zn);
    std::vector<uint8_t> f = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    std::vector<uint8_t> ihdr;
    put32(ihdr, (uint32_t)w);
    put32(ihdr, (uint32_t)h);
    const uint8_t rest[5] = {8, (uint8_t)(channels == 3 ? 2 : 6), 0, 0, 0};
    ihdr.insert(ihdr.end(), rest, rest + 5);
    put_chunk(f, "IHDR", ihdr.data(), ihdr.size());
    const size_t piece = (z.size() + idats - 1) / idats;
    for (size_t at = 0; at < z.size(); at += piece) put_chunk(f, "IDAT", z.data() + at, std::min(piece, z.size() - at));
    put_chunk(f, "IEND", nullptr, 0);
    return f;
}

// every chunk's CRC made right, walking the chunks as far as their lengths stay inside the file
void fix_crcs(std::vector<uint8_t>& b) {
    size_t pos = 8;
    while (pos + 12 <= b.size()) {
        const uint64_t len = ((uint64_t)b[pos] << 24) | ((uint64_t)b[pos + 1] << 16) | ((uint64_t)b[pos + 2] << 8) | b[pos + 3];
        if (len > b.size() - pos - 12) return;
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), b.data() + pos + 4, (uInt)(4 + len));
        for (int k = 0; k < 4; ++k) b[pos + 8 + len + k] = (uint8_t)(crc >> (24 - 8 * k));
        pos += 12 + (size_t)len;
    }
}

std::vector<uint8_t> mutate(const std::vector<uint8_t>& src, std::mt19937_64& rng) {
    std::vector<uint8_t> b = src;
    auto pick = [&](size_t lo, size_t hi) { return lo + (size_t)(rng() % (hi - lo + 1)); };
    switch (rng() % 5) {
        case 0:  // truncate anywhere
            b.resize(pick(0, b.size()));
            break;
        case 1:  // flip bits in the signature / IHDR
            for (int k = 0; k < 1 + (int)(rng() % 3); ++k) b[pick(0, std::min<size_t>(b.size(), 33) - 1)] ^= (uint8_t)(1u << (rng() % 8));
            break;
        case 2:  // flip bits anywhere
            for (int k = 0; k < 1 + (int)(rng() % 4); ++k) b[pick(0, b.size() - 1)] ^= (uint8_t)(1u << (rng() % 8));
            break;
        case 3: {  // edit the length field of one of the chunks
            std::vector<size_t> at;
            for (size_t pos = 8; pos + 12 <= b.size();) {
                at.push_back(pos);
                const uint64_t len = ((uint64_t)b[pos] << 24) | ((uint64_t)b[pos + 1] << 16) | ((uint64_t)b[pos + 2] << 8) | b[pos + 3];
                if (len > b.size() - pos - 12) break;
                pos += 12 + (size_t)len;
            }
            const size_t pos = at[rng() % at.size()];
            const uint32_t values[6] = {0u, 1u, 0x7fffffffu, 0xffffffffu, (uint32_t)rng(), (uint32_t)(b[pos + 3] + 1 - 2 * (int)(rng() % 2))};
            const uint32_t v = values[rng() % 6];
            for (int k = 0; k < 4; ++k) b[pos + k] = (uint8_t)(v >> (24 - 8 * k));
        } break;
        default: {  // overwrite a short range with one byte value
            const size_t a = pick(0, b.size() - 1), n = std::min<size_t>(b.size() - a, pick(1, 16));
            std::memset(b.data() + a, (int)(rng() & 0xff), n);
        } break;
    }
    if (rng() % 2) fix_crcs(b);
    return b;
}

void check_rank_metrics() {
    rto::MetricSums a, b, got;
    a.add(30.5, 0.5, 0.125);
    a.add(31.25, 0.75, 0.25);
    b.add(29.0, 0.875, 0.0625);
    const std::string la = rto::format_rank_metrics(a), lb = rto::format_rank_metrics(b);
    if (la != "RANK_METRICS 61.75 1.25 0.375 2") die("format_rank_metrics: " + la);
    rto::MetricSums total;
    for (const std::string& l : {la, lb}) {
        if (!rto::parse_rank_metrics(l, &got)) die("parse_rank_metrics refused its own line " + l);
        total.merge(got);
    }
    if (total.frames != 3 || total.psnr != 90.75 || total.ssim != 2.125 || total.smape != 0.4375) die("RANK_METRICS merge");
    if (rto::format_metric_means(total).rfind("psnr:   30.2500000000\nssim:   0.7083333333\nsmape:  0.1458333333\n", 0) != 0)
        die("format_metric_means: " + rto::format_metric_means(total));
    // the per-pose rows the parent turns into the one metrics.json of the run
    rto::FrameRow row, back;
    row.pose = 7, row.name = "r_7", row.mse = 0.001, row.psnr = 30.0, row.smape = 0.0625, row.ssim = 0.1 + 0.2;
    if (!rto::parse_frame_metrics(rto::format_frame_metrics(row), &back) || back.pose != 7 || back.name != "r_7" || back.mse != row.mse ||
        back.psnr != row.psnr || back.smape != row.smape || back.ssim != row.ssim)
        die("RANK_FRAME_METRICS round trip: " + rto::format_frame_metrics(row));
    if (!rto::parse_frame_metrics("RANK_FRAME_METRICS 0 0 inf 0 nan img 000", &back) || back.name != "img 000" || !std::isinf(back.psnr) || !std::isnan(back.ssim))
        die("RANK_FRAME_METRICS with non-finite values");
    for (const char* l : {"RANK_FRAME_METRICS 1 2 3 4 5", "RANK_FRAME_METRICS -1 2 3 4 5 x", "RANK_METRICS 1 2 3 4", "RANK_FRAME_METRICS 1 2 3 x"})
        if (rto::parse_frame_metrics(l, &back)) die(std::string("parse_frame_metrics took '") + l + "'");
    if (rto::json_double(0.1 + 0.2) != "0.30000000000000004" || rto::json_double(-INFINITY) != "-Infinity" || rto::json_double(NAN) != "NaN") die("json_double");
    // hand-made lines: an infinite PSNR sum (identical frames) parses; other lines and damaged ones do not
    if (!rto::parse_rank_metrics("RANK_METRICS inf 3 0 3", &got) || !std::isinf(got.psnr) || got.frames != 3) die("parse of an infinite sum");
    for (const char* l : {"RANK_REPORT 1 2 3 4", "RANK_METRICS 1 2 3", "RANK_METRICS 1 2 3 -1", "RANK_METRICS 1 2 3 4 5", "", "render: 1 ms per frame"})
        if (rto::parse_rank_metrics(l, &got)) die(std::string("parse_rank_metrics took '") + l + "'");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fputs("usage: png_fuzz <scratch dir> <iters> [<png to write>]\n", stderr);
        return 2;
    }
    const std::string dir = argv[1];
    const int iters = std::atoi(argv[2]);
    std::mt19937_64 rng(20230418);
    const int sizes[5][2] = {{1, 1}, {3, 5}, {64, 48}, {37, 100}, {11, 2}};
    std::vector<std::vector<uint8_t>> corpus;
    int round_trips = 0;
    for (const auto& s : sizes) {
        const int w = s[0], h = s[1];
        std::vector<uint8_t> px((size_t)w * h * 4);
        for (auto& v : px) v = (uint8_t)rng();
        const std::string path = dir + "/rt_" + std::to_string(w) + "x" + std::to_string(h) + ".png";
        if (!rto::write_png_rgba8(path, px.data(), w, h)) die("write_png_rgba8 " + path);
        const rto::PngImage back = rto::png_read(path);
        if (back.width != w || back.height != h || back.rgba != px) die("round trip through the project's writer: " + path);
        int rw = 0, rh = 0;
        rto::png_read_size(path, &rw, &rh);
        if (rw != w || rh != h) die("png_read_size " + path);
        corpus.push_back(slurp(path));
        ++round_trips;
        for (int channels = 3; channels <= 4; ++channels)
            for (int idats = 1; idats <= 3; idats += 2) {
                const std::vector<uint8_t> f = encode(px, w, h, channels, channels == 3 ? 9 : 1, idats);
                const rto::PngImage img = rto::png_decode(f.data(), f.size(), "encoded");
                bool same = img.width == w && img.height == h;
                for (size_t i = 0; same && i < (size_t)w * h; ++i)
                    for (int c = 0; c < 4; ++c) same = same && img.rgba[4 * i + c] == (c < channels ? px[4 * i + c] : 255);
                if (!same) die("decode of the filtered " + std::to_string(w) + "x" + std::to_string(h) + " image");
                corpus.push_back(f);
                ++round_trips;
            }
    }
    try {
        (void)rto::png_read(dir + "/does_not_exist.png");
        die("a missing file loaded");
    } catch (const std::runtime_error&) {
    }
    int loaded = 0, refused = 0;
    for (int i = 0; i < iters; ++i) {
        const std::vector<uint8_t> m = mutate(corpus[rng() % corpus.size()], rng);
        try {
            const rto::PngImage img = rto::png_decode(m.data(), m.size(), "mutation " + std::to_string(i));
            if (img.rgba.size() != (size_t)img.width * img.height * 4) die("a loaded mutation has the wrong size");
            ++loaded;
        } catch (const std::runtime_error&) {
            ++refused;
        } catch (...) {
            die("mutation " + std::to_string(i) + " threw something that is no std::runtime_error");
        }
    }
    check_rank_metrics();
    if (argc > 3) {
        const std::vector<uint8_t> px = pattern(64, 48);
        if (!rto::write_png_rgba8(argv[3], px.data(), 64, 48)) die(std::string("write_png_rgba8 ") + argv[3]);
    }
    std::printf("png_fuzz: clean: %d round trips, %d mutations (%d loaded, %d refused), RANK_METRICS merge ok\n", round_trips, iters, loaded, refused);
    return 0;
}
