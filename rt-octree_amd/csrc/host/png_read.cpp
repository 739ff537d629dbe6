// png_read.cpp -- see png_read.h.  A parser of untrusted files: every length is checked against what is left of the file
// before it is used, every size is computed in 64 bits, and tools/sanitize/run_png.sh runs it over mutated files under
// AddressSanitizer and UBSan.
#include "png_read.h"

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace rto {
namespace {

constexpr uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
constexpr uint64_t kMaxPixels = uint64_t(1) << 28;  // 1 GiB of RGBA8: far beyond any frame, far below what overflows an int

[[noreturn]] void refuse(const std::string& name, const std::string& why) { throw std::runtime_error("PNG " + name + ": " + why); }

uint32_t be32(const uint8_t* p) { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | uint32_t(p[3]); }

struct Header {
    int width = 0, height = 0, channels = 0;
};

struct Chunk {
    const uint8_t* type = nullptr;
    const uint8_t* data = nullptr;
    uint32_t len = 0;
};

// the chunk at `pos` (length, type, data, CRC all inside the file, CRC verified); advances pos past it
Chunk next_chunk(const uint8_t* bytes, size_t n, size_t* pos, const std::string& name) {
    if (n - *pos < 12) refuse(name, "truncated: no room for a chunk at byte " + std::to_string(*pos));
    Chunk c;
    c.len = be32(bytes + *pos);
    if ((uint64_t)c.len > (uint64_t)(n - *pos) - 12)
        refuse(name, "truncated: a chunk of " + std::to_string(c.len) + " bytes at byte " + std::to_string(*pos) + " runs past the end of the file");
    c.type = bytes + *pos + 4;
    c.data = c.type + 4;
    uLong crc = crc32(0L, Z_NULL, 0);
    crc = crc32(crc, c.type, 4);
    uint32_t left = c.len;  // (crc32 takes a uInt; a chunk is < 4 GiB, fed in one or two pieces whatever uInt is)
    const uint8_t* p = c.data;
    while (left > 0) {
        const uInt step = left > (1u << 30) ? (1u << 30) : (uInt)left;
        crc = crc32(crc, p, step);
        p += step;
        left -= step;
    }
    if ((uint32_t)crc != be32(c.data + c.len)) refuse(name, "bad CRC in the chunk at byte " + std::to_string(*pos));
    *pos += 12 + (size_t)c.len;
    return c;
}

bool is_type(const Chunk& c, const char* t) { return std::memcmp(c.type, t, 4) == 0; }

Header read_header(const uint8_t* bytes, size_t n, size_t* pos, const std::string& name) {
    if (n < 8 || std::memcmp(bytes, kSignature, 8) != 0) refuse(name, "not a PNG file (signature)");
    *pos = 8;
    const Chunk c = next_chunk(bytes, n, pos, name);
    if (!is_type(c, "IHDR") || c.len != 13) refuse(name, "the first chunk is not a 13-byte IHDR");
    const uint32_t w = be32(c.data), h = be32(c.data + 4);
    const int depth = c.data[8], colour = c.data[9], compression = c.data[10], filter = c.data[11], interlace = c.data[12];
    if (w == 0 || h == 0 || w > 0x7fffffffu || h > 0x7fffffffu) refuse(name, "IHDR: invalid size " + std::to_string(w) + " x " + std::to_string(h));
    if ((uint64_t)w * (uint64_t)h > kMaxPixels) refuse(name, "IHDR: " + std::to_string(w) + " x " + std::to_string(h) + " pixels are more than this reader takes");
    if (depth != 8) refuse(name, "bit depth " + std::to_string(depth) + " (only 8-bit images are read)");
    if (colour != 2 && colour != 6) refuse(name, "colour type " + std::to_string(colour) + " (only RGB and RGBA images are read)");
    if (compression != 0 || filter != 0) refuse(name, "IHDR: unknown compression or filter method");
    if (interlace != 0) refuse(name, "interlaced images are not read");
    Header hd;
    hd.width = (int)w, hd.height = (int)h, hd.channels = colour == 2 ? 3 : 4;
    return hd;
}

int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

std::vector<uint8_t> read_file(const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("PNG " + path + ": cannot open the file");
    std::vector<uint8_t> bytes;
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    if (bad) throw std::runtime_error("PNG " + path + ": read error");
    return bytes;
}

}  // namespace

PngImage png_decode(const uint8_t* bytes, size_t n, const std::string& name) {
    size_t pos = 0;
    const Header hd = read_header(bytes, n, &pos, name);
    std::vector<uint8_t> z;  // the IDAT chunks, concatenated
    bool seen_idat = false, idat_closed = false, seen_end = false;
    while (!seen_end) {
        const Chunk c = next_chunk(bytes, n, &pos, name);
        if (is_type(c, "IDAT")) {
            if (idat_closed) refuse(name, "IDAT chunks are not consecutive");
            seen_idat = true;
            z.insert(z.end(), c.data, c.data + c.len);
            continue;
        }
        if (seen_idat) idat_closed = true;
        if (is_type(c, "IEND")) {
            seen_end = true;
        } else if (is_type(c, "IHDR")) {
            refuse(name, "a second IHDR");
        } else if (!(c.type[0] & 0x20) && !is_type(c, "PLTE")) {  // (PLTE in an RGB / RGBA file is a suggested palette: ignored)
            refuse(name, "unknown critical chunk " + std::string((const char*)c.type, 4));
        }
    }
    if (!seen_idat) refuse(name, "no IDAT chunk");

    const size_t bpp = (size_t)hd.channels, stride = (size_t)hd.width * bpp;
    const uint64_t expect = (uint64_t)hd.height * (1 + (uint64_t)stride);
    // deflate expands by less than 1032 : 1, so a short stream cannot hold the image: refused before anything of the image's
    // size is allocated (an IHDR may claim any size)
    if (expect > (uint64_t)z.size() * 1032 + 64) refuse(name, "the inflated data is shorter than the image");
    std::vector<uint8_t> raw((size_t)expect);
    z_stream s;
    std::memset(&s, 0, sizeof(s));
    if (inflateInit(&s) != Z_OK) refuse(name, "zlib inflateInit failed");
    s.next_in = z.data();
    size_t in_left = z.size(), out_done = 0;
    int rc = Z_OK;
    uint8_t extra = 0;
    bool probing = false;  // the image is full and the one spare byte is on offer
    while (rc == Z_OK) {  // (avail_in / avail_out are uInt: fed in pieces)
        if (s.avail_in == 0 && in_left > 0) {
            const uInt step = in_left > (1u << 30) ? (1u << 30) : (uInt)in_left;
            s.avail_in = step;
            in_left -= step;
        }
        if (s.avail_out == 0) {
            if (out_done < raw.size()) {
                const size_t room = raw.size() - out_done;
                const uInt step = room > (1u << 30) ? (1u << 30) : (uInt)room;
                s.next_out = raw.data() + out_done;
                s.avail_out = step;
                out_done += step;
            } else {  // the image is full: one byte more decides between "ended exactly" and "too long"
                if (probing) break;
                s.next_out = &extra;
                s.avail_out = 1;
                probing = true;
            }
        }
        const uInt in_before = s.avail_in, out_before = s.avail_out;
        rc = inflate(&s, Z_NO_FLUSH);
        if (rc == Z_OK && s.avail_in == in_before && s.avail_out == out_before) break;  // no progress: out of input
        if (rc == Z_BUF_ERROR) break;
    }
    const uint64_t produced = (uint64_t)s.total_out;
    inflateEnd(&s);
    if (probing && (s.avail_out == 0 || produced > expect)) refuse(name, "the inflated data is longer than the image");
    if (rc != Z_STREAM_END) {
        if (rc == Z_DATA_ERROR || rc == Z_NEED_DICT || rc == Z_MEM_ERROR || rc == Z_STREAM_ERROR) refuse(name, "corrupt zlib stream");
        refuse(name, "the inflated data is shorter than the image (truncated zlib stream)");
    }
    if (produced != expect) refuse(name, "the inflated data is shorter than the image");

    PngImage img;
    img.width = hd.width, img.height = hd.height;
    img.rgba.resize((size_t)hd.width * (size_t)hd.height * 4);
    std::vector<uint8_t> prev(stride, 0), cur(stride);
    for (int y = 0; y < hd.height; ++y) {
        const uint8_t* line = raw.data() + (size_t)y * (1 + stride);
        const int ft = line[0];
        if (ft > 4) refuse(name, "filter type " + std::to_string(ft) + " in row " + std::to_string(y));
        const uint8_t* in = line + 1;
        for (size_t i = 0; i < stride; ++i) {
            const int a = i >= bpp ? cur[i - bpp] : 0, b = prev[i], c = i >= bpp ? prev[i - bpp] : 0;
            int v = in[i];
            switch (ft) {
                case 1: v += a; break;
                case 2: v += b; break;
                case 3: v += (a + b) >> 1; break;
                case 4: v += paeth(a, b, c); break;
                default: break;
            }
            cur[i] = (uint8_t)(v & 0xff);
        }
        uint8_t* out = img.rgba.data() + (size_t)y * hd.width * 4;
        if (hd.channels == 4) {
            std::memcpy(out, cur.data(), stride);
        } else {
            for (int x = 0; x < hd.width; ++x) {
                out[4 * x + 0] = cur[3 * (size_t)x + 0];
                out[4 * x + 1] = cur[3 * (size_t)x + 1];
                out[4 * x + 2] = cur[3 * (size_t)x + 2];
                out[4 * x + 3] = 255;
            }
        }
        prev.swap(cur);
    }
    return img;
}

PngImage png_read(const std::string& path) {
    const std::vector<uint8_t> bytes = read_file(path);
    return png_decode(bytes.data(), bytes.size(), path);
}

void png_read_size(const std::string& path, int* width, int* height) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("PNG " + path + ": cannot open the file");
    uint8_t head[33];  // signature + IHDR chunk
    const size_t got = std::fread(head, 1, sizeof(head), f);
    std::fclose(f);
    size_t pos = 0;
    const Header hd = read_header(head, got, &pos, path);
    *width = hd.width, *height = hd.height;
}

}  // namespace rto
