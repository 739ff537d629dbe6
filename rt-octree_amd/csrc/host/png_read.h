// png_read.h -- reader for the PNG files a dataset's ground-truth images and this project's own writer (cli/imwrite.cpp)
// produce: 8 bits per sample, RGB or RGBA, not interlaced.  png.h is not installed in this image, so the container is read by
// hand (signature, chunk lengths against the file size, the CRC of every chunk, IDAT chunks concatenated, zlib inflate into
// exactly height * (1 + width * bpp) bytes, the five row filters).  Everything else -- 16-bit, palette, grey or interlaced
// images, truncated files, inflated data too short or too long, a bad CRC, a filter type above 4 -- is refused with a
// std::runtime_error that names the file.  Host only.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace rto {

struct PngImage {
    int width = 0, height = 0;
    std::vector<uint8_t> rgba;  // [height][width][4]; alpha 255 for an RGB file
};

// the whole file
PngImage png_read(const std::string& path);
// signature and IHDR only (validated as png_read validates them)
void png_read_size(const std::string& path, int* width, int* height);
// the same on a file image in memory; `name` is what the error messages call it
PngImage png_decode(const uint8_t* bytes, size_t n, const std::string& name);

}  // namespace rto
