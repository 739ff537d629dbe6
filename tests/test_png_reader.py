"""rto_image_read_png / rt_octree_amd.read_png (csrc/host/png_read.cpp): the reader that brings a dataset's ground-truth
images in.  Host only.  The encoder below is the test's own (zlib + binascii.crc32): every row filter, RGB and RGBA, one and
several IDAT chunks, stored and compressed streams must decode to the exact bytes; PIL's and the project's own files too; and
everything the reader does not take must come back as a Python error that names the file."""
import binascii
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import rt_octree_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = b"\x89PNG\r\n\x1a\n"


def chunk(kind, data, crc=None):
    c = binascii.crc32(kind + data) & 0xffffffff if crc is None else crc
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", c)


def ihdr(w, h, depth=8, colour=6, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def filtered_rows(img, filters):
    """img uint8 [H,W,C] -> the bytes inflate must produce: per row the filter type and the filtered line (PNG spec 9.2)"""
    H, W, Cn = img.shape
    lines = img.reshape(H, W * Cn).astype(np.int64)
    out = bytearray()
    for y in range(H):
        ft = filters[y]
        cur = lines[y]
        up = lines[y - 1] if y > 0 else np.zeros_like(cur)
        left = np.concatenate([np.zeros(Cn, np.int64), cur[:-Cn]])
        upleft = np.concatenate([np.zeros(Cn, np.int64), up[:-Cn]])
        if ft == 0:
            pred = np.zeros_like(cur)
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (left + up) // 2
        else:
            pred = np.array([_paeth(int(a), int(b), int(c)) for a, b, c in zip(left, up, upleft)], np.int64)
        out.append(ft)
        out += bytes(((cur - pred) & 0xff).astype(np.uint8))
    return bytes(out)


def encode(img, filters, level=9, idats=1, raw=None):
    H, W, Cn = img.shape
    raw = filtered_rows(img, filters) if raw is None else raw
    z = zlib.compress(raw, level)
    step = max(1, -(-len(z) // idats))
    body = b"".join(chunk(b"IDAT", z[i:i + step]) for i in range(0, len(z), step))
    return SIG + ihdr(W, H, colour=2 if Cn == 3 else 6) + body + chunk(b"IEND", b"")


def expect_rgba(img):
    if img.shape[2] == 4:
        return img
    return np.concatenate([img, np.full(img.shape[:2] + (1,), 255, np.uint8)], 2)


def _image(h, w, cn, seed):
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (h, w, cn)).astype(np.uint8)
    img[: h // 2] = (img[: h // 2] // 64) * 64  # (runs, so that the filters and deflate have something to do)
    return img


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (48, 64)])
@pytest.mark.parametrize("cn", [3, 4])
def test_every_filter_chunking_and_level_decodes_to_the_exact_bytes(tmp_path, size, cn):
    h, w = size
    img = _image(h, w, cn, seed=h * 10 + cn)
    cases = [([ft] * h, 9, 1) for ft in range(5)]
    cases += [([y % 5 for y in range(h)], 9, 1), ([(y * 3 + 1) % 5 for y in range(h)], 0, 1),
              ([(y + 2) % 5 for y in range(h)], 9, 4), ([4 - y % 5 for y in range(h)], 0, 3)]
    for k, (filters, level, idats) in enumerate(cases):
        p = tmp_path / ("f%d.png" % k)
        p.write_bytes(encode(img, filters, level, idats))
        got = R.read_png(str(p))
        assert got.dtype == np.uint8 and got.shape == (h, w, 4)
        assert np.array_equal(got, expect_rgba(img)), (size, cn, filters[:5], level, idats)


def test_pil_files_decode_like_pil(tmp_path):
    from PIL import Image
    for cn, mode in ((3, "RGB"), (4, "RGBA")):
        img = _image(48, 64, cn, seed=cn)
        for opt in (False, True):
            p = str(tmp_path / ("pil_%s_%d.png" % (mode, opt)))
            Image.fromarray(img, mode).save(p, optimize=opt)
            assert np.array_equal(R.read_png(p), np.asarray(Image.open(p).convert("RGBA")))


def test_sizes_only_and_null_arguments(tmp_path):
    import ctypes as C
    p = tmp_path / "a.png"
    p.write_bytes(encode(_image(5, 3, 4, 0), [0] * 5))
    w, h = C.c_int(0), C.c_int(0)
    L = R.lib()
    assert L.rto_image_read_png(str(p).encode(), C.byref(w), C.byref(h), None, 0) == 0 and (w.value, h.value) == (3, 5)
    buf = np.full(3 * 5 * 4, 7, np.uint8)
    w.value = h.value = 0
    assert L.rto_image_read_png(str(p).encode(), C.byref(w), C.byref(h), C.c_void_p(buf.ctypes.data), buf.nbytes - 1) == 0
    assert (w.value, h.value) == (3, 5) and (buf == 7).all()  # cap too small: sizes only, nothing written
    assert L.rto_image_read_png(None, C.byref(w), C.byref(h), None, 0) == -1
    assert L.rto_image_read_png(str(p).encode(), None, C.byref(h), None, 0) == -1
    rc = L.rto_image_read_png(str(tmp_path / "missing.png").encode(), C.byref(w), C.byref(h), None, 0)
    assert rc == -5 and "missing.png" in L.rto_last_error().decode()


def _refused(tmp_path, name, data, word):
    p = tmp_path / name
    p.write_bytes(data)
    with pytest.raises(R.RtoError) as e:
        R.read_png(str(p))
    assert e.value.code == -5 and name in e.value.msg and word in e.value.msg, e.value.msg


def test_refusals(tmp_path):
    img = _image(6, 7, 4, seed=1)
    raw = filtered_rows(img, [0, 1, 2, 3, 4, 0])
    good = encode(img, [0, 1, 2, 3, 4, 0])
    p = tmp_path / "good.png"
    p.write_bytes(good)
    assert np.array_equal(R.read_png(str(p)), img)
    idat = chunk(b"IDAT", zlib.compress(raw))
    end = chunk(b"IEND", b"")
    _refused(tmp_path, "sixteen.png", SIG + ihdr(7, 6, depth=16) + idat + end, "bit depth 16")
    _refused(tmp_path, "palette.png", SIG + ihdr(7, 6, colour=3) + chunk(b"PLTE", b"\0" * 6) + idat + end, "colour type 3")
    _refused(tmp_path, "grey.png", SIG + ihdr(7, 6, colour=0) + idat + end, "colour type 0")
    _refused(tmp_path, "greyalpha.png", SIG + ihdr(7, 6, colour=4) + idat + end, "colour type 4")
    _refused(tmp_path, "interlaced.png", SIG + ihdr(7, 6, interlace=1) + idat + end, "interlaced")
    _refused(tmp_path, "badcrc.png", SIG + ihdr(7, 6) + chunk(b"IDAT", zlib.compress(raw), crc=0x12345678) + end, "CRC")
    flipped = bytearray(good)
    flipped[len(SIG) + 25 + 8 + 3] ^= 1  # a data byte of the IDAT chunk (behind the 25 bytes of IHDR), its CRC left as it was
    _refused(tmp_path, "flipped.png", bytes(flipped), "CRC")
    for cut in (len(good) - 1, len(good) - 12, len(SIG) + 30, 20, 4, 0):
        _refused(tmp_path, "truncated.png", good[:cut], "truncated" if cut >= 8 else "signature")
    bad_filter = bytearray(raw)
    bad_filter[(1 + 7 * 4) * 2] = 5
    _refused(tmp_path, "filter5.png", encode(img, None, raw=bytes(bad_filter)), "filter type 5")
    _refused(tmp_path, "short.png", encode(img, None, raw=raw[:-1]), "shorter")
    _refused(tmp_path, "long.png", encode(img, None, raw=raw + b"\0"), "longer")
    _refused(tmp_path, "halfstream.png", SIG + ihdr(7, 6) + chunk(b"IDAT", zlib.compress(raw)[:-6]) + end, "shorter")
    _refused(tmp_path, "noidat.png", SIG + ihdr(7, 6) + end, "IDAT")
    _refused(tmp_path, "noend.png", SIG + ihdr(7, 6) + idat, "truncated")
    _refused(tmp_path, "huge.png", SIG + ihdr(1 << 16, 1 << 15) + idat + end, "pixels")  # 2^31 pixels
    _refused(tmp_path, "zero.png", SIG + ihdr(0, 6) + idat + end, "size")
    _refused(tmp_path, "critical.png", SIG + ihdr(7, 6) + chunk(b"ABCD", b"x") + idat + end, "critical chunk")
    _refused(tmp_path, "notpng.png", b"GIF89a" + good, "signature")
    # an ancillary chunk before and after the image data is skipped
    p.write_bytes(SIG + ihdr(7, 6) + chunk(b"tEXt", b"k\0v") + idat + chunk(b"tIME", b"1234567") + end)
    assert np.array_equal(R.read_png(str(p)), img)


@pytest.fixture(scope="module")
def sanitizer_run(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("png_san") / "writer.png")
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    assert "LD_PRELOAD" not in env
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "run_png.sh"), "300", out], capture_output=True, text=True,
                       timeout=600, env=env)
    return r, out


def test_reader_and_writer_are_clean_under_the_sanitizers(sanitizer_run):
    """tools/sanitize/run_png.sh: a stand-alone program built with -fsanitize=address,undefined round-trips images through the
    project's writer and reader, then reads 300 mutated files: each loads or is refused, nothing else; it also merges
    hand-made RANK_METRICS lines (cli/rank_metrics.h)"""
    r, _ = sanitizer_run
    assert r.returncode == 0, r.stdout + r.stderr
    assert "png_fuzz: clean:" in r.stdout and "300 mutations" in r.stdout and "RANK_METRICS merge ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_file_of_the_projects_own_writer_round_trips(sanitizer_run):
    """cli/imwrite.cpp (through the sanitizer program) -> read_png: the pattern the program wrote"""
    r, out = sanitizer_run
    assert r.returncode == 0, r.stdout + r.stderr
    y, x, c = np.meshgrid(np.arange(48), np.arange(64), np.arange(4), indexing="ij")
    want = ((x * 7 + y * 13 + c * 29 + x * y) & 0xff).astype(np.uint8)
    assert np.array_equal(R.read_png(out), want)
