"""The host side of the Bayer formats without a GPU.

tests/host_check/bayer_host.cpp is a stand-alone program (its own main, no GPU code, never loaded into Python) built with
AddressSanitizer and UBSan over xrslam_amd/csrc/host/pixel_format.hpp: it runs reduce_frame / scale_frame -- the demosaic of the CPU
reference build -- over the frames written here, each in a heap block of exactly the bytes a frame has, and prints a checksum per
plane, which must be the checksum of the model's plane (tests/bayer_model.py).  It also checks the argument rules: 11..15 and 24 are
not formats, limited_range is refused, bits 7 and 17 are refused for the 16-bit formats.

Frames: all eight formats at 32, 33, 34, 35 x 33, dense and with a padded stride at an odd base offset (16-bit samples at odd
addresses); the scaled geometries of tests/test_bayer_gpu.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bayer_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_check", "bayer_host.cpp")
OUT = os.path.join(ROOT, "tests", "host_check", "_build", "bayer_host")
DEPS = [SRC, os.path.join(ROOT, "xrslam_amd", "csrc", "host", "pixel_format.hpp"), os.path.join(ROOT, "include", "xrslam_hip.h")]
BITS = (10, 12, 0, 16)
# (src_width, src_height, crop_x, crop_y, cw, ch) -> 32 x 32: odd crop origin and a non-integer ratio; 2x; a plain crop at (1, 0)
SCALED = [(70, 67, 3, 5, 61, 59), (64, 64, 0, 0, 64, 64), (40, 36, 1, 0, 32, 32)]


def fnv1a(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def block_of(px, pad, offset, rows_needed, last_row_bytes, seed):
    """[h][w][bpp] -> (the bytes from the block's first byte to the frame's last needed byte: `offset` bytes, then rows of w * bpp + pad
    bytes, the last needed row cut after last_row_bytes; the row stride)"""
    h, w, bpp = px.shape
    stride = w * bpp + pad
    buf = np.random.RandomState(seed).randint(0, 256, size=offset + stride * h, dtype=np.uint8)
    rows = buf[offset:].reshape(h, stride)
    rows[:, :w * bpp] = px.reshape(h, w * bpp)
    return buf[:offset + stride * (rows_needed - 1) + last_row_bytes].tobytes(), stride


def cases():
    """-> [(header words, block, the model's plane)]"""
    out = []
    for fmt in bm.FORMATS:
        bpp = bm.BYTES[fmt]
        for k, w in enumerate((32, 33, 34, 35)):
            h = 33
            bits = BITS[k] if bpp == 2 else 0
            px = np.random.RandomState(100 * fmt + w).randint(0, 256, size=(h, w, bpp), dtype=np.uint8)
            if bpp == 2 and bits:
                px[..., 1] &= (1 << (bits - 8)) - 1 | (0 if k else 1 << (bits - 8))    # mostly inside the significant bits
            for pad, offset in ((0, 0), (5, 1), (6, 3)):
                block, stride = block_of(px, pad, offset, h, w * bpp, seed=w + pad)
                out.append(((fmt, bits, stride, offset, 0, w, h, 0, 0, 0, 0, 0, 0, len(block)), block, bm.reduce(px, fmt, bits)))
        for k, geo in enumerate(SCALED):
            sw, sh, x, y, cw, ch = geo
            bits = BITS[k] if bpp == 2 else 0
            px = np.random.RandomState(200 * fmt + k).randint(0, 256, size=(sh, sw, bpp), dtype=np.uint8)
            block, stride = block_of(px, 5, 1, y + ch, (x + cw) * bpp, seed=k)
            out.append(((fmt, bits, stride, 1, 1, 32, 32) + geo + (len(block),), block, bm.scale(px, geo, 32, 32, fmt, bits)))
    return out


def test_host_demosaic_equals_the_model_and_is_clean_under_the_sanitizers(tmp_path):
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(d) for d in DEPS):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", SRC, "-o", OUT])
    cs = cases()
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        for words, block, _ in cs:
            fh.write(struct.pack("<14i", *words))
            fh.write(block)
    p = subprocess.run([OUT, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == len(cs) + 1
    for k, ((words, _, want), line) in enumerate(zip(cs, lines)):
        assert line == "case %d %016x" % (k, fnv1a(want.tobytes())), "case %d: %s, words %s" % (k, bm.NAMES[words[0]], words)
    # (one plane per format and size / geometry, whatever the padding and offset: the checksums tell them apart)
    assert len({ln.split()[2] for ln in lines[:-1]}) == len(bm.FORMATS) * (4 + len(SCALED))


CALLER = r"""
#include "XRSLAM.h"
#include "xrslam_hip.h"
#define SAME(n, v) ((int)XRSLAM_AMD_PIXEL_BAYER_##n == XRHIP_PIXFMT_BAYER_##n && XRHIP_PIXFMT_BAYER_##n == (v))
int enum_matches[SAME(RGGB8, 16) && SAME(GRBG8, 17) && SAME(GBRG8, 18) && SAME(BGGR8, 19) && SAME(RGGB16, 20) && SAME(GRBG16, 21) &&
                 SAME(GBRG16, 22) && SAME(BGGR16, 23) && (int)XRSLAM_AMD_PIXEL_P010 == 10 ? 1 : -1];
"""


def test_the_format_numbers_agree_in_both_headers_and_in_python(tmp_path):
    from xrslam_amd import abi
    from xrslam_amd.harness import runner
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++17")):
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "gcc" else "c++", "-I" + os.path.join(ROOT, "include"), "-c",
                               str(src), "-o", str(tmp_path / ("caller_%s.o" % cc))])
    for fmt, name in bm.NAMES.items():
        assert getattr(abi, "PIXFMT_" + name.upper()) == fmt == runner.PIXEL_FORMATS[name]
    assert abi.PIXFMT_BAYER_BYTES == bm.BYTES
    f = runner.frame_format(("bayer_bggr16", 12))
    assert (f.format, f.bits, f.limited_range) == (23, 12, 0)
    assert sorted(runner.PIXEL_FORMATS.values()) == list(range(11)) + list(range(16, 24))
    assert C.sizeof(runner.XRSLAMAmdFrameFormat) == 12
