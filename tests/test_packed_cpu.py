"""The host side of the packed 10 / 12-bit formats without a GPU.

tests/host_check/packed_host.cpp is a stand-alone program (its own main, no GPU code, never loaded into Python) built with
AddressSanitizer and UBSan over xrslam_amd/csrc/host/pixel_format.hpp: it runs describe_pixel_format, check_frame_geometry,
reduce_frame and scale_frame -- the unpacking of the CPU reference build -- over the frames written here, each in a heap block of
exactly the bytes a packed frame has, and prints a checksum per plane, which must be the checksum of the model's plane
(tests/packed_model.py: the existing GRAY16 / BAYER_*16 models over the unpacked samples).

Frames: all 20 formats at 32, 33, 34, 35 x 33 (every w % 4: rows that end mid-group, every bit phase at a row's end), dense and with a
padded stride at an odd base offset; limited_range on the mono forms; scaled geometries with odd crop origins (the crop starts
mid-group, the Bayer phase shifts) and a ratio-1 crop.

The CPU reference build (oracle/_build/libxrslam_oracle.so: the product's host sources over a shim without the format uploads)
unpacks such frames itself: a packed stream writes the output log of the same samples pushed as GRAY16 with bits 10."""
import os
import struct
import subprocess

import numpy as np

from tests import packed_model as pk
from tests.test_bayer_cpu import fnv1a

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_check", "packed_host.cpp")
OUT = os.path.join(ROOT, "tests", "host_check", "_build", "packed_host")
DEPS = [SRC, os.path.join(ROOT, "xrslam_amd", "csrc", "host", "pixel_format.hpp"), os.path.join(ROOT, "include", "xrslam_hip.h")]
# (src_width, src_height, crop_x, crop_y, cw, ch) -> 32 x 32
SCALED = [(70, 67, 3, 5, 61, 59), (65, 65, 1, 1, 64, 64), (40, 36, 1, 0, 32, 32), (41, 36, 6, 3, 35, 33)]


def block_of(rows, pad, offset, rows_needed, last_row_bytes, seed):
    """packed rows [h][n] -> (the bytes from the block's first byte to the frame's last needed byte: `offset` bytes, then rows of n + pad
    bytes, the last needed row cut after last_row_bytes; the row stride)"""
    h, n = rows.shape
    stride = n + pad
    buf = np.random.RandomState(seed).randint(0, 256, size=offset + stride * h, dtype=np.uint8)
    buf[offset:].reshape(h, stride)[:, :n] = rows
    return buf[:offset + stride * (rows_needed - 1) + last_row_bytes].tobytes(), stride


def cases():
    """-> [(header words, block, the model's plane)]"""
    out = []
    for fmt in pk.FORMATS:
        packing = pk.PACKING[fmt]
        for w in (32, 33, 34, 35):
            h = 33
            rows = pk.pack(pk.random_samples(w, h, packing, seed=100 * fmt + w), packing)
            for pad, offset in ((0, 0), (5, 1)):
                lim = 1 if fmt in pk.MONO and pad else 0
                block, stride = block_of(rows, pad, offset, h, rows.shape[1], seed=w + pad)
                out.append(((fmt, lim, stride, offset, 0, w, h, 0, 0, 0, 0, 0, 0, len(block)), block, pk.reduce(rows, w, fmt, lim)))
        for k, geo in enumerate(SCALED):
            sw, sh, x, y, cw, ch = geo
            lim = 1 if fmt in pk.MONO and k == 0 else 0
            rows = pk.pack(pk.random_samples(sw, sh, packing, seed=200 * fmt + k), packing)
            block, stride = block_of(rows, 5, 1, y + ch, pk.row_bytes(x + cw, packing), seed=k)
            out.append(((fmt, lim, stride, 1, 1, 32, 32) + geo + (len(block),), block, pk.scale(rows, geo, 32, 32, fmt, lim)))
    return out


def test_host_unpacking_equals_the_model_and_is_clean_under_the_sanitizers(tmp_path):
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
        assert line == "case %d %016x" % (k, fnv1a(want.tobytes())), "case %d: %s, words %s" % (k, pk.NAMES[words[0]], words)


CALLER = r"""
#include "XRSLAM.h"
#include "xrslam_hip.h"
#define SAME(n, v) ((int)XRSLAM_AMD_PIXEL_##n == XRHIP_PIXFMT_##n && XRHIP_PIXFMT_##n == (v))
int mono_matches[SAME(GRAY10_MIPI, 32) && SAME(GRAY12_MIPI, 33) && SAME(GRAY10P, 34) && SAME(GRAY12P, 35) ? 1 : -1];
int mipi_matches[SAME(BAYER_RGGB10_MIPI, 40) && SAME(BAYER_GRBG10_MIPI, 41) && SAME(BAYER_GBRG10_MIPI, 42) && SAME(BAYER_BGGR10_MIPI, 43) &&
                 SAME(BAYER_RGGB12_MIPI, 44) && SAME(BAYER_GRBG12_MIPI, 45) && SAME(BAYER_GBRG12_MIPI, 46) && SAME(BAYER_BGGR12_MIPI, 47) ? 1 : -1];
int lsb_matches[SAME(BAYER_RGGB10P, 48) && SAME(BAYER_GRBG10P, 49) && SAME(BAYER_GBRG10P, 50) && SAME(BAYER_BGGR10P, 51) &&
                SAME(BAYER_RGGB12P, 52) && SAME(BAYER_GRBG12P, 53) && SAME(BAYER_GBRG12P, 54) && SAME(BAYER_BGGR12P, 55) ? 1 : -1];
int old_ones_stay[SAME(BAYER_BGGR16, 23) && SAME(P010, 10) ? 1 : -1];
"""


def test_the_format_numbers_agree_in_both_headers_and_in_python(tmp_path):
    from tests import bayer_model as bm
    from tests import pixfmt_model as pm
    from xrslam_amd import abi
    from xrslam_amd.harness import runner
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++17")):
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "gcc" else "c++", "-I" + os.path.join(ROOT, "include"), "-c",
                               str(src), "-o", str(tmp_path / ("caller_%s.o" % cc))])
    for fmt, name in pk.NAMES.items():
        assert getattr(abi, "PIXFMT_" + name.upper()) == fmt == runner.PACKED_PIXEL_FORMATS[name]
        packing, bits, phase = abi.PIXFMT_PACKED[fmt]
        assert (packing == "mipi") == (pk.PACKING[fmt] in (pk.MIPI10, pk.MIPI12)) and bits == pk.BITS[pk.PACKING[fmt]]
        assert phase == (None if fmt in pk.MONO else bm.PHASE[pk.UNPACKED[fmt]])
        for w in (1, 2, 3, 4, 5, 752):
            assert abi.packed_row_bytes(fmt, w) == pk.row_bytes(w, pk.PACKING[fmt])
    assert sorted(abi.PIXFMT_PACKED) == sorted(pk.FORMATS) == sorted(runner.PACKED_PIXEL_FORMATS.values())
    # the table of the unpacked formats is what it was
    want = {n: i for i, n in enumerate(pm.NAMES)}
    want.update({n: f for f, n in bm.NAMES.items()})
    assert runner.PIXEL_FORMATS == want and sorted(want.values()) == list(range(11)) + list(range(16, 24))
    f = runner.frame_format("gray12p")
    assert (f.format, f.bits, f.limited_range) == (35, 0, 0)
    f = runner.frame_format(("bayer_gbrg10_mipi", 0, 0))
    assert (f.format, f.bits, f.limited_range) == (42, 0, 0)
    f = runner.frame_format(("gray16", 10))
    assert (f.format, f.bits) == (5, 10)


# ------------------------------------------------------------------------------------------------ the CPU reference pipeline
def test_cpu_reference_unpacks_a_packed_stream_to_the_gray16_streams_log():
    from tests import pixfmt_model as pm
    from tests.test_pixfmt_cpu import BENCH_YAML, N, ORACLE_LIB, _run
    from xrslam_amd.harness import scene
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    q = scene.make_sequence(n_frames=N, seed=1)
    g = q["frames"]
    n, h, w = g.shape
    s10 = (g.astype(np.int64) << 2) | np.random.RandomState(5).randint(0, 4, size=g.shape)     # 10-bit samples, noise in the low bits
    gray16 = pm.samples16(s10)
    np.testing.assert_array_equal(pm.reduce(gray16, pm.GRAY16, 10), g)
    want = _run(q, gray16, ("gray16", 10))
    assert want[3] == N and 1 in want[2], "the GRAY16 stream does not reach TRACKING_SUCCESS within %d frames" % N
    for packing, name in ((pk.MIPI10, "gray10_mipi"), (pk.P10, "gray10p")):
        rows = np.stack([pk.pack(s, packing) for s in s10])
        buf = np.full(rows.shape[:2] + (rows.shape[2] + 3,), 0xEE, np.uint8)     # rows padded by 3 bytes
        frames = buf[:, :, :rows.shape[2]]
        frames[...] = rows
        got = _run(q, frames, name)
        assert got[3] == N, name
        assert got[0] == want[0], "%s: the output log differs from the GRAY16 run's" % name
    # a stride one byte short of the packed row drops the frame with an error that names it
    from xrslam_amd.harness import runner
    s = runner.Session(ORACLE_LIB, dict(q, frames=np.ascontiguousarray(frames[:, :, :-1])), slam_yaml=BENCH_YAML, pixel_format="gray10p")
    assert s.step()
    assert "stride" in s.error() and s.times().frames == 0
    s.close()
