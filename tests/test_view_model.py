"""CPU checks of the tracking view: the model's own properties (tests/view_model.py), the new declarations as plain C, the exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import view_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_marker_sizes():
    assert len(vm.marker_pixels(0, 0, 10)) == 37
    assert len(vm.marker_pixels(5, -3, 2)) == 9
    assert vm.marker_pixels(7, 9, 0) == [(7, 9)]
    g = np.zeros((40, 40), np.uint8)
    out = vm.render(g, markers=[(20, 20, 0, 10)], palette=[(1, 2, 3)])
    assert (out[:, :, 0] == 1).sum() == 37 and (out[:, :, 2] == 3).sum() == 37
    assert tuple(out[20, 23]) == (1, 2, 3) and tuple(out[20, 24]) == (0, 0, 0) and tuple(out[23, 21]) == (1, 2, 3) and tuple(out[23, 22]) == (0, 0, 0)


@pytest.mark.parametrize("seg", [(0, 0, 9, 0), (3, 4, 3, -8), (0, 0, 7, 7), (0, 0, -7, 7), (2, 1, 13, 5), (2, 1, -4, 19), (5, 5, 5, 5),
                                 (-3, 8, 11, -2), (10, 10, 3, 9), (0, 0, 1, 1000)])
def test_segment_has_n_plus_1_pixels_both_ends_and_is_8_connected(seg):
    px = vm.segment_pixels(*seg)
    n = max(abs(seg[2] - seg[0]), abs(seg[3] - seg[1]))
    assert len(px) == n + 1 and len(set(px)) == n + 1
    assert px[0] == seg[:2] and px[-1] == seg[2:]
    for a, b in zip(px, px[1:]):
        assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1


# one hand-computed segment per octant: n = 5, minor delta 2 (or -2); pixel k has minor offset floor((4k + 5) / 10) for +2:
# k = 0..5 -> 0, 0, 1, 1, 2, 2; for -2 floor((-4k + 5) / 10): 0, 0, -1, -1, -2, -2  (truncation would give 0, 0, 0, 0, -1, -1)
PLUS, MINUS = [0, 0, 1, 1, 2, 2], [0, 0, -1, -1, -2, -2]
OCTANTS = [((5, 2), "x", 1, PLUS), ((2, 5), "y", 1, PLUS), ((-2, 5), "y", 1, MINUS), ((-5, 2), "x", -1, PLUS),
           ((-5, -2), "x", -1, MINUS), ((-2, -5), "y", -1, MINUS), ((2, -5), "y", -1, PLUS), ((5, -2), "x", 1, MINUS)]


@pytest.mark.parametrize("d,major,step,minor", OCTANTS)
def test_floor_division_in_every_octant(d, major, step, minor):
    px = vm.segment_pixels(10, 20, 10 + d[0], 20 + d[1])
    if major == "x":
        want = [(10 + step * k, 20 + minor[k]) for k in range(6)]
    else:
        want = [(10 + minor[k], 20 + step * k) for k in range(6)]
    assert px == want


def test_priority():
    g = np.full((30, 30), 9, np.uint8)
    pal = [(10, 0, 0), (20, 0, 0), (30, 0, 0), (40, 0, 0)]
    a = vm.render(g, segments=[(0, 15, 29, 15, 2), (15, 0, 15, 29, 3)], markers=[(15, 15, 0, 10), (17, 15, 1, 10)], palette=pal)
    assert a[15, 16, 0] == 20 and a[15, 13, 0] == 10          # the later marker beats the earlier one where they overlap
    assert a[15, 15, 0] == 20 and a[12, 15, 0] == 10          # any marker beats any segment (the crossing lies under both discs)
    assert a[15, 2, 0] == 30 and a[2, 15, 0] == 40            # segments alone
    b = vm.render(g, segments=[(15, 0, 15, 29, 3), (0, 15, 29, 15, 2)], markers=[(17, 15, 1, 10), (15, 15, 0, 10)], palette=pal)
    assert b[15, 16, 0] == 10 and b[15, 19, 0] == 20
    c = vm.render(g, segments=[(0, 15, 29, 15, 2), (15, 0, 15, 29, 3)], palette=pal)
    assert c[15, 15, 0] == 40                                 # the later segment wins the crossing
    c = vm.render(g, segments=[(15, 0, 15, 29, 3), (0, 15, 29, 15, 2)], palette=pal)
    assert c[15, 15, 0] == 30
    assert a[0, 0, 0] == 9 and (a[:, :, 1] == a[:, :, 2]).all()


def test_outside_primitives_leave_the_canvas_alone():
    g = np.random.RandomState(3).randint(0, 256, size=(41, 67), dtype=np.uint8)
    for ch in (3, 4):
        want = np.repeat(g[:, :, None], ch, 2)
        if ch == 4:
            want[:, :, 3] = 255
        out = vm.render(g, segments=[(-50, -1, 200, -1, 0), (67, 0, 67, 40, 0), (-8192, 41, 8191, 41, 0), (-5, -5, -5, -5, 0), (70, 10, 8191, 30, 0)],
                        markers=[(-4, 10, 0, 10), (30, -4, 0, 10), (70, 44, 0, 10), (8191, -8192, 0, 2), (33, 45, 0, 10)],
                        palette=[(255, 0, 255)], channels=ch)
        np.testing.assert_array_equal(out, want)
    # ... and one pixel closer they show
    assert tuple(vm.render(g, markers=[(-3, 10, 0, 10)], palette=[(255, 0, 255)])[10, 0]) == (255, 0, 255)


def test_view_primitives_from_a_feature_list():
    f = np.zeros(3, [("x", "f8"), ("y", "f8"), ("track_id", "i8"), ("age", "i4"), ("n_trail", "i4"), ("trail", "f8", (8, 2))])
    f[0] = (10.9, 20.2, 7, 3, 2, np.arange(16).reshape(8, 2) + 0.5)
    f[1] = (30.0, 40.99, -1, 0, 0, np.zeros((8, 2)))
    f[2] = (50.5, 60.5, 9, 12, 0, np.zeros((8, 2)))
    segs, mk = vm.view_primitives(f)
    assert segs == [] and mk == [(10, 20, 0, 10), (50, 60, 0, 10)]
    segs, mk = vm.view_primitives(f, color_mode=1, draw_new=1, trail=4)
    assert mk == [(30, 40, 4, 2), (10, 20, 1, 10), (50, 60, 3, 10)]
    assert segs == [(10, 20, 0, 1, 5), (0, 1, 2, 3, 5)]


C_SNIPPET = r"""
#include "XRSLAM.h"
#include "xrslam_hip.h"
int use(void) {
    XRSLAMAmdFeature f[4];
    XRSLAMAmdViewOptions o = {1, 1, 4};
    double t;
    xrhip_view_marker m = {1, 2, 0u | (10u << 8)};
    xrhip_view_segment s = {0, 0, 5, 5, 1u};
    unsigned char pal[6] = {0, 255, 255, 255, 160, 0}, out[12];
    int n = XRSLAMAmdGetFeatures(f, 4, &t) + XRSLAMAmdInstanceGetFeatures(0, f, 4, &t);
    XRSLAMAmdSetFeatureHistory(XRSLAM_AMD_VIEW_MAX_TRAIL);
    XRSLAMAmdInstanceSetFeatureHistory(0, 4);
    n += XRSLAMAmdRenderTrackingView(out, 6, 3, 0, &o) + XRSLAMAmdInstanceRenderTrackingView(0, out, 6, 3, 0, &o);
    n += (int)sizeof(f[0].trail) + xrhip_image_render_view(0, &s, 1, &m, 1, pal, 2, out, 6, 3, 0);
    return n + xrhip_debug_view_timing(0, -1, 0, 0, 0);
}
"""


def test_new_declarations_compile_as_c(tmp_path):
    src = tmp_path / "view_decl.c"
    src.write_text(C_SNIPPET)
    p = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_library_exports_the_view_symbols():
    from xrslam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("xrhip_image_render_view", "xrhip_debug_view_timing", "XRSLAMAmdGetFeatures", "XRSLAMAmdSetFeatureHistory",
                 "XRSLAMAmdRenderTrackingView", "XRSLAMAmdInstanceGetFeatures", "XRSLAMAmdInstanceSetFeatureHistory",
                 "XRSLAMAmdInstanceRenderTrackingView"):
        assert hasattr(lib, name), name
    from xrslam_amd.harness import runner
    assert C.sizeof(runner.XRSLAMAmdFeature) == 8 + 8 + 8 + 4 + 4 + 128
