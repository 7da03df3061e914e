"""tests/contour_ref.py (the restatement the device's rotated box is compared against) pinned independently of the device:
closed forms of the contour area, the polygons the reference's unchanged tool returned (tests/golden/tracker_*.npz
`f_polygon`), and an independent hull + calipers implementation (tests/compat/cv2_stub: scipy ConvexHull, its own loop)."""
import os
import re

import numpy as np

import contour_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")


def area_of(m):
    c = R.components(m)
    assert len(c) == 1, len(c)
    return c[0]["area"]


def test_closed_forms_of_the_contour_area():
    m = np.zeros((20, 30), np.uint8)
    m[3:10, 4:15] = 1                                    # solid 11 x 7 rectangle: (w-1)(h-1)
    assert area_of(m) == 60.0
    m[:] = 0
    m[5, 5] = 1                                          # a single pixel
    assert area_of(m) == 0.0
    m[:] = 0
    m[5, 5:9] = 1                                        # a one-pixel-wide line: walked out and back
    assert area_of(m) == 0.0 and len(R.components(m)[0]["pts"]) == 6
    m[:] = 0
    m[3:10, 4:15] = 1
    m[5:8, 7:11] = 0                                     # a hole does not matter
    assert area_of(m) == 60.0
    m[:] = 0
    m[3:8, 3:8] = 1
    m[8, 8] = 1
    m[9:14, 9:14] = 1                                    # two 5 x 5 squares joined diagonally through one pixel
    assert area_of(m) == 32.0
    m[:] = 0
    m[2, 5] = m[3, 4] = m[3, 6] = m[4, 5] = 1            # the four 4-neighbours of an empty pixel
    assert area_of(m) == 2.0


def test_selection_is_strict_and_ties_go_to_the_first_raster_pixel():
    m = np.zeros((40, 60), np.uint8)
    m[5:16, 5:16] = 1                                    # 11 x 11: area exactly 100 -> not found
    r = R.mask_rbox(m)
    assert (r["area"], r["found"], r["n_components"]) == (100.0, 0, 1)
    m[5:16, 5:17] = 1                                    # 12 x 11: 110
    r = R.mask_rbox(m)
    assert (r["area"], r["found"]) == (110.0, 1)
    assert R.corner_set_distance(r["corners"], [[5, 5], [16, 5], [16, 15], [5, 15]]) == 0.0
    m[20:31, 30:42] = 1                                  # an equal second one later in raster order
    r = R.mask_rbox(m)
    assert r["n_components"] == 2 and r["margin"] == 0.0
    assert R.corner_set_distance(r["corners"], [[5, 5], [16, 5], [16, 15], [5, 15]]) == 0.0
    assert R.mask_rbox(np.zeros((4, 4), np.uint8))["found"] == 0


def golden_masks():
    out = []
    for variant in ("sharp", "base"):
        g = np.load(os.path.join(GOLD, "tracker_%s.npz" % variant), allow_pickle=False)
        H, W = g["frames"].shape[1:3]
        for f in range(g["f_mask_bits"].shape[0]):
            out.append((variant, f, np.unpackbits(g["f_mask_bits"][f])[:H * W].reshape(H, W), g["f_polygon"][f]))
    return out


def test_golden_masks_give_the_polygon_the_unchanged_tool_returned():
    """f_polygon went through a float32 boxPoints: 2^-24 * 512 = 3e-5 per coordinate covers that"""
    cases = golden_masks()
    assert len(cases) == 6
    areas = []
    for variant, f, mask, poly in cases:
        r = R.mask_rbox(mask)
        assert r["found"] == 1
        d = R.corner_set_distance(r["corners"], poly)
        print(variant, f, "area", r["area"], "distance to f_polygon", d)
        assert d <= 1e-4, (variant, f, d)
        areas.append(r["area"])
    assert areas == [58310.0, 72656.0, 76241.0, 40400.5, 11436.0, 8688.5]


def test_ellipses_against_the_independent_calipers():
    from tests.compat import cv2_stub as cv
    worst, gap = 0.0, np.inf
    for m in R.ellipse_masks():
        r = R.mask_rbox(m)
        assert r["found"] == 1 and r["n_components"] == 1
        _, cs, _ = cv.findContours(m, 0, 1)
        want = cv.boxPoints(cv.minAreaRect(cs[0])).astype(np.float64)
        worst = max(worst, R.corner_set_distance(r["corners"], want))
        gap = min(gap, r["rect_gap"])
    print("worst distance to the stub", worst, "smallest distinct-rectangle gap", gap)
    assert worst <= 1e-4
    assert gap >= 1e-7                                   # the input condition tests/test_gpu_rbox.py relies on


def test_noisy_recipe_has_a_clear_winner():
    for m in R.noisy_masks():
        r = R.mask_rbox(m)
        assert 123 <= r["n_components"] <= 168 and r["margin"] >= 76 and r["rect_gap"] >= 1e-7


def test_export_contract():
    """the C ABI carries the rotated box: declared in the product header, listed for the binding, ABI minor >= 7"""
    from siammask_amd import _lib
    hdr = open(os.path.join(REPO, "include", "siammask_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", hdr))
    for s in ("smk_mask_rbox", "smk_mask_rbox_workspace"):
        assert s in declared and s in _lib.SYMBOLS, s
    L = _lib.lib()
    assert L.smk_version() & 0xffff >= 7
    # host-side argument checks need no device: the size grows with the worst case of ceil(W/2) * H runs, bad geometry gives 0
    assert L.smk_mask_rbox_workspace(1, 320, 240) >= 240 * 160 * 4 + 240 * 5 * 8
    assert L.smk_mask_rbox_workspace(8, 320, 240) >= 8 * (240 * 160 * 4 + 240 * 5 * 8)
    for bad in ((0, 320, 240), (1, 0, 240), (1, 320, 0), (1, 4097, 240), (1, 320, 4097)):
        assert L.smk_mask_rbox_workspace(*bad) == 0
    one = (np.zeros(1, np.uint8).ctypes.data, 1, 1, 1, 100.0, np.zeros(1, np.uint8).ctypes.data, 1 << 20, np.zeros(12).ctypes.data, None)
    assert L.smk_mask_rbox(None, *one[1:]) == -1 and L.smk_mask_rbox(*one[:4], -1.0, *one[5:]) == -1
