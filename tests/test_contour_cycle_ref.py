"""tests/contour_cycle_ref.py (the contour area as a sum over one cycle of the border permutation, what SMK_RBOX_CYCLES computes)
against tests/contour_ref.py (the border followed vertex by vertex), and the host side of the smk_mask_rbox_ex contract."""
import os
import re

import numpy as np
import pytest

import contour_cycle_ref as C
import contour_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def agree(mask, tag):
    """areas and first pixels equal contour_ref's, component by component; the root of every outer cycle is (p0, k0)"""
    want, got = R.components(mask), C.components(mask)
    assert [c["first"] for c in got] == [c["first"] for c in want], tag
    for w, g in zip(want, got):
        assert g["area"] == w["area"], (tag, w["first"], g["area"], w["area"])
        assert g["root_ok"], (tag, w["first"])
    return len(want)


def nested_rings(H=40, W=60):
    m = np.zeros((H, W), np.uint8)
    m[2:38, 3:57] = 1
    m[5:35, 6:54] = 0
    m[9:31, 12:48] = 1                                   # a separate component inside the hole ...
    m[12:28, 15:45] = 0                                  # ... itself a ring
    m[17:23, 22:38] = 1                                  # and a blob in the inner hole
    return m


@pytest.mark.parametrize("recipe", ["noisy", "ellipse"])
def test_seeded_recipes(recipe):
    masks = R.noisy_masks(3) if recipe == "noisy" else R.ellipse_masks(3)
    n = sum(agree(m, "%s %d" % (recipe, i)) for i, m in enumerate(masks))
    assert n >= (300 if recipe == "noisy" else 3)


def test_random_masks():
    rng = np.random.default_rng(20261020)
    n = 0
    for i in range(64):
        density = 0.15 + 0.75 * i / 63
        n += agree((rng.random((24, 40)) < density).astype(np.uint8), "random %d density %.2f" % (i, density))
    assert n > 500


def test_traps():
    checker = (np.indices((16, 16)).sum(0) % 2).astype(np.uint8)
    assert agree(checker, "checkerboard") == 1
    assert agree(nested_rings(), "nested rings") == 3
    assert agree(np.ones((12, 17), np.uint8), "all ones") == 1
    assert C.components(np.ones((12, 17), np.uint8))[0]["area"] == 11 * 16.0
    grid = np.zeros((16, 16), np.uint8)
    grid[::2, ::2] = 1
    assert agree(grid, "isolated pixels") == 64
    assert C.components(np.zeros((4, 4), np.uint8)) == [] and C.cycles(np.zeros((4, 4), np.uint8)) is None
    ring = np.zeros((9, 9), np.uint8)
    ring[2:7, 2:7] = 1
    ring[3:6, 3:6] = 0                                   # one pixel thick: every pixel on the outer and the hole border at once
    assert agree(ring, "thin ring") == 1 and C.components(ring)[0]["area"] == 16.0


def test_the_map_is_a_permutation_of_the_states():
    rng = np.random.default_rng(5)
    m = rng.random((24, 40)) < 0.5
    nb = C.neighbour_bits(m)
    seen = set()
    for y, x in zip(*np.nonzero(m)):
        for k in range(8):
            if (int(nb[y, x]) >> k) & 1:
                d = C.successor_dir(int(nb[y, x]), k)
                seen.add((int(y) + R.CW[d][0], int(x) + R.CW[d][1], (d + 4) % 8))
    assert len(seen) == sum(bin(int(v)).count("1") for v in nb[m])           # injective on a finite set


def test_export_contract():
    from siammask_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "siammask_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", hdr))
    for s in ("smk_mask_rbox_ex", "smk_mask_rbox_workspace_ex"):
        assert s in declared and s in _lib.SYMBOLS, s
    assert re.search(r"#define\s+SMK_RBOX_TRACE\s+0\b", hdr) and re.search(r"#define\s+SMK_RBOX_CYCLES\s+1\b", hdr)
    assert "smk_test_mask_rbox_paths" in _lib.SYMBOLS and "smk_test_mask_rbox_paths" not in declared
    L = _lib.lib()
    assert L.smk_version() == (1 << 16) | 10
    states = 4 * (1 << 22)
    for B, W, H in ((1, 320, 240), (8, 320, 240), (8, 1280, 720), (3, 1, 1), (2, 4096, 4096), (64, 40, 24)):
        w0 = L.smk_mask_rbox_workspace(B, W, H)
        assert L.smk_mask_rbox_workspace_ex(B, W, H, 0) == w0 > 0
        w1 = L.smk_mask_rbox_workspace_ex(B, W, H, 1)
        assert w0 + B * H * ((W + 1) // 2) * 8 < w1 <= 3 * w0 + B * min(states, 32 * W * H) + 256, (B, W, H, w0, w1)
    for bad in ((0, 320, 240, 1), (1, 0, 240, 1), (1, 320, 4097, 1), (1, 320, 240, 2), (1, 320, 240, -1)):
        assert L.smk_mask_rbox_workspace_ex(*bad) == 0, bad
    # host-side refusals need no device
    buf = np.zeros(1 << 12, np.uint8)
    one = [np.zeros(1, np.uint8).ctypes.data, 1, 1, 1, 100.0, 1, buf.ctypes.data, buf.size, np.zeros(12).ctypes.data, None]
    for i, v in ((5, 2), (5, -1), (0, None), (4, -1.0), (7, L.smk_mask_rbox_workspace_ex(1, 1, 1, 1) - 1)):
        args = list(one)
        args[i] = v
        assert L.smk_mask_rbox_ex(*args) == -1, (i, v)
    assert L.smk_test_mask_rbox_paths(buf.ctypes.data, 1, 1, 1, 0, np.zeros(1, np.int32).ctypes.data) == -1
