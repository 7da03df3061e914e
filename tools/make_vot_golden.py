#!/usr/bin/env python
"""Generate tests/golden/vot_overlap.npz: inputs for, and the values returned by, the reference's UNCHANGED VOT helpers, run on the
CPU: utils.pyvotkit.region.vot_overlap / vot_float2str (its Cython extension, built by the compatibility shim) and
utils.bbox_helper.get_axis_aligned_bbox.

    python tools/make_vot_golden.py

The reference is imported through tests/compat/shim -- never edited, never copied; this file holds none of its text.  The fixture
keeps what the functions are given and what they return:

  per bounds (W, H) in BOUNDS: p1_<W>x<H>, p2_<W>x<H> float64 [N,8] corner lists, ov_<W>x<H> float32 [N] = the float the
      extension returns for vot_overlap(p1, p2, (W, H)), kind_<W>x<H> int8 [N] = index into KINDS
  probe_*: four hand-made pairs at bounds 64 x 48: a nearby quad, one outside the image, one inside but disjoint, two points
  f2s_values float64 [M], f2s_text [M]: vot_float2str("%.4f", v)
  bbox_regions float64 [R,8], bbox_out float64 [R,4]: get_axis_aligned_bbox

Which return of the reference a pair takes is not visible from outside; the generator classifies the pairs with the bitmap
restatement of the tests (tests/vot_overlap_ref.py), asserts that the restatement agrees with the reference on every pair, and
that every return, a NaN and a small positive overlap occur."""
import os
import sys
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")

from tests.compat import shim  # noqa: E402
import vot_overlap_ref as V  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "vot_overlap.npz")
BOUNDS = ((64, 48), (40, 700))
KINDS = ("rotated", "half_integer", "negative", "axis_edges", "bow_tie", "on_bounds", "touch_column", "disjoint", "outside",
         "point", "sliver", "mixed")
QUAD = [10, 10, 50, 12, 48, 40, 8, 38]


def rot_quad(rng, W, H, n, scale=1.0):
    """n rotated rectangles with centres in and around the image -> [n,8]"""
    cx, cy = rng.uniform(-0.2 * W, 1.2 * W, n), rng.uniform(-0.2 * H, 1.2 * H, n)
    w, h = rng.uniform(2, 0.8 * W * scale, n), rng.uniform(2, 0.8 * H * scale, n)
    a = rng.uniform(0, np.pi, n)
    dx = np.stack([-w, w, w, -w], 1) / 2
    dy = np.stack([-h, -h, h, h], 1) / 2
    x = cx[:, None] + dx * np.cos(a)[:, None] - dy * np.sin(a)[:, None]
    y = cy[:, None] + dx * np.sin(a)[:, None] + dy * np.cos(a)[:, None]
    return np.stack([x, y], 2).reshape(n, 8)


def near(rng, p, amount):
    """p moved and jittered a little: pairs that overlap"""
    return p + rng.uniform(-amount, amount, (p.shape[0], 1, 2)).repeat(4, 1).reshape(-1, 8) + rng.uniform(-1, 1, p.shape)


def rect(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def cases(rng, W, H):
    out = []

    def add(kind, a, b):
        a, b = np.asarray(a, dtype=np.float64).reshape(-1, 8), np.asarray(b, dtype=np.float64).reshape(-1, 8)
        out.append((np.full(a.shape[0], KINDS.index(kind), dtype=np.int8), a, b))

    a = rot_quad(rng, W, H, 60)
    add("rotated", a, near(rng, a, 0.1 * min(W, H)))
    a = np.round(rot_quad(rng, W, H, 40) * 2) / 2                       # .0 and .5: round() half away from zero, both signs
    add("half_integer", a, np.round(near(rng, a, 4) * 2) / 2)
    a = rot_quad(rng, W, H, 30) - np.tile([0.6 * W, 0.5 * H], 4)         # mostly left of / above the image
    add("negative", a, near(rng, a, 3))
    lo = rng.integers(0, [W // 2, H // 2], (30, 2))
    hi = lo + rng.integers(1, [W // 2, H // 2], (30, 2))
    a = np.array([rect(l[0], l[1], h[0], h[1]) for l, h in zip(lo, hi)], dtype=np.float64)
    add("axis_edges", a, a + rng.integers(-3, 4, (30, 1)).astype(np.float64))
    a = rot_quad(rng, W, H, 30)
    bow = a.reshape(-1, 4, 2)[:, [0, 2, 1, 3]].reshape(-1, 8)           # corners out of cyclic order: the edges cross
    add("bow_tie", bow, near(rng, a, 2))
    add("bow_tie", near(rng, a, 2), bow)
    a = np.array([rect(0, 0, W, H), rect(0, 5, W, H - 5), rect(W - 6, 0, W, H), rect(0, 0, 7, H), rect(0, H - 4, W, H),
                  rect(W, 0, W + 9, H), rect(0, H, W, H + 6), rect(-8, 0, 0, H), rect(W - 1, H - 1, W, H)], dtype=np.float64)
    add("on_bounds", a, np.roll(a, 1, axis=0))
    add("on_bounds", a, a)
    for x in (5, W // 2, W - 3):                                        # two boxes that share exactly one pixel column
        add("touch_column", rect(x - 6, 4, x, H - 5), rect(x, 2, x + 7, H - 9))
        add("touch_column", rect(x, 2, x + 7, H - 9), rect(x - 6, 4, x, H - 5))
    add("disjoint", rect(2, 2, W // 3, H // 3), rect(W // 2 + 2, H // 2 + 2, W - 3, H - 3))
    add("disjoint", rect(2, 2, W // 3, H - 2), rect(W // 2, 2, W - 2, H - 2))           # bounding boxes apart in x only
    add("disjoint", [2, 2, W - 4, 2, W - 4, 5, 2, 5], [2, H - 9, W - 4, H - 9, W - 4, H - 3, 2, H - 3])
    add("disjoint", [1, 1, W // 2, 1, 1, H // 2, 1, 1.5], [W - 2, H - 2, W // 2 + 3, H - 2, W - 2, H // 2 + 3, W - 2, H - 3])   # boxes meet, shapes do not
    inside = rot_quad(rng, W, H, 6, 0.5)
    add("outside", inside, inside + np.tile([1.5 * W, 0], 4))
    add("outside", inside - np.tile([0, 1.5 * H], 4), inside)
    add("outside", inside + np.tile([1.5 * W, 1.5 * H], 4), inside - np.tile([1.4 * W, 0], 4))
    add("point", [10.0] * 8, [10.0] * 8)                                # all four vertices equal, both polygons: 0 / 0
    add("point", [10.0] * 8, rect(4, 4, 20, 20))
    add("point", rect(4, 4, 20, 20), [7.5, 9.5] * 4)
    add("point", [W + 20.0, 3.0] * 4, [W + 20.0, 3.0] * 4)
    add("point", [3, 7, 30, 7, 30, 7, 3, 7], rect(2, 2, 33, 12))        # a horizontal segment
    add("point", [9, 2, 9, 2, 9, H - 2, 9, H - 2], rect(2, 2, 33, 12))  # a vertical one
    big = rect(1, 1, W - 1, H - 1)                                      # a large annotation against a sliver: small overlaps
    for k in range(8):
        add("sliver", big, rect(3 + k, 3 + 2 * k, 4 + k, 4 + 2 * k + (k % 3)))
        add("sliver", rect(3 + k, 3 + 2 * k, 5 + k, 3 + 2 * k), big)
    a, b = rot_quad(rng, W, H, 60), rot_quad(rng, W, H, 60)             # unrelated pairs: whatever comes
    add("mixed", a, b)
    kind = np.concatenate([c[0] for c in out])
    return kind, np.concatenate([c[1] for c in out]), np.concatenate([c[2] for c in out])


def main():
    shim.install(os.path.join(shim.REF, "experiments", "siammask_sharp"))
    region = sys.modules["utils.pyvotkit.region"]
    assert region.__smk_kind__ == "built", "the reference's extension could not be built here"
    from utils.bbox_helper import get_axis_aligned_bbox

    def ref(p1, p2, wh):
        as_pts = lambda p: tuple((float(p[2 * k]), float(p[2 * k + 1])) for k in range(4))
        return np.array([region.vot_overlap(as_pts(a), as_pts(b), wh) for a, b in zip(p1, p2)], dtype=np.float32)

    rng = np.random.default_rng(354)
    save = {"kinds": np.array(KINDS)}
    paths, values = [], []
    for W, H in BOUNDS:
        kind, p1, p2 = cases(rng, W, H)
        side = max(W, H)                                                # coordinates stay near the image (a rotated quad of a
        assert min(p1.min(), p2.min()) >= -2 * side and max(p1.max(), p2.max()) <= 3 * side      # tall image is wider than it)
        ov = ref(p1, p2, (W, H))
        mine, counts = V.overlap(p1, p2, W, H)
        assert np.array_equal(V.bits(np.nan_to_num(ov, nan=-1.0)), V.bits(np.nan_to_num(mine, nan=-1.0))), \
            "the bitmap restatement differs from the reference on pairs %s" % np.nonzero(V.bits(ov) != V.bits(mine))[0][:10]
        assert np.array_equal(np.isnan(ov), np.isnan(mine))
        tag = "%dx%d" % (W, H)
        save.update({"p1_" + tag: p1, "p2_" + tag: p2, "ov_" + tag: ov, "kind_" + tag: kind})
        paths.append(counts[:, 3])
        values.append(ov)
        print(tag, len(ov), "pairs; paths", np.bincount(counts[:, 3], minlength=5).tolist(), "NaN", int(np.isnan(ov).sum()),
              "zero", int((ov == 0).sum()))
    paths, values = np.concatenate(paths), np.concatenate(values)
    assert set(paths.tolist()) == {0, 1, 2, 3, 4}, "not every return of the reference is taken: %s" % sorted(set(paths.tolist()))
    assert np.isnan(values).any() and ((values > 0) & (values < 0.01)).any() and (values == 1).any()
    # four hand-made probes
    probes = {"near": [12, 11, 52, 14, 47, 42, 9, 36], "outside": [100, 10, 140, 12, 138, 40, 98, 38],
              "disjoint": [52, 41, 62, 41, 62, 46, 52, 46]}
    for k, p in probes.items():
        save["probe_" + k] = np.array([QUAD, p], dtype=np.float64)
        save["probe_" + k + "_ov"] = ref([QUAD], [p], (64, 48))
    save["probe_point"] = np.full((2, 8), 10.0)
    save["probe_point_ov"] = ref([[10.0] * 8], [[10.0] * 8], (64, 48))
    assert save["probe_outside_ov"][0] == 0 and save["probe_disjoint_ov"][0] == 0 and np.isnan(save["probe_point_ov"][0])
    assert 0 < save["probe_near_ov"][0] < 1
    # vot_float2str and get_axis_aligned_bbox
    vals = np.concatenate([rng.uniform(-500, 900, 40), [0.0, -0.0, 0.00005, 0.00015, 1e-7, 123.45675, 2.5e-5, 16777217.0,
                                                        0.1, 1 / 3, 319.99996, -7.00005]])
    save["f2s_values"] = vals
    save["f2s_text"] = np.array([region.vot_float2str("%.4f", float(v)) for v in vals])
    regions = np.concatenate([rot_quad(rng, 320, 240, 12), [rect(10, 20, 110, 70), rect(0.5, 0.25, 33.75, 90.125)]])
    save["bbox_regions"] = regions
    save["bbox_out"] = np.array([[float(v) for v in get_axis_aligned_bbox(r)] for r in regions], dtype=np.float64)
    np.savez_compressed(OUT, **save)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    print({k: float(save["probe_" + k + "_ov"][0]) for k in ("near", "outside", "disjoint", "point")})


if __name__ == "__main__":
    main()
