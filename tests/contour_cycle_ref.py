"""numpy restatement of the cycle form of the contour area (smk_mask_rbox_ex with SMK_RBOX_CYCLES, mask_rbox_cycles.hip).
Test infrastructure: tests/test_contour_cycle_ref.py pins it against contour_ref.components.

The border rule of contour_ref.outer_border is a map on states (p, k): p a set pixel, k a direction in which p has a set
neighbour.  The next direction d is the first set neighbour of p counter-clockwise from k, k itself last; the next state is
(p + dir(d), (d + 4) % 8).  For a fixed p every set direction goes to its cyclic successor, so the map is a permutation of the
states.  The trace of a component starts in (p0, k0) -- its first raster pixel, the lowest set direction -- and stops when it is
about to re-enter that state: 2 * area = |sum over the cycle of (p0, k0) of x y' - x' y|.

  states    : numbered ((y - y0) * bw + (x - x0)) * 8 + k inside the bounding rectangle of the set pixels; only border pixels
              (fewer than 8 set neighbours, the frame edge counting as zero) own states
  links     : s ~ successor(s), dropped when the successor's pixel is interior
  roots     : union-by-minimum, so the root of a class is its smallest state
  sums      : per root, the integer cross terms of its states"""
import numpy as np
from scipy import ndimage

from contour_ref import CW


def neighbour_bits(m):
    """bit k of out[y, x] = the neighbour of (x, y) in direction CW[k] is set (0 outside the array)"""
    H, W = m.shape
    g = np.zeros((H + 2, W + 2), bool)
    g[1:-1, 1:-1] = m
    out = np.zeros((H, W), np.int64)
    for k, (dy, dx) in enumerate(CW):
        out |= g[1 + dy:1 + dy + H, 1 + dx:1 + dx + W].astype(np.int64) << k
    return out


def successor_dir(nb, k):
    for s in range(1, 9):
        d = (k - s) % 8
        if (nb >> d) & 1:
            return d
    raise AssertionError("a state without a set neighbour")


def cycles(mask):
    """-> dict(rect = (x0, y0, bw, bh), root = {state: root state}, sums = {root state: sum of x y' - x' y over its states}),
    or None for a mask without set pixels"""
    m = np.asarray(mask) != 0
    if not m.any():
        return None
    ys, xs = np.nonzero(m)
    x0, y0, bw, bh = int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)
    sub = m[y0:y0 + bh, x0:x0 + bw]
    nb = neighbour_bits(sub)
    border = sub & (nb != 0xff)
    parent, term = {}, {}
    links = []
    for y, x in zip(*np.nonzero(border)):
        n = int(nb[y, x])
        for k in range(8):
            if not (n >> k) & 1:
                continue
            s = (int(y) * bw + int(x)) * 8 + k
            parent[s] = s
            d = successor_dir(n, k)
            y4, x4 = int(y) + CW[d][0], int(x) + CW[d][1]
            term[s] = (int(x) + x0) * (y4 + y0) - (x4 + x0) * (int(y) + y0)
            if nb[y4, x4] != 0xff:                       # a link into an interior pixel is dropped
                links.append((s, (y4 * bw + x4) * 8 + (d + 4) % 8))

    def find(s):
        while parent[s] != s:
            parent[s] = parent[parent[s]]
            s = parent[s]
        return s
    for a, b in links:
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = {s: find(s) for s in parent}
    sums = {}
    for s, r in root.items():
        sums[r] = sums.get(r, 0) + term[s]
    return {"rect": (x0, y0, bw, bh), "root": root, "sums": sums}


def components(mask):
    """what contour_ref.components returns without the vertex lists, computed from the cycles: list of dicts (first = (x, y) of
    the first raster pixel, area, root_ok: the root of the component's outer cycle is the state (p0, k0)), in raster order"""
    m = np.asarray(mask) != 0
    c = cycles(m)
    if c is None:
        return []
    x0, y0, bw, bh = c["rect"]
    nb = neighbour_bits(m[y0:y0 + bh, x0:x0 + bw])
    lab, n = ndimage.label(m, structure=np.ones((3, 3), int))
    out = []
    for k, sl in enumerate(ndimage.find_objects(lab), start=1):
        y = sl[0].start
        x = sl[1].start + int(np.argmax(lab[sl][0] == k))
        n0 = int(nb[y - y0, x - x0])
        if n0 == 0:                                      # a pixel without neighbours: no state, area 0
            out.append({"first": (x, y), "area": 0.0, "root_ok": True})
            continue
        s0 = ((y - y0) * bw + (x - x0)) * 8 + (n0 & -n0).bit_length() - 1
        out.append({"first": (x, y), "area": abs(c["sums"].get(s0, 0)) / 2.0, "root_ok": c["root"].get(s0) == s0})
    out.sort(key=lambda d: (d["first"][1], d["first"][0]))
    return out
