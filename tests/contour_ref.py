"""numpy / scipy restatement of the rotated-box stage of the tracker (tools/test.py:283-300 of the reference: cv2.findContours
RETR_EXTERNAL / CHAIN_APPROX_NONE -> largest cv2.contourArea -> cv2.minAreaRect -> cv2.boxPoints), as include/siammask_hip.h
states it for smk_mask_rbox.  Test infrastructure: tests/test_contour_ref.py pins it (closed forms, the polygons the unchanged
tool returned, an independent calipers implementation); tests/test_gpu_rbox.py compares the device against it.

Pixel (x, y) is the lattice point (x, y); a pixel is set when its value is non-zero.
  components : 8-connected components of the set pixels
  contour    : outer border of a component followed from its first raster pixel (Suzuki-Abe, 8-neighbour; every visit of a
               border pixel is a vertex, so a one-pixel spur is walked out and back)
  area       : 1/2 |sum x_i y_{i+1} - x_{i+1} y_i| over that closed vertex list
  selection  : largest area, on equal areas the component whose first raster pixel comes first; found = area > min_area
  rectangle  : minimum-area enclosing rectangle of the convex hull (monotone chain, rotating calipers in float64)"""
import numpy as np
from scipy import ndimage

# neighbours clockwise on the screen (y down) from west: W NW N NE E SE S SW, as (dy, dx)
CW = [(0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1)]


def outer_border(m, i, j):
    """m: bool array that holds ONE component (plus anything not connected to it); (i, j) = (row, column) of its first raster
    pixel.  -> list of (x, y) vertices"""
    H, W = m.shape
    g = np.zeros((H + 2, W + 2), bool)
    g[1:-1, 1:-1] = m
    i, j = i + 1, j + 1
    first = None
    for s in range(8):                                   # clockwise from west (step 3.1)
        d = CW[s]
        if g[i + d[0], j + d[1]]:
            first = (i + d[0], j + d[1])
            break
    if first is None:
        return [(j - 1, i - 1)]
    pts = []
    p2, p3 = first, (i, j)
    cap = 4 * H * W + 4
    while len(pts) < cap:
        k = CW.index((p2[0] - p3[0], p2[1] - p3[1]))
        for s in range(1, 9):                            # counter-clockwise, the previous pixel itself last (step 3.3)
            d = CW[(k - s) % 8]
            q = (p3[0] + d[0], p3[1] + d[1])
            if g[q]:
                p4 = q
                break
        pts.append((p3[1] - 1, p3[0] - 1))
        if p4 == (i, j) and p3 == first:
            return pts
        p2, p3 = p3, p4
    raise AssertionError("border following did not close")


def contour_area(pts):
    """shoelace over the closed vertex list, in exact integer arithmetic -> a multiple of 1/2"""
    p = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    return abs(int(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))) / 2.0


def components(mask):
    """-> list of dicts (first = (x, y) of the first raster pixel, pts = contour vertices, area), in raster order of `first`"""
    m = np.asarray(mask) != 0
    lab, n = ndimage.label(m, structure=np.ones((3, 3), int))
    out = []
    for c, sl in enumerate(ndimage.find_objects(lab), start=1):
        sub = lab[sl] == c
        j = int(np.argmax(sub[0]))                       # the slice starts at the component's first row
        pts = [(x + sl[1].start, y + sl[0].start) for x, y in outer_border(sub, 0, j)]
        out.append({"first": (j + sl[1].start, sl[0].start), "pts": pts, "area": contour_area(pts)})
    out.sort(key=lambda c: (c["first"][1], c["first"][0]))
    return out


def convex_hull(pts):
    """Andrew's monotone chain, strictly convex (no collinear vertices) -> int64 [n, 2]"""
    p = sorted(set(map(tuple, pts)))
    if len(p) < 3:
        return np.array(p, dtype=np.int64).reshape(-1, 2)

    def cr(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lo = []
    for q in p:
        while len(lo) >= 2 and cr(lo[-2], lo[-1], q) <= 0:
            lo.pop()
        lo.append(q)
    up = []
    for q in reversed(p):
        while len(up) >= 2 and cr(up[-2], up[-1], q) <= 0:
            up.pop()
        up.append(q)
    return np.array(lo[:-1] + up[:-1], dtype=np.int64)


def min_area_rect(hull):
    """rotating calipers over every hull edge in float64 -> (corners [4, 2] in cyclic order, candidates [n, 2] = area and
    direction modulo a quarter turn of the rectangle on each edge)"""
    h = np.asarray(hull, dtype=np.float64).reshape(-1, 2)
    if len(h) == 1:
        return np.repeat(h, 4, axis=0), np.zeros((1, 2))
    best, cand = None, []
    for i in range(len(h)):
        e = h[(i + 1) % len(h)] - h[i]
        u = e / np.hypot(e[0], e[1])
        v = np.array([-u[1], u[0]])
        pu, pv = h @ u, h @ v
        a = (pu.max() - pu.min()) * (pv.max() - pv.min())
        cand.append((a, np.arctan2(u[1], u[0]) % (np.pi / 2)))
        if best is None or a < best[0]:
            best = (a, np.stack([u * pu.min() + v * pv.min(), u * pu.max() + v * pv.min(),
                                 u * pu.max() + v * pv.max(), u * pu.min() + v * pv.max()]))
    return best[1], np.array(cand)


def distinct_rect_gap(cand):
    """relative gap between the smallest candidate area and the smallest area of a DIFFERENT rectangle (hull edges that are
    parallel or perpendicular to the best one give the same rectangle); inf when there is no other"""
    c = np.asarray(cand, dtype=np.float64).reshape(-1, 2)
    k = int(np.argmin(c[:, 0]))
    dd = np.abs(c[:, 1] - c[k, 1])
    other = np.minimum(dd, np.pi / 2 - dd) > 1e-9
    if not other.any():
        return float("inf")
    return float((c[other, 0].min() - c[k, 0]) / max(c[k, 0], 1.0))


def mask_rbox(mask, min_area=100.0):
    """what smk_mask_rbox returns for one mask, plus the margins a test asserts on its inputs.
    -> dict(corners [4,2] float64, area, found, n_components, n_hull, margin, rect_gap)"""
    comps = components(mask)
    if not comps:
        return {"corners": np.zeros((4, 2)), "area": 0.0, "found": 0, "n_components": 0, "n_hull": 0,
                "margin": float("inf"), "rect_gap": float("inf")}
    areas = [c["area"] for c in comps]
    k = int(np.argmax(areas))                            # the first of equal maxima = the earlier first raster pixel
    rest = areas[:k] + areas[k + 1:]
    hull = convex_hull(comps[k]["pts"])
    corners, cand = min_area_rect(hull)
    return {"corners": corners, "area": areas[k], "found": int(areas[k] > min_area), "n_components": len(comps),
            "n_hull": len(hull), "margin": areas[k] - max(rest) if rest else float("inf"),
            "rect_gap": distinct_rect_gap(cand)}


def corner_set_distance(a, b):
    """largest coordinate difference between two rectangles given as four corners in cyclic order, minimised over the four
    starting corners and the two directions"""
    a = np.asarray(a, dtype=np.float64).reshape(4, 2)
    b = np.asarray(b, dtype=np.float64).reshape(4, 2)
    best = np.inf
    for bb in (b, b[::-1]):
        for r in range(4):
            best = min(best, float(np.abs(a - np.roll(bb, r, axis=0)).max()))
    return best


# ---- the seeded recipes the tests share --------------------------------------------------------
def _ellipse(xx, yy, cx, cy, a, b, th):
    u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
    v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
    return (u / a) ** 2 + (v / b) ** 2 <= 1


def ellipse_masks(n=64, seed=20261016, H=240, W=320):
    """n rotated ellipses, one per mask -> uint8 [n, H, W]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        cx, cy = rng.uniform(80, 240), rng.uniform(70, 170)
        a, b = rng.uniform(20, 60), rng.uniform(8, 30)
        th = rng.uniform(0, np.pi)
        out[i] = _ellipse(xx, yy, cx, cy, a, b, th)
    return out


def noisy_masks(n=16, seed=7, H=240, W=320):
    """three ellipses OR-ed together plus salt noise (123-168 components per mask) -> uint8 [n, H, W]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for t in range(n):
        m = np.zeros((H, W), np.uint8)
        for _ in range(3):
            cx, cy = rng.uniform(40, 280), rng.uniform(40, 200)
            a, b = rng.uniform(10, 50), rng.uniform(5, 25)
            th = rng.uniform(0, np.pi)
            m |= _ellipse(xx, yy, cx, cy, a, b, th).astype(np.uint8)
        m |= (rng.random((H, W)) < 0.002).astype(np.uint8)
        out[t] = m
    return out
