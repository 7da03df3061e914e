"""Brute-force restatement of the VOT polygon overlap (tools/test.py:354 vot_overlap -> utils/pyvotkit region.c:848-945, non-legacy
rasterisation) in numpy, for N pairs of 4-vertex polygons at once: both masks of the joint window are MATERIALISED as boolean
arrays, painted row by row from the sorted nodes as the fill loop does, and counted.  The guard for the interval arithmetic of
csrc/vot_overlap.h, which never stores a mask.  float32 where the reference has float, float64 where it has double."""
import numpy as np

F32_MAX = np.float32(3.402823466e+38)
PATH_RASTER, PATH_RATIO_12, PATH_RATIO_21, PATH_SIZE, PATH_BOUNDS = 0, 1, 2, 3, 4


def _min(a, b):
    return np.where(a < b, a, b)


def _max(a, b):
    return np.where(a > b, a, b)


def _round_away(x):
    """C round() of float32 values, through float64 (exact), back to float32"""
    x = x.astype(np.float64)
    return np.trunc(x + np.copysign(0.5, x)).astype(np.float32)


def _bounds(px, py, im_w, im_h):
    """compute_bounds -> bounds_round -> bounds_intersection with the image -> top, bottom, left, right (float32 [N])"""
    n = px.shape[0]
    top, bottom = np.full(n, F32_MAX), np.full(n, -F32_MAX)
    left, right = np.full(n, F32_MAX), np.full(n, -F32_MAX)
    for k in range(4):
        top, bottom = _min(top, py[:, k]), _max(bottom, py[:, k])
        left, right = _min(left, px[:, k]), _max(right, px[:, k])
    top, bottom, left, right = np.floor(top), np.ceil(bottom), np.floor(left), np.ceil(right)
    zero = np.float32(0)
    return _max(top, zero), _min(bottom, np.float32(im_h)), _max(left, zero), _min(right, np.float32(im_w))


def _paint(px, py, width, rows, cols):
    """rasterize_polygon (non-legacy) of N placed polygons into a boolean [N, rows, cols]; width [N] is each pair's own"""
    n = px.shape[0]
    mask = np.zeros((n, rows, cols), dtype=bool)
    col = np.arange(cols)[None, :]
    iy = py.astype(np.int64)
    big = np.int64(1) << 40
    for Y in range(rows):
        nodes = np.full((n, 4), big)
        for i in range(4):
            j = (i + 3) % 4
            yi, yj = iy[:, i], iy[:, j]
            hit = (((yi <= Y) & (yj > Y)) | ((yj <= Y) & (yi > Y)) | ((yi < Y) & (yj >= Y)) | ((yj < Y) & (yi >= Y)) |
                   ((yi == yj) & (yi == Y)))
            r = (py[:, j] - py[:, i]).astype(np.float64)
            k = (px[:, j] - px[:, i]).astype(np.float64)
            hit &= r != 0
            with np.errstate(all="ignore"):
                v = px[:, i].astype(np.float64) + (np.float32(Y) - py[:, i]).astype(np.float64) / r * k
            nodes[:, i] = np.where(hit, np.trunc(np.where(hit, v, 0.0)).astype(np.int64), big)
        nodes.sort(axis=1)
        cnt = (nodes < big).sum(axis=1)
        i = np.zeros(n, dtype=np.int64)
        stop = np.zeros(n, dtype=bool)
        ar = np.arange(n)
        for _ in range(3):
            act = ~stop & (i < cnt - 1)
            a = nodes[ar, np.minimum(i, 3)]
            b = nodes[ar, np.minimum(i + 1, 3)]
            same = act & (a == b)
            brk = act & ~same & (a >= width)
            fill = act & ~same & ~brk
            lo, hi = np.maximum(a, 0), np.minimum(b, width - 1)
            paint = (fill & (b >= 0))[:, None] & (col >= lo[:, None]) & (col <= hi[:, None])
            mask[:, Y, :] |= paint
            stop |= brk
            i = i + np.where(same, 1, np.where(fill, 2, 0))
    return mask


def overlap(p1, p2, im_w, im_h):
    """p1, p2: float64 [N,8] corners -> (overlap float32 [N], counts int32 [N,4] = only1, only2, inter, path)"""
    p1 = np.asarray(p1, dtype=np.float64).reshape(-1, 8).astype(np.float32)
    p2 = np.asarray(p2, dtype=np.float64).reshape(-1, 8).astype(np.float32)
    n = p1.shape[0]
    x1, y1, x2, y2 = p1[:, 0::2], p1[:, 1::2], p2[:, 0::2], p2[:, 1::2]
    t1, b1, l1, r1 = _bounds(x1, y1, im_w, im_h)
    t2, b2, l2, r2 = _bounds(x2, y2, im_w, im_h)
    with np.errstate(all="ignore"):
        ox, oy = _min(l1, l2), _min(t1, t2)
        width = np.trunc((_max(r1, r2) - ox).astype(np.float64)).astype(np.int64) + 1
        height = np.trunc((_max(b1, b2) - oy).astype(np.float64)).astype(np.int64) + 1
        a1 = ((r1 - l1) * (b1 - t1)).astype(np.float64)
        a2 = ((r2 - l2) * (b2 - t2)).astype(np.float64)
        it, ib, il, ir = _max(t1, t2), _min(b1, b2), _max(l1, l2), _min(r1, r2)
        inter = (ir - il) * (ib - it)
        bo = inter / ((((r1 - l1) * (b1 - t1)) + ((r2 - l2) * (b2 - t2))) - inter)
        bo = np.where(np.float32(0) > bo, np.float32(0), bo)
        path = np.select([a1 / a2 < 1e-10, a2 / a1 < 1e-10, (width < 1) | (height < 1), bo == 0],
                         [PATH_RATIO_12, PATH_RATIO_21, PATH_SIZE, PATH_BOUNDS], PATH_RASTER)
    out = np.zeros(n, dtype=np.float32)
    counts = np.zeros((n, 4), dtype=np.int32)
    counts[:, 3] = path
    go = np.nonzero(path == PATH_RASTER)[0]
    if go.size:
        w, h = width[go], height[go]
        rows, cols = int(h.max()), int(w.max())
        q = []
        for px, py in ((x1, y1), (x2, y2)):
            q.append((_round_away(px[go] + (-ox[go])[:, None]), _round_away(py[go] + (-oy[go])[:, None])))
        inside = np.arange(rows)[None, :, None] < h[:, None, None]     # a pair's own rows; its columns are clamped to its width
        m1 = _paint(q[0][0], q[0][1], w, rows, cols) & inside
        m2 = _paint(q[1][0], q[1][1], w, rows, cols) & inside
        both = (m1 & m2).sum(axis=(1, 2))
        only1 = (m1 & ~m2).sum(axis=(1, 2))
        only2 = (m2 & ~m1).sum(axis=(1, 2))
        counts[go, 0], counts[go, 1], counts[go, 2] = only1, only2, both
        with np.errstate(all="ignore"):
            out[go] = both.astype(np.float32) / (only1 + only2 + both).astype(np.float32)
    return out, counts


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
