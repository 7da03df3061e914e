"""COCO run-length codes on the host (data/coco/pycocotools/common/maskApi.c), numpy only: what a caller does with the counts
the device wrote (smk_rle_encode / smk_paste_rle_dev, DeviceTracker.run(rle=)).

counts: the run lengths of an h x w mask read column-major (j = x * h + y), alternating unset / set and starting with the unset
run (0 when pixel 0 is set); they sum to h * w.  An empty mask is [h * w], a full one [0, h * w].

    r = tr.run(frames, rle=True)['rle']                 # counts on the device, n / area on the host
    per = rle.to_host(r)                                # ONE copy of counts[..., :n.max()] -> [T][B] numpy arrays (None: n > cap)
    rle.to_coco(per[t][b], *r['size'])                  # {'size': [h, w], 'counts': b'...'}: what pycocotools takes

Streams with their own frame sizes (dataset.run_videos): r['sizes'] [T,B,2] = (h, w) per frame and stream stands for r['size'], and
to_host_v(r) is to_host with None also where n == 0 (the slot had no video that step).

The fused label map of a VOS frame as one code per object (smk_vos_rle / smk_labels_rle_encode, run(vos={..., 'rle': True})):
plane o is labels == o + 1, so the planes are disjoint and a frame's map is their union.

    r = tr.run(frames, vos={'object_ids': ids, 'rle': True, ...})['label_rle']      # the layout of res['rle'], B = the objects
    per = rle.to_host(r)
    rle.labels_decode(per[t], *r['size'])               # uint8 [h, w] label map of frame t
    rle.labels_to_coco(per[t], *r['size'], object_ids=ids)      # [{'size', 'counts', 'label', 'object_id'}] of the non-empty planes
"""
import numpy as np


def default_cap(H, W):
    """counts per stream the tracker reserves: 8 W + 2 = four set runs per column (eight counts, a blob with one concavity -- a
    'U' or a ring -- cuts a column into that many) plus the leading and the trailing count, and never more than the H W + 1 a
    mask can have.  A mask with more runs is reported through n > cap, not truncated silently."""
    return min(int(H) * int(W) + 1, 8 * int(W) + 2)


def _counts(counts):
    c = np.asarray(counts)
    if c.ndim != 1 or c.size < 1 or c.dtype.kind not in "iu":
        raise ValueError("counts must be a 1-D integer array with at least one entry")
    return c.astype(np.int64)


def to_string(counts):
    """rleToString: each count -- from the fourth on, its difference to the count two places back -- as a little-endian sequence
    of 5-bit groups, bit 5 = 'more follows', offset 48; the last group carries the sign in its bit 4"""
    c = _counts(counts)
    d = c.copy()
    d[3:] -= c[1:-2]                                                  # (i > 2: the same kind of run, usually of similar length)
    out = bytearray()
    for x in d.tolist():
        while True:
            g = x & 0x1F
            x >>= 5                                                   # arithmetic: -1 stays -1
            more = x != (-1 if g & 0x10 else 0)
            out.append(48 + (g | 0x20 if more else g))
            if not more:
                break
    return bytes(out)


def from_string(s):
    """rleFrString: the counts of to_string's bytes (str is taken as ASCII) -> int64 array"""
    if isinstance(s, str):
        s = s.encode("ascii")
    out, p, n = [], 0, len(s)
    while p < n:
        x, k = 0, 0
        while True:
            if p >= n:
                raise ValueError("rle string ends inside a number")
            g = s[p] - 48
            p += 1
            x |= (g & 0x1F) << (5 * k)
            k += 1
            if not g & 0x20:
                if g & 0x10:
                    x -= 1 << (5 * k)                                 # sign extension
                break
        if len(out) > 2:
            x += out[-2]
        out.append(x)
    return np.asarray(out, dtype=np.int64)


def decode(counts, h, w):
    """rleDecode -> uint8 [h, w] of 0 / 1"""
    c = _counts(counts)
    if int(c.sum()) != int(h) * int(w) or (c < 0).any():
        raise ValueError("counts sum to %d, the mask has %d pixels" % (int(c.sum()), int(h) * int(w)))
    v = np.zeros(c.size, dtype=np.uint8)
    v[1::2] = 1
    return np.ascontiguousarray(np.repeat(v, c).reshape(int(w), int(h)).T)


def area(counts):
    """rleArea: the set pixels"""
    return int(_counts(counts)[1::2].sum())


def to_bbox(counts, h, w):
    """rleToBbox's arithmetic -> float64 (x, y, w, h): the extremes over the FIRST and the LAST pixel of every set run (a run
    that wraps into the next column contributes only those two pixels, as there); zeros for a mask without a set run"""
    c = _counts(counts)
    m = c.size // 2 * 2
    if m == 0:
        return np.zeros(4)
    t = np.cumsum(c[:m]) - (np.arange(m) % 2)
    y = t % int(h)
    x = (t - y) // int(h)
    return np.array([x.min(), y.min(), x.max() - x.min() + 1, y.max() - y.min() + 1], dtype=np.float64)


def to_coco(counts, h, w):
    """the dict pycocotools' mask API takes"""
    return {"size": [int(h), int(w)], "counts": to_string(counts)}


def labels_decode(per_object_counts, h, w):
    """the label map of O per-object codes (plane o = labels == o + 1) -> uint8 [h, w]; ValueError where two planes overlap"""
    out = np.zeros((int(h), int(w)), dtype=np.uint8)
    if len(per_object_counts) > 255:
        raise ValueError("a uint8 label map holds up to 255 objects, got %d" % len(per_object_counts))
    for o, c in enumerate(per_object_counts):
        m = decode(c, h, w) != 0
        if out[m].any():
            raise ValueError("the planes of objects %d and %d overlap" % (int(out[m].max()) - 1, o))
        out[m] = o + 1
    return out


def labels_to_coco(per_object_counts, h, w, object_ids=None):
    """one to_coco dict per NON-EMPTY plane, with 'label' = o + 1 (the value in the label map) and, given object_ids, 'object_id'
    = object_ids[o] (the dataset's id of the object on stream o)"""
    if object_ids is not None and len(object_ids) != len(per_object_counts):
        raise ValueError("%d object_ids for %d planes" % (len(object_ids), len(per_object_counts)))
    out = []
    for o, c in enumerate(per_object_counts):
        if area(c) == 0:
            continue
        d = dict(to_coco(c, h, w), label=o + 1)
        if object_ids is not None:
            d["object_id"] = int(object_ids[o])
        out.append(d)
    return out


def to_host(r):
    """res['rle'] of DeviceTracker.collect() / run() -> a list [T][B] of int64 count arrays, None where the stream's n exceeded
    cap (its counts are incomplete).  One device -> host copy, of counts[..., :min(n.max(), cap)]."""
    n, cap = np.asarray(r["n"]), int(r["cap"])
    T, B = n.shape
    if T == 0:
        return []
    k = int(min(n.max(), cap))
    host = r["counts"][..., :k].cpu().numpy().view(np.uint32)
    return [[host[t, b, :n[t, b]].astype(np.int64) if n[t, b] <= cap else None for b in range(B)] for t in range(T)]


def to_host_v(r):
    """to_host for the res['rle'] of streams with their own sizes (dataset.run_videos; 'sizes' int32 [T,B,2] = (h, w) per frame and
    stream in place of 'size'): None also where n == 0 -- the slot had no video that step, nothing was encoded.  The code of
    (t, b) is that of an h x w mask with (h, w) = r['sizes'][t, b]: to_coco(per[t][b], *r['sizes'][t, b])."""
    n, cap = np.asarray(r["n"]), int(r["cap"])
    T, B = n.shape
    if T == 0:
        return []
    k = int(min(n.max(), cap))
    host = r["counts"][..., :k]
    host = (host if isinstance(host, np.ndarray) else host.cpu().numpy()).view(np.uint32)
    return [[host[t, b, :n[t, b]].astype(np.int64) if 0 < n[t, b] <= cap else None for b in range(B)] for t in range(T)]
