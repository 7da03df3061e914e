"""Numpy restatement of the VOT evaluation in the order csrc/vot_eval.h fixes: the value a "%.4f" result line
parses back to, the two per-frame overlaps (through the bitmap restatement tests/vot_overlap_ref.py), the fragments found from the
codes, the expected-overlap curve with every sum sequential in float64, and the EAO.  Pure Python / numpy; the guard for the
host entries and the kernels, which must equal it bit for bit.

The frames of the V videos are concatenated: offsets [V+1], wh [V,2]; code [G,N] int8 (-1 tracked, 1 init, 2 lost, 0 skipped),
poly [G,N,8] float64, gt [N,8] float64 (gt[n,0] NaN: an annotation row of one value)."""
import numpy as np

import vot_overlap_ref as V

TRACKED, SKIPPED, INIT, LOST = -1, 0, 1, 2
INNER, LAST, WHOLE = 0, 1, 2


def quantise(x):
    """float('%.4f' % float32(x)) without a string: exact, see csrc/vot_eval.h"""
    return np.rint(np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64) * 1e4) / 1e4


def burnin_mask(code_row, offsets, burnin):
    """bool [N]: the frames i .. i + burnin - 1 of its own video behind every init frame i"""
    mask = np.zeros(len(code_row), dtype=bool)
    for v in range(len(offsets) - 1):
        a, b = int(offsets[v]), int(offsets[v + 1])
        for i in np.nonzero(code_row[a:b] == INIT)[0]:
            mask[a + i:min(a + i + burnin, b)] = True
    return mask


def overlaps(code, poly, gt, offsets, wh, burnin=10, quantised=True):
    """-> ov_eao, ov_ar float32 [G,N]: bounds (w - 1, h - 1) without burn-in, bounds (w, h) with it; NaN where not tracked"""
    code, poly, gt = np.asarray(code), np.asarray(poly, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    G, N = code.shape
    ov_eao, ov_ar = np.full((G, N), np.nan, dtype=np.float32), np.full((G, N), np.nan, dtype=np.float32)
    pred = quantise(poly) if quantised else poly
    for g in range(G):
        burn = burnin_mask(code[g], offsets, burnin)
        for v in range(len(offsets) - 1):
            a, b = int(offsets[v]), int(offsets[v + 1])
            w, h = int(wh[v][0]), int(wh[v][1])
            on = np.nonzero((code[g, a:b] == TRACKED) & ~np.isnan(gt[a:b, 0]))[0] + a
            if on.size:
                ov_eao[g, on] = V.overlap(pred[g, on], gt[on], w - 1, h - 1)[0]     # the prediction is polygon 1
                keep = on[~burn[on]]
                if keep.size:
                    ov_ar[g, keep] = V.overlap(pred[g, keep], gt[keep], w, h)[0]
    return ov_eao, ov_ar


def fragments(code_row, offsets, skipping=5):
    """-> [(first frame in the concatenation, length, kind, video)], weights float64 [F], in video order then position"""
    frags, weights = [], []
    for v in range(len(offsets) - 1):
        a, T = int(offsets[v]), int(offsets[v + 1] - offsets[v])
        failures = [int(t) for t in np.nonzero(code_row[a:a + T] == LOST)[0]]
        if not failures:
            frags.append((a, T, WHOLE, v))
            weights.append(float(T) / float(T))
            continue
        p = 0
        for q in [x + skipping for x in failures if x + skipping <= T]:
            end = min(q + 1, T)
            frags.append((a + p, end - p, INNER, v))
            weights.append(float(end - p) / float(q - p + 1))
            p = q
        frags.append((a + p, T - p, LAST, v))
        weights.append(float(T - p) / (float(T - p) + 1e-16))
    return frags, np.array(weights, dtype=np.float64)


def fragment_matrix(ov_row, frags, max_len):
    """the padded matrix the fragments stand for, float64 [F,max_len]"""
    m = np.full((len(frags), max_len), np.nan)
    for f, (start, ln, kind, _) in enumerate(frags):
        vals = np.asarray(ov_row[start:start + ln], dtype=np.float64)
        if kind == INNER:
            m[f, :] = 0.0
        m[f, :ln] = vals if kind == WHOLE else np.where(np.isnan(vals), 0.0, vals)
    return m


def curve(ov_row, frags, weights, max_len):
    """float32 [max_len]: prefix sums sequential over j (np.cumsum), numerator / denominator sequential over the fragments, the
    division by i before the multiplication by the weight, one rounding at the end"""
    m = fragment_matrix(ov_row, frags, max_len)
    idx = np.arange(max_len, dtype=np.float64)
    num, den, some = np.zeros(max_len), np.zeros(max_len), np.zeros(max_len, dtype=bool)
    with np.errstate(all="ignore"):
        for f in range(len(frags)):
            valid = ~np.isnan(m[f])
            valid[0] = False
            body = m[f].copy()
            body[0] = 0.0                                               # the sums start at j = 1
            pre = np.cumsum(body)
            num[valid] = num[valid] + pre[valid] / idx[valid] * weights[f]
            den[valid] = den[valid] + weights[f]
            some |= valid
        out = np.zeros(max_len, dtype=np.float32)
        out[some] = (num[some] / den[some]).astype(np.float32)
    out[0] = 1
    return out


def eao(curve_row, low, high):
    """sequential float64 sum over i ascending of curve[low - 1 : high] without its NaNs, over their number"""
    s, n = 0.0, 0
    for e in np.asarray(curve_row)[low - 1:high]:
        if not np.isnan(e):
            s += float(e)
            n += 1
    return s / n if n else float("nan")


def evaluate(code, ov_eao, offsets, skipping, low, high):
    """-> curve float32 [G,max_len], eao float64 [G], n_fragments [G], per tracker (frags, weights)"""
    code, offsets = np.asarray(code), np.asarray(offsets)
    max_len = int(np.diff(offsets).max())
    curves, eaos, parts = [], [], []
    for g in range(code.shape[0]):
        fr, w = fragments(code[g], offsets, skipping)
        c = curve(ov_eao[g], fr, w, max_len)
        curves.append(c)
        eaos.append(eao(c, low, high))
        parts.append((fr, w))
    return np.stack(curves), np.array(eaos, dtype=np.float64), np.array([len(p[0]) for p in parts]), parts


def random_dataset(seed, V, G, t_min=2, t_max=70, skipping=5, all_codes=None, sizes=None):
    """seeded trajectories of the supervised protocol on V videos of t_min..t_max frames: rotated boxes as annotations, their
    perturbation as predictions (some across the right / bottom edge, some "%.4f" ties), failures at random frames.
    all_codes: the index of a video without a tracked frame; sizes: (w, h) of the first videos.  -> dict(offsets, wh, gt, code, polygon)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(t_min, t_max + 1, V)
    wh = np.stack([rng.integers(2, 200, V), rng.integers(2, 150, V)], 1).astype(np.int32)
    for v, size in enumerate(sizes or ()):
        wh[v] = size
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    N = int(offsets[-1])
    gt, code = np.zeros((N, 8)), np.full((G, N), TRACKED, dtype=np.int8)
    for v in range(V):
        a, T = int(offsets[v]), int(lens[v])
        w, h = float(wh[v, 0]), float(wh[v, 1])
        cx, cy = rng.uniform(0.2 * w, 1.05 * w, T), rng.uniform(0.2 * h, 1.05 * h, T)
        bw, bh, ang = rng.uniform(1, 0.6 * w + 1, T), rng.uniform(1, 0.6 * h + 1, T), rng.uniform(0, np.pi, T)
        dx, dy = np.stack([-bw, bw, bw, -bw], 1) / 2, np.stack([-bh, -bh, bh, bh], 1) / 2
        c, s = np.cos(ang)[:, None], np.sin(ang)[:, None]
        gt[a:a + T] = np.stack([cx[:, None] + dx * c - dy * s, cy[:, None] + dx * s + dy * c], 2).reshape(T, 8)
        for g in range(G):
            row = code[g, a:a + T]
            if v == all_codes:
                row[:] = np.resize(np.array([INIT, LOST] + [SKIPPED] * max(skipping - 1, 0), dtype=np.int8), T)
                continue
            t = 0
            while t < T:
                row[t] = INIT
                fail = t + 1 + int(rng.integers(0, 25)) if rng.random() < 0.7 else T
                if fail >= T:
                    break
                row[fail] = LOST
                row[fail + 1:fail + skipping] = SKIPPED
                t = fail + max(skipping, 1)
    poly = gt[None] + rng.uniform(-2, 2, (G, N, 8))
    tie = rng.random((G, N)) < 0.15
    poly[tie] = np.floor(poly[tie] * 8) / 8 + 1 / 32
    return {"offsets": offsets, "wh": wh, "gt": np.round(gt, 2), "code": code, "polygon": poly}


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """float32 arrays equal bit for bit, NaN equal to NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits32(a)[~na], bits32(b)[~nb])
