"""Plain numpy float64 restatement of the fp16 front end -- stem_pool_kernel and l1_block_kernel -- with the kernels'
rounding points and nothing of their structure (no tiles, no halos, no fragments):

  stem   p0 = f16(relu(conv 7x7 stride 2 pad 0 (f16(x), f16(w)) + b)),  x1 = 3x3 stride 2 pad 1 maximum over the p0 pixels
         that exist (padding takes no part)
  block  t1 = f16(relu(conv1x1(f16(x), f16(w1)) + b1)),  t2 = f16(relu(conv3x3 pad 1 over the ZERO-padded t1 + b2)),
         y = f16(relu(conv1x1(t2, f16(w3)) + b3 + shortcut)),  shortcut = f16(x) (Cin = 256) or conv1x1(f16(x), f16(wd)) + bd
         (Cin = 64; not rounded on its own -- the fused kernel keeps it in the accumulator, the per-launch path stores it)

Sums are exact in float64 for the exact-data generators below (every partial sum is an integer number of quanta far below
2^53), so a result is ONE fp16 rounding of an exact number, whatever order a kernel sums in.

The generators produce small integers over powers of two; `exact_preconditions_*` state, from the reference alone, what a
bit-equality test needs of its data (tests/test_gpu_front.py asserts them before it launches anything, tests/test_front_ref.py
holds the generators inside them on the CPU)."""
import numpy as np

F16_MAX = 65504.0


def f16(a):
    """one IEEE round-to-nearest-even to fp16, returned as float64"""
    with np.errstate(over="ignore"):          # (beyond 65504: inf, which the preconditions then reject)
        return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def conv(x, w, stride=1, pad=0):
    """cross-correlation, NCHW float64, zero padding, one tap at a time"""
    B, C, H, W = x.shape
    Co, Ci, k, k2 = w.shape
    assert Ci == C and k == k2
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = np.zeros((B, Co, Ho, Wo))
    for ky in range(k):
        for kx in range(k):
            patch = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            y += np.einsum("oc,bchw->bohw", w[:, :, ky, kx], patch)
    return y


def _bias(b):
    return np.asarray(b, dtype=np.float64).reshape(1, -1, 1, 1)


def pool(p0):
    """3x3 stride 2 pad 1 maximum over the pixels that exist"""
    B, C, H, W = p0.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = np.empty((B, C, Ho, Wo))
    for oy in range(Ho):
        for ox in range(Wo):
            out[:, :, oy, ox] = p0[:, :, max(2 * oy - 1, 0):min(2 * oy + 2, H), max(2 * ox - 1, 0):min(2 * ox + 2, W)].max(axis=(2, 3))
    return out


def stem(x, w, b):
    """-> dict: p0_pre (before the fp16 store), p0, x1, mass (sum |w||x| + |b|: the bound on every partial sum)"""
    xq, wq = f16(x), f16(w)
    pre = np.maximum(conv(xq, wq, 2, 0) + _bias(b), 0)
    p0 = f16(pre)
    return {"p0_pre": pre, "p0": p0, "x1": pool(p0), "mass": conv(np.abs(xq), np.abs(wq), 2, 0) + np.abs(_bias(b))}


def block(x, w1, b1, w2, b2, w3, b3, wd=None, bd=None):
    """-> dict: t1_pre, t1, t2_pre, t2, y_pre, y and mass1 / mass2 / mass3 (sum |w||a| + |b| (+ |shortcut| terms) per layer)"""
    xq = f16(x)
    w1q, w2q, w3q = f16(w1), f16(w2), f16(w3)
    r = {}
    r["t1_pre"] = np.maximum(conv(xq, w1q) + _bias(b1), 0)
    r["t1"] = f16(r["t1_pre"])
    r["t2_pre"] = np.maximum(conv(r["t1"], w2q, 1, 1) + _bias(b2), 0)
    r["t2"] = f16(r["t2_pre"])
    if wd is None:
        assert x.shape[1] == 256
        short, smass = xq, np.abs(xq)
    else:
        assert x.shape[1] == 64
        wdq = f16(wd)
        short, smass = conv(xq, wdq) + _bias(bd), conv(np.abs(xq), np.abs(wdq)) + np.abs(_bias(bd))
    r["y_pre"] = np.maximum(conv(r["t2"], w3q) + _bias(b3) + short, 0)
    r["y"] = f16(r["y_pre"])
    r["mass1"] = conv(np.abs(xq), np.abs(w1q)) + np.abs(_bias(b1))
    r["mass2"] = conv(r["t1"], np.abs(w2q), 1, 1) + np.abs(_bias(b2))
    r["mass3"] = conv(r["t2"], np.abs(w3q)) + np.abs(_bias(b3)) + smass
    return r


def block_per_launch(x, w1, b1, w2, b2, w3, b3, wd, bd):
    """the Cin = 64 block as the per-launch path rounds it: the projection shortcut is stored as fp16 before it is added"""
    r = block(x, w1, b1, w2, b2, w3, b3, wd, bd)
    short = f16(conv(f16(x), f16(wd)) + _bias(bd))
    return f16(np.maximum(conv(r["t2"], f16(w3)) + _bias(b3) + short, 0))


# ---- exact data: small integers over powers of two -------------------------------------------------------------------------

def _sparse_ints(rng, shape, amp, density):
    return rng.integers(-amp, amp + 1, size=shape) * (rng.random(shape) < density)


def exact_stem_data(S, B=3, seed=0):
    """pixels 0..255 (a different image per batch entry), w in {-2..2} at density 0.5, integer biases in +-3000: of the
    order of the sums' own spread, so that some channels are mostly zero and others mostly positive (the pooled maximum of a
    tensor that is half zeros everywhere would be nonzero almost everywhere)."""
    rng = np.random.default_rng([7, S, seed])
    x = rng.integers(0, 256, size=(B, 3, S, S)).astype(np.float32)
    w = _sparse_ints(rng, (64, 3, 7, 7), 2, 0.5).astype(np.float32)
    b = rng.integers(-3000, 3001, size=64).astype(np.float32)
    return x, w, b


def exact_block_data(Cin, S, B=3, seed=0):
    """x integers 0..31; w1 in {-3..3} (density 0.5), b1 integers in +-40; w2 in {-3..3}/4 (density 0.25), b2 multiples of 1/4 in
    +-16; w3 in {-3..3}/2 (density 0.5), b3 multiples of 1/8 in +-8; Cin = 64: wd in {-3..3} (density 0.5), bd multiples of
    1/8 in +-8.  At S = 1 only conv2's centre tap meets the image (64 terms where larger images sum up to 576), so w2 is
    dense there: otherwise t2 stays below 512 and its quarters are stored unrounded."""
    rng = np.random.default_rng([11, Cin, S, seed])
    x = rng.integers(0, 32, size=(B, Cin, S, S)).astype(np.float32)
    w1 = _sparse_ints(rng, (64, Cin, 1, 1), 3, 0.5).astype(np.float32)
    b1 = rng.integers(-40, 41, size=64).astype(np.float32)
    w2 = (_sparse_ints(rng, (64, 64, 3, 3), 3, 0.25 if S > 1 else 1.0) / 4.0).astype(np.float32)
    b2 = (rng.integers(-64, 65, size=64) / 4.0).astype(np.float32)
    w3 = (_sparse_ints(rng, (256, 64, 1, 1), 3, 0.5) / 2.0).astype(np.float32)
    b3 = (rng.integers(-64, 65, size=256) / 8.0).astype(np.float32)
    if Cin == 64:
        wd = _sparse_ints(rng, (256, 64, 1, 1), 3, 0.5).astype(np.float32)
        bd = (rng.integers(-64, 65, size=256) / 8.0).astype(np.float32)
        return x, w1, b1, w2, b2, w3, b3, wd, bd
    return x, w1, b1, w2, b2, w3, b3, None, None


STEM_QUANTA = (1.0,)                  # integer pixels x integer weights + integer biases
BLOCK_QUANTA = (1.0, 0.25, 0.125)     # conv1: integers; conv2: quarters; conv3 + shortcut: eighths


def _signs(b):
    b = np.asarray(b)
    return bool((b > 0).any() and (b < 0).any())


def _changed(pre, stored):
    return float((pre != stored).mean())


def _check(facts, lim_mass, stored, out_keys):
    """the conditions of a bit-equality test, as a list of the ones that do NOT hold (empty = fine)"""
    bad = []
    for k, v in facts.items():
        if k.startswith("mass") and not v < lim_mass:
            bad.append("%s = %.4g quanta >= 2^22: a partial sum may round in fp32" % (k, v))
        if k.startswith("max") and not v < F16_MAX:
            bad.append("%s = %.6g >= 65504" % (k, v))
        if k.startswith("rounded_") and k[8:] in stored and not v >= 0.05:
            bad.append("%s = %.3f < 0.05: the rounding point is not exercised" % (k, v))
        if k.startswith("nonzero_") and k[8:] in out_keys and not 0.2 <= v <= 0.8:
            bad.append("%s = %.3f outside 0.2 .. 0.8" % (k, v))
        if k.startswith("signs_") and not v:
            bad.append("%s: the biases need a positive and a negative entry" % k)
    return bad


def exact_preconditions_stem(x, w, b, ref):
    """(facts, violated) for stem data and its reference ref = stem(x, w, b)"""
    for a in (x, w, b):
        assert np.array_equal(a, np.round(a)), "integers"
    facts = {"mass": float(ref["mass"].max() / STEM_QUANTA[0]), "max_p0": float(ref["p0_pre"].max()),
             "rounded_p0": _changed(ref["p0_pre"], ref["p0"]),
             "nonzero_p0": float((ref["p0"] != 0).mean()), "nonzero_x1": float((ref["x1"] != 0).mean()),
             "signs_b": _signs(b)}
    return facts, _check(facts, 2.0 ** 22, ("p0",), ("p0", "x1"))


def exact_preconditions_block(data, ref):
    """(facts, violated) for block data (the tuple of exact_block_data) and its reference ref = block(*data)"""
    x, w1, b1, w2, b2, w3, b3, wd, bd = data
    # integers x integers -> t1 integers; quarters x t1 -> t2 quarters; halves x t2 -> eighths, + integers (the shortcut)
    for a, unit in ((x, 1), (w1, 1), (b1, 1), (w2, 0.25), (b2, 0.25), (w3, 0.5), (b3, 0.125), (wd, 1), (bd, 0.125)):
        if a is not None:
            assert np.array_equal(a / unit, np.round(a / unit)), "multiples of %g" % unit
    facts = {"mass1": float(ref["mass1"].max() / BLOCK_QUANTA[0]), "mass2": float(ref["mass2"].max() / BLOCK_QUANTA[1]),
             "mass3": float(ref["mass3"].max() / BLOCK_QUANTA[2]),
             "max_t1": float(ref["t1_pre"].max()), "max_t2": float(ref["t2_pre"].max()), "max_y": float(ref["y_pre"].max()),
             "rounded_t1": _changed(ref["t1_pre"], ref["t1"]), "rounded_t2": _changed(ref["t2_pre"], ref["t2"]),
             "rounded_y": _changed(ref["y_pre"], ref["y"]),
             "nonzero_y": float((ref["y"] != 0).mean()),
             "signs_b1": _signs(b1), "signs_b2": _signs(b2), "signs_b3": _signs(b3)}
    if bd is not None:
        facts["signs_bd"] = _signs(bd)
    return facts, _check(facts, 2.0 ** 22, ("t2", "y"), ("y",))


# ---- real-valued data (gaussian inputs, weights scaled by 1 / sqrt(fan-in) as in test_gpu_ops.test_conv_classes) ---------------

def _w(rng, cout, cin, k):
    return (rng.uniform(-1, 1, size=(cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)


def _b(rng, n):
    return rng.uniform(-1, 1, size=n).astype(np.float32)


def real_stem_data(S, B=2, seed=0):
    rng = np.random.default_rng([13, S, seed])
    return rng.standard_normal((B, 3, S, S)).astype(np.float32), _w(rng, 64, 3, 7), _b(rng, 64)


def real_block_data(Cin, S, B=2, seed=0):
    rng = np.random.default_rng([17, Cin, S, seed])
    x = rng.standard_normal((B, Cin, S, S)).astype(np.float32)
    d = (x, _w(rng, 64, Cin, 1), _b(rng, 64), _w(rng, 64, 64, 3), _b(rng, 64), _w(rng, 256, 64, 1), _b(rng, 256))
    return d + ((_w(rng, 256, 64, 1), _b(rng, 256)) if Cin == 64 else (None, None))
