"""Shared helpers for the parity tests: golden-fixture loading and tolerance checks."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("sharp_damped_b2", "sharp_stress_b1", "base_damped_b1", "rpn_damped_b1")


def load_golden(name):
    g = np.load(os.path.join(GOLD, "golden_%s.npz" % name), allow_pickle=False)
    return {k: g[k] for k in g.files}


def rel_err(got, ref):
    """max|got-ref| / max|ref| (the tolerance form of SURVEY.md 8c)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


def sampled_err(gold, key, full):
    """Compare a full tensor (any float dtype, NCHW) with the strided sample stored in a fixture."""
    stride = int(gold[key + "__stride"])
    ref = gold[key + "__vals"].astype(np.float64)
    a = np.asarray(full, dtype=np.float64)
    assert tuple(a.shape) == tuple(gold[key + "__shape"]), (key, a.shape, gold[key + "__shape"])
    got = a.ravel()[::stride]
    return float(np.abs(got - ref).max() / (float(gold[key + "__maxabs"]) + 1e-30))


def assert_close(got, ref, tol, what):
    e = rel_err(got, ref)
    assert e <= tol, "%s: rel-to-max error %.3e > %.1e" % (what, e, tol)
    return e


# ---- conv_seq lists (ops.conv_seq / ops.plan_seq layer dicts) ----------------------------------------------------------

def seq_weight(rng, cout, cin, k):
    return (rng.uniform(-1, 1, size=(cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)


def seq_bottleneck(rng, cin, planes, k2=3, dil=2, tile=None, kstag=-1):
    """conv1 1x1 -> conv2 3x3 (dilated, same size) -> conv3 1x1 + input, ReLU: resnet.py:80-103"""
    return [
        dict(w=seq_weight(rng, planes, cin, 1), b=rng.uniform(-1, 1, planes).astype(np.float32), relu=True, tile=tile, kstag=kstag),
        dict(w=seq_weight(rng, planes, planes, k2), b=rng.uniform(-1, 1, planes).astype(np.float32), pad=dil * (k2 // 2), dil=dil,
             relu=True, tile=tile, kstag=kstag),
        dict(w=seq_weight(rng, cin, planes, 1), b=rng.uniform(-1, 1, cin).astype(np.float32), relu=True, res=-1, res_mode=1,
             tile=tile, kstag=kstag),
    ]


def seq_chain(rng, cin, planes, nblocks, dil, adjust=True):
    """nblocks identity Bottlenecks, each reading the previous one's output, then a 1x1 cin -> planes (adjust: no ReLU)"""
    layers = []
    for b in range(nblocks):
        blk = seq_bottleneck(rng, cin, planes, dil=dil)
        if b:
            blk[0]["src"] = len(layers) - 1
            blk[2]["res"] = len(layers) - 1
        layers += blk
    layers.append(dict(w=seq_weight(rng, planes, cin, 1), b=rng.uniform(-1, 1, planes).astype(np.float32), relu=not adjust))
    return layers
