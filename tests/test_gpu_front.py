"""Unit parity of the fused front end of the fp16 path -- stem_pool_kernel (smk_op_stem_pool) and l1_block_kernel
(smk_op_l1_block) -- against the plain float64 restatement tests/front_ref.py.

(a) EXACT DATA, bit-equal, no tolerance.  Inputs, weights and biases are small integers over powers of two, so that every
    partial sum, in any order and on any MFMA shape, is exact in fp32: a result is one well-defined fp16 rounding of an exact
    number and the kernel has to give the very bits of the restatement.  The conditions this rests on are asserted from the
    reference before anything is launched.  The entries fill their output buffers with fp16 NaN first (an unwritten pixel fails
    the comparison) and return an error when a tile writes outside its image.  Shapes: every tile-geometry case of the two
    kernels (one pixel, one exact tile, a ragged last tile that owns one row, an interior tile, even / odd sizes), B = 3 with a
    different image per batch entry.  The per-launch kernels on the same data must give the same bits: the fused kernels round
    where the per-launch path rounds (block 0 excepted: its shortcut is stored once more there).
(b) REAL-VALUED DATA: max-norm gates against the restatement (2e-3 one layer deep, 5e-3 three layers deep), and the rms error
    of the fused kernel must not exceed 1.2 x the rms error of the per-launch chain on the same inputs -- identical rounding
    points give a ratio of 1 to within about a percent at >= 1e4 elements, one extra fp16 rounding on the output path gives
    sqrt(2).  Values: front_ops.json in the report directory of the GPU tests (test_gpu_e2e.OUT).
(c) ENGINE WIRING: a context with stem_fused = l1_fused = 1 against one with both 0.  Values: front_fused_ab.json, same directory."""
import json
import os

import numpy as np
import pytest
import torch

import front_ref as F
from helpers import rel_err
from siammask_amd import synth
from test_gpu_e2e import OUT            # where the GPU tests leave their reports

pytestmark = pytest.mark.gpu

STEM_SIZES = (7, 9, 37, 39, 40, 71)
BLOCK_CASES = [(cin, S) for cin in (64, 256) for S in (1, 7, 8, 9, 17)]
_CACHE = {}


def _ops():
    from siammask_amd import ops
    return ops


def _frozen(d):
    for a in (d.values() if isinstance(d, dict) else d):
        if a is not None:
            a.setflags(write=False)
    return d


def _exact_stem(S):
    """(data, reference) of the exact stem case, computed once, read-only; the preconditions hold or the test stops here"""
    if ("stem", S) not in _CACHE:
        d = _frozen(F.exact_stem_data(S))
        ref = _frozen(F.stem(*d))
        facts, bad = F.exact_preconditions_stem(*d, ref)
        assert not bad, (bad, facts)
        _CACHE["stem", S] = (d, ref)
    return _CACHE["stem", S]


def _exact_block(cin, S):
    if ("block", cin, S) not in _CACHE:
        d = _frozen(F.exact_block_data(cin, S))
        ref = _frozen(F.block(*d))
        facts, bad = F.exact_preconditions_block(d, ref)
        assert not bad, (bad, facts)
        _CACHE["block", cin, S] = (d, ref)
    return _CACHE["block", cin, S]


def _assert_bits(got, ref, what):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):            # (a NaN -- a pixel the kernel did not write -- equals nothing)
        ne = ~(got == ref)
        idx = np.argwhere(ne)
        raise AssertionError("%s: %d of %d elements differ (%d NaN); first at [b, c, y, x] = %s: got %r, reference %r; rows hit: %s"
                             % (what, ne.sum(), ne.size, np.isnan(got).sum(), idx[0].tolist(), got[tuple(idx[0])],
                                ref[tuple(idx[0])], sorted(set(idx[:, 2].tolist()))[:12]))


def _dev(a):
    return torch.tensor(a, device="cuda")            # (a copy: the cached arrays are read-only)


def _chain_stem(ops, x, w, b):
    p0 = ops.conv2d(x, w, b, stride=2, relu=True, dtype="f16", algo="mfma")
    return p0, ops.maxpool3x3s2(p0, dtype="f16")


def _chain_block(ops, x, w1, b1, w2, b2, w3, b3, wd=None, bd=None):
    t1 = ops.conv2d(x, w1, b1, relu=True, dtype="f16", algo="mfma")
    t2 = ops.conv2d(t1, w2, b2, pad=1, relu=True, dtype="f16", algo="mfma")
    short = x if wd is None else ops.conv2d(x, wd, bd, dtype="f16", algo="mfma")
    return ops.conv2d(t2, w3, b3, relu=True, res=short, res_mode=1, dtype="f16", algo="mfma")


# ---- (a) exact data ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", STEM_SIZES)
def test_stem_pool_exact_bits(S):
    (x, w, b), ref = _exact_stem(S)
    p0, x1 = _ops().stem_pool(_dev(x), w, b)
    _assert_bits(p0, ref["p0"], "stem_pool S=%d p0" % S)
    _assert_bits(x1, ref["x1"], "stem_pool S=%d x1" % S)


@pytest.mark.parametrize("cin,S", BLOCK_CASES)
def test_l1_block_exact_bits(cin, S):
    d, ref = _exact_block(cin, S)
    y = _ops().l1_block(_dev(d[0]), *d[1:])
    _assert_bits(y, ref["y"], "l1_block Cin=%d S=%d y" % (cin, S))


@pytest.mark.parametrize("S", STEM_SIZES)
def test_stem_per_launch_chain_exact_bits(S):
    """conv2d + maxpool3x3s2 as separate launches: the bits of the restatement, hence of the fused kernel"""
    (x, w, b), ref = _exact_stem(S)
    p0, x1 = _chain_stem(_ops(), _dev(x), w, b)
    _assert_bits(p0, ref["p0"], "per-launch stem S=%d p0" % S)
    _assert_bits(x1, ref["x1"], "per-launch stem S=%d x1" % S)


@pytest.mark.parametrize("S", [s for c, s in BLOCK_CASES if c == 256])
def test_block_per_launch_chain_exact_bits(S):
    """three conv2d launches (Cin = 256: identity shortcut): the bits of the restatement, hence of the fused kernel"""
    d, ref = _exact_block(256, S)
    y = _chain_block(_ops(), _dev(d[0]), *d[1:7])
    _assert_bits(y, ref["y"], "per-launch block S=%d y" % S)


# ---- (b) real-valued data -----------------------------------------------------------------------------------------------------

def _rms(a, ref):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - ref) ** 2)))


def _record(name, key, values):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name)
    rep = {}
    if os.path.exists(path):
        with open(path) as f:
            rep = json.load(f)
    rep[key] = values
    with open(path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print(key, values)


def _rms_report(fused, chain, ref, tol):
    fused, chain = fused.cpu().numpy(), chain.cpu().numpy()
    assert np.isfinite(fused).all()
    r = {"n": int(ref.size), "rel_fused": rel_err(fused, ref), "rel_chain": rel_err(chain, ref), "tol": tol,
         "rms_fused": _rms(fused, ref), "rms_chain": _rms(chain, ref)}
    r["rms_ratio"] = r["rms_fused"] / r["rms_chain"]
    return r


def test_stem_pool_real_data():
    ops = _ops()
    x, w, b = F.real_stem_data(71, B=2)
    ref = F.stem(x, w, b)
    xd = _dev(x)
    fused, chain = ops.stem_pool(xd, w, b), _chain_stem(ops, xd, w, b)
    rep = {k: _rms_report(fused[i], chain[i], ref[k], 2e-3) for i, k in enumerate(("p0", "x1"))}
    _record("front_ops.json", "stem_S71", rep)
    for k, r in rep.items():
        assert r["n"] >= 10000
        assert r["rel_fused"] <= 2e-3, (k, r)
        assert r["rms_fused"] <= 1.2 * r["rms_chain"], (k, r)


@pytest.mark.parametrize("cin", [64, 256])
def test_l1_block_real_data(cin):
    ops = _ops()
    d = F.real_block_data(cin, 17, B=2)
    ref = F.block(*d)["y"]
    xd = _dev(d[0])
    r = _rms_report(ops.l1_block(xd, *d[1:]), _chain_block(ops, xd, *d[1:]), ref, 5e-3)
    _record("front_ops.json", "block_Cin%d_S17" % cin, r)
    assert r["n"] >= 10000
    assert r["rel_fused"] <= 5e-3, r
    assert r["rms_fused"] <= 1.2 * r["rms_chain"], r      # (Cin = 64: the chain rounds the shortcut once more, so fused can only be better)


# ---- (c) engine wiring ----------------------------------------------------------------------------------------------------------

def test_fused_front_equals_per_launch_front_in_a_context():
    """the knobs stem_fused / l1_fused: same rounding points, different summation order -- p0 to the one-layer gate, what
    follows to the gate test_refine_chain_equals_layer_path uses for that"""
    from siammask_amd import _lib
    from siammask_amd.custom import build
    z = torch.from_numpy(synth.image_batch(3, 127)).cuda()
    x = torch.from_numpy(synth.image_batch(3, 255)).cuda()
    before = {k: _lib.tune_get(k) for k in ("stem_fused", "l1_fused")}
    got = {}
    try:
        for on in (1, 0):
            _lib.tune(stem_fused=on, l1_fused=on)
            m = build("sharp", dtype="f16", graph=True)                 # (built after the knobs are set)
            m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
            m = m.eval().cuda()
            m.template(z)
            t = {"zf": m.debug_tensor("zf").cpu().numpy()}
            m.track_mask(x)
            for k in ("p0", "p1", "search"):
                t[k] = m.debug_tensor(k).cpu().numpy()
            got[on] = t
    finally:
        _lib.tune(**before)
    assert before == {"stem_fused": 1, "l1_fused": 1}                   # the defaults are the fused kernels
    gates = {"p0": 2e-3, "p1": 5e-3, "zf": 5e-3, "search": 5e-3}
    errs = {k: rel_err(got[1][k], got[0][k]) for k in gates}
    _record("front_fused_ab.json", "fused_vs_per_launch", {"errors": errs, "gates": gates, "shapes": {k: list(got[1][k].shape) for k in gates}})
    assert got[1]["p0"].shape == (3, 64, 125, 125) and got[1]["p1"].shape == (3, 256, 63, 63)
    bad = {k: e for k, e in errs.items() if not e <= gates[k]}
    assert not bad, (bad, errs)
