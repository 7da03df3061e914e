"""CPU tests around the front-end unit parity (tests/test_gpu_front.py): the plain restatement tests/front_ref.py is pinned
against chains of the oracle's conv2d, the exact-data generators are held inside the preconditions of a bit-equality test
at every shape the GPU tests use, and every SMK_E_ARG of smk_op_stem_pool / smk_op_l1_block is exercised (no device)."""
import ctypes

import numpy as np
import pytest

from oracle import np_oracle as O
from siammask_amd import _lib
import front_ref as F

STEM_SIZES = (7, 9, 37, 39, 40, 71)
BLOCK_SIZES = (1, 7, 8, 9, 17)
BLOCK_CASES = [(cin, S) for cin in (64, 256) for S in BLOCK_SIZES]


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def test_stem_restatement_equals_oracle_chain():
    """stage by stage, from the restatement's own stored tensors, so that a 1e-16 difference cannot flip a rounding"""
    x, w, b = F.real_stem_data(23, B=2, seed=5)
    r = F.stem(x, w, b)
    pre = O.relu(O.conv2d(O.q16(x), O.q16(w), b.astype(np.float64), 2, 0, 1))
    assert r["p0_pre"].shape == (2, 64, 9, 9) and _rel(r["p0_pre"], pre) <= 1e-12
    assert np.array_equal(r["x1"], O.maxpool_3x3_s2_p1(r["p0"])) and r["x1"].shape == (2, 64, 5, 5)
    assert np.array_equal(r["p0"], r["p0"].astype(np.float16).astype(np.float64))
    # even p0 size: the last pooled row has its far halo row outside p0
    r = F.stem(*F.real_stem_data(21, B=1, seed=6))
    assert r["p0"].shape[2] == 8 and np.array_equal(r["x1"], O.maxpool_3x3_s2_p1(r["p0"]))


@pytest.mark.parametrize("cin", [64, 256])
def test_block_restatement_equals_oracle_chain(cin):
    d = F.real_block_data(cin, 6, B=2, seed=3)
    x, w1, b1, w2, b2, w3, b3, wd, bd = d
    r = F.block(*d)
    q, f8 = O.q16, lambda a: a.astype(np.float64)
    assert _rel(r["t1_pre"], O.relu(O.conv2d(q(x), q(w1), f8(b1)))) <= 1e-12
    assert _rel(r["t2_pre"], O.relu(O.conv2d(r["t1"], q(w2), f8(b2), 1, 1, 1))) <= 1e-12
    short = q(x) if cin == 256 else O.conv2d(q(x), q(wd), f8(bd))
    assert _rel(r["y_pre"], O.relu(O.conv2d(r["t2"], q(w3), f8(b3)) + short)) <= 1e-12
    for k in ("t1", "t2", "y"):
        assert np.array_equal(r[k], r[k + "_pre"].astype(np.float16).astype(np.float64))      # one rounding, straight from float64
    if cin == 64:
        # the per-launch form stores the shortcut: one more rounding, a different (never a better) result
        y2 = F.block_per_launch(*d)
        assert _rel(y2, r["y"]) <= 2e-3 and not np.array_equal(y2, r["y"])


def test_padding_rules_of_the_restatement():
    """conv2 pads t1 with ZEROS (not relu(b1)); the pool ignores what lies outside p0 (not zero: -inf)"""
    d = list(F.exact_block_data(256, 3, B=1))
    r = F.block(*d)
    t1p = np.pad(r["t1"], ((0, 0), (0, 0), (1, 1), (1, 1)))
    assert np.array_equal(r["t2_pre"], O.relu(O.conv2d(t1p, O.q16(d[3]), d[4].astype(np.float64))))
    p0 = -np.ones((1, 8, 4, 4))
    assert np.array_equal(F.pool(p0), -np.ones((1, 8, 2, 2)))


@pytest.mark.parametrize("S", STEM_SIZES)
def test_exact_stem_generator_meets_the_preconditions(S):
    x, w, b = F.exact_stem_data(S)
    assert x.shape == (3, 3, S, S) and not np.array_equal(x[0], x[1]) and not np.array_equal(x[1], x[2])
    facts, bad = F.exact_preconditions_stem(x, w, b, F.stem(x, w, b))
    assert not bad, (bad, facts)


@pytest.mark.parametrize("cin,S", BLOCK_CASES)
def test_exact_block_generator_meets_the_preconditions(cin, S):
    d = F.exact_block_data(cin, S)
    assert d[0].shape == (3, cin, S, S) and not np.array_equal(d[0][0], d[0][1])
    facts, bad = F.exact_preconditions_block(d, F.block(*d))
    assert not bad, (bad, facts)


def test_exact_data_is_order_independent_in_float32():
    """what the bit-equality rests on: with every partial sum an integer number of quanta below 2^22, float32 accumulation in
    k-steps of 16, on two accumulators, gives the very numbers of the exact sums"""
    x, w1, b1, w2, b2, w3, b3, wd, bd = F.exact_block_data(64, 9, B=1)
    r = F.block(x, w1, b1, w2, b2, w3, b3, wd, bd)
    f8 = lambda a: a.astype(np.float64)
    assert np.array_equal(O.relu(O.conv2d_f32acc(f8(x), f8(w1), f8(b1), ksplit=2)), r["t1_pre"])
    assert np.array_equal(O.relu(O.conv2d_f32acc(r["t1"], f8(w2), f8(b2), 1, 1, 1, ksplit=2)), r["t2_pre"])
    xs, ws, bs = F.exact_stem_data(9, B=1)
    assert np.array_equal(O.relu(O.conv2d_f32acc(f8(xs), f8(ws), f8(bs), 2, 0, 1, ksplit=2)), F.stem(xs, ws, bs)["p0_pre"])


def test_preconditions_reject_unsuitable_data():
    x, w, b = F.exact_stem_data(9)
    _, bad = F.exact_preconditions_stem(x, w, np.abs(b) + 1, F.stem(x, w, np.abs(b) + 1))
    assert any("signs_b" in m for m in bad)
    _, bad = F.exact_preconditions_stem(x, w * 64, b, F.stem(x, w * 64, b))
    assert any("max_p0" in m for m in bad)
    d = list(F.exact_block_data(256, 7))
    d[0] = d[0] * 0
    _, bad = F.exact_preconditions_block(tuple(d), F.block(*d))
    assert any("rounded_" in m for m in bad)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_argument_checks_of_the_front_entries():
    """every check answers SMK_E_ARG before a device is touched (there is none here); the pointers are host memory never read"""
    L = _lib.lib()
    E = -1
    f = _ptr(np.zeros(64, np.float32))
    stem = lambda **k: L.smk_op_stem_pool(*[k.get(n, d) for n, d in (
        ("x", f), ("w", f), ("b", f), ("S", 39), ("B", 3), ("p0", f), ("x1", f), ("stream", None))])
    for bad in (dict(x=None), dict(w=None), dict(b=None), dict(p0=None), dict(x1=None), dict(S=6), dict(S=0), dict(S=-1),
                dict(S=8193), dict(B=0), dict(B=-2), dict(B=1025)):
        assert stem(**bad) == E, bad
        assert b"smk_op_stem_pool" in L.smk_last_error()
    blk = lambda **k: L.smk_op_l1_block(*[k.get(n, d) for n, d in (
        ("x", f), ("w1", f), ("b1", f), ("w2", f), ("b2", f), ("w3", f), ("b3", f), ("wd", None), ("bd", None), ("Cin", 256),
        ("S", 9), ("B", 3), ("y", f), ("stream", None))])
    for bad in (dict(x=None), dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None), dict(w3=None), dict(b3=None),
                dict(y=None), dict(Cin=128), dict(Cin=0), dict(Cin=64), dict(Cin=64, wd=f), dict(Cin=64, bd=f),
                dict(wd=f), dict(bd=f), dict(wd=f, bd=f), dict(S=0), dict(S=-3), dict(S=4097), dict(B=0), dict(B=1025)):
        assert blk(**bad) == E, bad
        assert b"smk_op_l1_block" in L.smk_last_error()
    assert blk(Cin=128) == E and b"128" in L.smk_last_error()
