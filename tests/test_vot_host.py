"""The VOT overlap and the host half of the supervised loop on the CPU: csrc/vot_overlap.h through the host-only entry
smk_host_vot_overlap against the values the reference's extension returned (tests/golden/vot_overlap.npz, BIT-equal, NaN as NaN)
and against a bitmap restatement that materialises both masks (tests/vot_overlap_ref.py); siammask_amd.vot's box, number
formatting and loss / skip / re-init bookkeeping; the argument checks of the new entries, which need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import vot_overlap_ref as V
from siammask_amd import _lib, vot

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "vot_overlap.npz"))
BOUNDS = ((64, 48), (40, 700))
E = -1


def host_overlap(p1, p2, W, H):
    """vot_overlap(p1, p2, (W, H)) through the library: p1 is the annotation's place, p2 the prediction's"""
    p1 = np.ascontiguousarray(np.asarray(p1, dtype=np.float64).reshape(-1, 8))
    p2 = np.ascontiguousarray(np.asarray(p2, dtype=np.float64).reshape(-1, 8))
    ov = np.full(p1.shape[0], -3.0, dtype=np.float32)
    cnt = np.full((p1.shape[0], 4), -3, dtype=np.int32)
    L = _lib.lib()
    assert L.smk_host_vot_overlap(p2.ctypes.data, p1.ctypes.data, p1.shape[0], W, H, ov.ctypes.data, cnt.ctypes.data) == 0, \
        L.smk_last_error()
    return ov, cnt


def same_bits(a, b):
    return np.array_equal(V.bits(a)[~np.isnan(a)], V.bits(b)[~np.isnan(a)]) and np.array_equal(np.isnan(a), np.isnan(b))


@pytest.mark.parametrize("W,H", BOUNDS)
def test_host_entry_equals_the_reference_values(W, H):
    tag = "%dx%d" % (W, H)
    p1, p2, want = GOLD["p1_" + tag], GOLD["p2_" + tag], GOLD["ov_" + tag]
    got, cnt = host_overlap(p1, p2, W, H)
    bad = np.nonzero(~((V.bits(got) == V.bits(want)) | (np.isnan(got) & np.isnan(want))))[0]
    assert bad.size == 0, "pairs %s (kinds %s): got %s, the reference %s" % (
        bad[:8], GOLD["kinds"][GOLD["kind_" + tag][bad[:8]]], got[bad[:8]], want[bad[:8]])
    # the fixture is what it is meant to be: every kind, every return, NaN, tiny and full overlaps
    assert set(GOLD["kind_" + tag].tolist()) == set(range(len(GOLD["kinds"])))
    assert set(cnt[:, 3].tolist()) == {0, 1, 2, 3, 4}
    assert np.isnan(want).any() and ((want > 0) & (want < 0.01)).any() and (want == 1).any() and (want == 0).any()
    early = cnt[:, 3] != 0
    assert not cnt[early, :3].any() and not got[early].any()
    tot = cnt[~early, :3].sum(axis=1)
    with np.errstate(all="ignore"):
        assert same_bits(got[~early], cnt[~early, 2].astype(np.float32) / tot.astype(np.float32))
    # the counts without the optional output, and one pair at a time
    p1c, p2c = np.ascontiguousarray(p1), np.ascontiguousarray(p2)
    ov = np.zeros(len(p1), dtype=np.float32)
    assert _lib.lib().smk_host_vot_overlap(p2c.ctypes.data, p1c.ctypes.data, len(p1), W, H, ov.ctypes.data, None) == 0
    assert same_bits(ov, got)
    assert same_bits(np.concatenate([host_overlap(p1[i], p2[i], W, H)[0] for i in range(0, len(p1), 7)]), got[::7])


def test_probes():
    for k in ("near", "outside", "disjoint", "point"):
        p, want = GOLD["probe_" + k], GOLD["probe_" + k + "_ov"]
        got, cnt = host_overlap(p[0], p[1], 64, 48)
        assert same_bits(got, want), (k, got, want)
        back, _ = host_overlap(p[1], p[0], 64, 48)                      # finite inputs: the value does not depend on the order
        assert same_bits(back, want), k
    assert np.isnan(GOLD["probe_point_ov"][0]) and GOLD["probe_outside_ov"][0] == 0 and GOLD["probe_disjoint_ov"][0] == 0
    assert 0 < GOLD["probe_near_ov"][0] < 1


def _random_pairs(rng, n, W, H):
    def quads(n):
        q = np.empty((n, 4, 2))
        q[..., 0] = rng.uniform(-0.4 * W, 1.4 * W, (n, 4))
        q[..., 1] = rng.uniform(-0.4 * H, 1.4 * H, (n, 4))
        c = rng.uniform([0, 0], [W, H], (n, 1, 2))
        small = rng.random(n) < 0.5                                     # half of them compact: vertices near one centre
        q[small] = c[small] + rng.uniform(-0.3 * min(W, H), 0.3 * min(W, H), (int(small.sum()), 4, 2))
        return q
    a, b = quads(n), quads(n)
    b[::4] = a[::4] + rng.uniform(-3, 3, (len(a[::4]), 1, 2))           # near copies: large overlaps
    a[1::6] = np.round(a[1::6] * 2) / 2                                 # half-integers: round() half away from zero
    b[2::6] = np.round(b[2::6])                                         # integers: vertices on rows, equal neighbouring nodes
    a[3::10, 1] = a[3::10, 0]                                           # a repeated vertex
    b[5::10, 2, 1] = b[5::10, 1, 1]                                     # a horizontal edge
    b[7::10, 2, 0] = b[7::10, 1, 0]                                     # a vertical one
    return a.reshape(n, 8), b.reshape(n, 8)


@pytest.mark.parametrize("W,H,n,seed", [(64, 48, 16000, 1), (40, 700, 2500, 2), (129, 31, 1500, 3), (7, 5, 1000, 4)])
def test_host_entry_equals_the_bitmap_restatement(W, H, n, seed):
    """about 20 000 seeded random pairs in all: the interval arithmetic against materialised masks, counts included"""
    a, b = _random_pairs(np.random.default_rng(seed), n, W, H)
    got, cnt = host_overlap(a, b, W, H)
    want, wcnt = V.overlap(a, b, W, H)
    bad = np.nonzero((cnt != wcnt).any(axis=1))[0]
    assert bad.size == 0, "pairs %s: counts %s, bitmap %s" % (bad[:5], cnt[bad[:5]].tolist(), wcnt[bad[:5]].tolist())
    assert same_bits(got, want)
    assert (cnt[:, 3] == 0).sum() > n // 2 and (got[cnt[:, 3] == 0] > 0.5).any()


def test_the_restatement_reads_its_own_masks():
    """the helper on cases small enough to count by eye: two 4 x 3-pixel boxes (closed pixel ranges) sharing two columns; and
    two that share one column only -- their bounds meet in a line of no area, which the reference calls no overlap"""
    ov, cnt = V.overlap([[1, 1, 4, 1, 4, 3, 1, 3]], [[3, 1, 6, 1, 6, 3, 3, 3]], 16, 16)
    assert cnt.tolist() == [[6, 6, 6, 0]] and ov[0] == np.float32(6) / np.float32(18)
    ov, cnt = V.overlap([[1, 1, 3, 1, 3, 3, 1, 3]], [[3, 1, 5, 1, 5, 3, 3, 3]], 16, 16)
    assert cnt.tolist() == [[0, 0, 0, V.PATH_BOUNDS]] and ov[0] == 0


def test_axis_aligned_bbox_and_number_format():
    for region, want in zip(GOLD["bbox_regions"], GOLD["bbox_out"]):
        got = np.array(vot.axis_aligned_bbox(region), dtype=np.float64)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (region, got, want)
    for v, text in zip(GOLD["f2s_values"], GOLD["f2s_text"]):
        assert vot.format_value(v) == str(text), (v, vot.format_value(v), text)
    with pytest.raises(ValueError):
        vot.axis_aligned_bbox([1, 2, 3, 4])
    res = {"vot_code": np.array([[1], [-1], [2], [0], [0]], dtype=np.int8), "vot_length": np.array([4]),
           "polygon": np.arange(40, dtype=np.float64).reshape(5, 1, 4, 2) + 0.00005}
    assert vot.region_lines(res, 0) == ["1", ",".join(vot.format_value(v) for v in res["polygon"][1, 0].reshape(-1)), "2", "0"]
    # the narrowing to float32 shows in the fixture: a value whose float64 prints differently
    assert any("%.4f" % v != str(t) for v, t in zip(GOLD["f2s_values"], GOLD["f2s_text"]))


def _track_vot_codes(T, ov, skip=5):
    """the codes of tools/test.py:322-365 for one video, fed the overlap each tracked frame WOULD give: ov[f]"""
    start, lost, codes = 0, 0, []
    for f in range(T):
        if f == start:
            codes.append(1)
        elif f > start:
            if ov[f]:
                codes.append(-1)
            else:
                codes.append(2)
                lost += 1
                start = f + skip
        else:
            codes.append(0)
    return codes, lost


def _drive(T, B, ov, skip=5, length=None):
    """vot.Schedule as DeviceTracker.run(vot=) drives it: reports lag the queue head by skip - 1 frames"""
    s = vot.Schedule(T, B, skip=skip, length=length)
    starts, max_lag = [], 0
    for g in range(T):
        while s.reported <= g - s.skip:
            s.report(ov[s.reported])
        max_lag = max(max_lag, g - s.reported)
        starts.append(s.starts(g))
    while s.reported < T:
        s.report(ov[s.reported])
    return s, starts, max_lag


def test_schedule_gives_the_codes_of_track_vot():
    T, B = 20, 5
    ov = np.full((T, B), 0.5, dtype=np.float32)
    ov[3, 0] = 0                 # stream 0: a loss at 3, 3 + 5 < T; the frames of its skip window report zeros, which are ignored
    ov[4:8, 0] = 0
    ov[16, 1] = 0                # stream 1: a loss with f + 5 >= T: never starts again
    ov[2, 2] = np.nan            # stream 2: NaN is not lost
    ov[5, 3], ov[11, 3] = 0, 0   # stream 3: two losses; 11 is the first tracked frame behind the re-init at 10
    ov[0, 4] = 0                 # stream 4: a zero on its init frame is ignored; length 12, lost at 9: the start at 14 is beyond its end
    ov[9, 4] = 0
    length = [T, T, T, T, 12]
    s, starts, lag = _drive(T, B, ov, length=length)
    for b in range(B):
        n = length[b]
        codes, lost = _track_vot_codes(n, ov[:n, b])
        assert s.code[:n, b].tolist() == codes, b
        assert not s.code[n:, b].any() and not s.overlap[n:, b].any()
        assert s.lost_times[b] == lost
    assert s.code[:, 0].tolist() == [1, -1, -1, 2, 0, 0, 0, 0, 1] + [-1] * 11
    assert s.code[:, 1].tolist() == [1] + [-1] * 15 + [2, 0, 0, 0]
    assert s.code[:, 2].tolist() == [1] + [-1] * 19 and np.isnan(s.overlap[2, 2])
    assert s.code[:, 3].tolist() == [1, -1, -1, -1, -1, 2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 1, -1, -1, -1]
    assert s.code[:, 4].tolist() == [1] + [-1] * 8 + [2, 0, 0] + [0] * 8
    assert s.lost_times.tolist() == [1, 1, 0, 2, 1]
    assert [g for g, st in enumerate(starts) if st] == [0, 8, 10, 16] and starts[0] == [0, 1, 2, 3, 4]
    assert starts[8] == [0] and starts[10] == [3] and starts[16] == [3]
    assert lag == 4                                                      # the queue head is never more than skip - 1 frames ahead
    # overlap: the reported value on tracked and lost frames, 0 elsewhere
    on = (s.code == vot.TRACKED) | (s.code == vot.LOST)
    assert same_bits(s.overlap[on], ov[on]) and not s.overlap[~on].any()
    # other skips, every frame lost
    for skip in (1, 2, 7):
        z = np.zeros((T, 1), dtype=np.float32)
        s, _, lag = _drive(T, 1, z, skip=skip)
        assert s.code[:, 0].tolist() == _track_vot_codes(T, z[:, 0], skip)[0] and lag == skip - 1
    with pytest.raises(RuntimeError):
        s = vot.Schedule(10, 1)
        s.starts(5)                                                      # frame 0 has not been reported
    for bad in (dict(skip=0), dict(length=[11]), dict(length=[1, 2])):
        with pytest.raises(ValueError):
            vot.Schedule(10, 1, **bad)


def test_export_contract_and_argument_checks():
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)
    declared = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", strip("siammask_hip.h")))
    test_only = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", strip("siammask_hip_test.h")))
    L = _lib.lib()
    assert "smk_vot_overlap" in declared and "smk_host_vot_overlap" in test_only - declared
    assert all(s in _lib.SYMBOLS and hasattr(L, s) for s in ("smk_vot_overlap", "smk_host_vot_overlap"))
    f64, f32, i32 = np.zeros(64), np.zeros(8, np.float32), np.zeros(16, np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    names = (("pred", ptr(f64)), ("stride", 8), ("adv", None), ("gt", ptr(f64)), ("B", 2), ("W", 64), ("H", 48), ("ov", ptr(f32)),
             ("cnt", ptr(i32)), ("stream", None))
    dev = lambda **k: L.smk_vot_overlap(*[k.get(n, d) for n, d in names])
    # (every refusal comes before the device is touched: none of these pointers is device memory)
    assert dev(gt=None) == E and dev(ov=None) == E and dev(pred=None) == E       # no prediction and no advance rows
    assert dev(stride=9) == E and dev(stride=0) == E and dev(stride=16) == E
    assert dev(B=0) == E and dev(B=65536) == E
    assert dev(W=0) == E and dev(H=0) == E and dev(W=4097) == E and dev(H=4097) == E
    assert dev(pred=ctypes.c_void_p(f64.ctypes.data + 4)) == E and dev(ov=ctypes.c_void_p(f32.ctypes.data + 2)) == E
    assert b"smk_vot_overlap" in L.smk_last_error()
    host = lambda **k: L.smk_host_vot_overlap(*[k.get(n, d) for n, d in (
        ("pred", ptr(f64)), ("gt", ptr(f64)), ("n", 2), ("W", 64), ("H", 48), ("ov", ptr(f32)), ("cnt", None))])
    assert host() == 0
    assert host(pred=None) == E and host(gt=None) == E and host(ov=None) == E and host(n=0) == E
    assert host(W=0) == E and host(H=4097) == E
    # the largest window: 4097 x 4097 pixels, counted exactly
    full = [[0, 0, 4096, 0, 4096, 4096, 0, 4096]]
    ov, cnt = host_overlap(full, full, 4096, 4096)
    assert cnt.tolist() == [[0, 0, 4097 * 4097, 0]] and ov[0] == 1
