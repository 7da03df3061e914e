"""The fused VOS label map as per-object COCO run lengths on the device (smk_labels_rle_encode / smk_vos_rle / smk_vos_rle_dev,
preproc.labels_rle / vos_rle / vos_rle_dev).  Everything is compared with ==: the reference values are the label bytes
smk_vos_score*_ex write (existing entries) and tests/vos_rle_ref.py over them or over tests/golden/vos_rle.npz, never the code under
test."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tracker_state_ref as R
import vos_rle_ref
from siammask_amd import _lib, preproc, rle
from test_gpu_vos import _ids, _objects

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vos_rle.npz"))
SEG = 0.35


def _ref_labels(logits, bbs, W, H, ids, alive=None, given=None, init=None, seg_thr=SEG):
    """the label map smk_vos_score_ex writes for these arguments (the counts are of no interest here) -> uint8 [H,W]"""
    O = logits.shape[0]
    bits = lambda v: (1 << O) - 1 if v is None else sum(1 << o for o in range(O) if v[o])
    inv = np.ascontiguousarray(np.stack([preproc.invert_affine(preproc.crop_back_map(bb, (W, H))) for bb in bbs]))
    idb, thr = np.ascontiguousarray(np.asarray(ids, dtype=np.uint8)), np.array([0.5])
    gt = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    cnt = torch.empty((O, 1, 2), dtype=torch.int32, device="cuda")
    lab = torch.full((H, W), 255, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().smk_vos_score_ex(
        logits.data_ptr(), int(round(logits.shape[1] ** 0.5)), inv.ctypes.data, O, W, H, -1.0, gt.data_ptr(), idb.ctypes.data,
        bits(alive), thr.ctypes.data, 1, seg_thr, cnt.data_ptr(), lab.data_ptr(), bits(given) if given is not None else 0,
        init.data_ptr() if init is not None else None, _lib.current_stream_ptr()))
    return lab.cpu().numpy()


def _planes(counts, meta):
    """(counts int32 CUDA [O,cap], meta [O,4]) -> the O int64 count arrays (None where m > cap), meta on the host"""
    c, m = counts.cpu().numpy().view(np.uint32), meta.cpu().numpy()
    return [c[o, :m[o, 0]].astype(np.int64) if m[o, 0] <= c.shape[1] else None for o in range(c.shape[0])], m


def _check(counts, meta, lab, O, what=""):
    """the device's counts and meta are those of tests/vos_rle_ref.py over the label map, and decode back to it"""
    H, W = lab.shape
    per, m = _planes(counts, meta)
    want = vos_rle_ref.encode(lab, O)
    assert np.array_equal(m, vos_rle_ref.meta(lab, O)), what
    for o in range(O):
        assert np.array_equal(per[o], want[o]), (what, o)
        assert np.array_equal(rle.decode(per[o], H, W), lab == o + 1), (what, o)
    assert np.array_equal(m[:, 1], [(lab == o + 1).sum() for o in range(O)])
    assert np.array_equal(rle.labels_decode(per, H, W), np.where(lab <= O, lab, 0))
    return per


# ---- 1. the byte source over the fixture's label maps ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one_bg", "one_fg", "one_of_32", "tiny_3", "ragged_1", "ragged_32", "tile_3", "mid_32",
                                  "two_chunks_3", "two_chunks_idle"])
def test_labels_rle_equals_the_fixture(case):
    lab, O = GOLD[case + "_labels"], GOLD[case + "_pred"].shape[0]
    h, w = lab.shape
    counts, meta = preproc.labels_rle(torch.from_numpy(lab).cuda(), O, cap=h * w + 1)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (O, h * w + 1) and tuple(meta.shape) == (O, 4)
    per, m = _planes(counts, meta)
    want = np.split(GOLD[case + "_counts"], np.cumsum(GOLD[case + "_m"])[:-1])
    assert np.array_equal(m[:, 0], GOLD[case + "_m"]) and (m[:, 2] == h).all() and (m[:, 3] == w).all()
    for o in range(O):
        assert np.array_equal(per[o], want[o]), o
    _check(counts, meta, lab, O, case)
    # fewer planes than labels: the bytes above n_obj belong to no plane
    if O == 3:
        c2, m2 = preproc.labels_rle(torch.from_numpy(lab).cuda(), 2, cap=h * w + 1)
        _check(c2, m2, lab, 2, case)


# ---- 2. the fused source against the label bytes of smk_vos_score_ex -----------------------------------------------------------
@pytest.mark.parametrize("W,H", [(33, 17), (320, 240)])
@pytest.mark.parametrize("O", [1, 3, 32])
def test_vos_rle_decodes_to_the_labels_of_vos_score(W, H, O):
    rng = np.random.default_rng(W + 7 * O)
    logits, bbs = _objects(rng, O, W, H)
    ids = _ids(rng, O)
    gt = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    _, lab = preproc.vos_score(logits, bbs, (W, H), gt, ids, [0.5], seg_thr=SEG, want_labels=True)
    lab = lab.cpu().numpy()
    cap = H * W + 1
    counts, meta = preproc.vos_rle(logits, bbs, (W, H), ids, seg_thr=SEG, cap=cap)
    _check(counts, meta, lab, O, "fused")
    assert len(np.unique(lab)) >= min(O, 2)                             # the map is not one value
    # the byte source over those bytes gives the same counts and meta
    c2, m2 = preproc.labels_rle(torch.from_numpy(lab).cuda(), O, cap=cap)
    assert torch.equal(meta, m2)
    for a, b in zip(_planes(counts, meta)[0], _planes(c2, m2)[0]):
        assert np.array_equal(a, b)
    # the default cap
    c3, m3 = preproc.vos_rle(logits, bbs, (W, H), ids, seg_thr=SEG)
    assert tuple(c3.shape) == (O, rle.default_cap(H, W)) and torch.equal(m3, meta)


def test_special_rows():
    rng = np.random.default_rng(21)
    W, H, O = 130, 70, 4
    logits, bbs = _objects(rng, O, W, H)
    ids = np.array([9, 4, 200, 17])
    a = H * W
    # idle objects: their planes are [a]
    alive = [True, False, True, False]
    lab = _ref_labels(logits, bbs, W, H, ids, alive=alive)
    per = _check(*preproc.vos_rle(logits, bbs, (W, H), ids, alive=alive, cap=a + 1), lab, O, "idle objects")
    assert per[1].tolist() == [a] and per[3].tolist() == [a] and per[0].size > 1 and per[2].size > 1
    # all idle: best = -1 is not above seg_thr
    counts, meta = preproc.vos_rle(logits, bbs, (W, H), ids, alive=[False] * O, cap=a + 1)
    per, m = _planes(counts, meta)
    assert all(p.tolist() == [a] for p in per) and m.tolist() == [[1, 0, H, W]] * O
    # ... and -1 is above a seg_thr below it: object 0 is the first maximum everywhere, as the label bytes say
    lab = _ref_labels(logits, bbs, W, H, ids, alive=[False] * O, seg_thr=-2.0)
    assert (lab == 1).all()
    per = _check(*preproc.vos_rle(logits, bbs, (W, H), ids, alive=[False] * O, seg_thr=-2.0, cap=a + 1), lab, O, "all idle, thr -2")
    assert per[0].tolist() == [0, a]
    # given rows: the init labels stand for the probability, whatever alive says
    init = np.zeros((H, W), dtype=np.uint8)
    init[5:40, 10:60] = 4
    init[30:65, 50:120] = 17
    init[0:3, :] = 200                                                  # an id that is not given: ignored
    init_d = torch.from_numpy(init).cuda()
    given = [False, True, False, True]
    for al in (None, [True, False, True, False], [False, True, False, True]):
        lab = _ref_labels(logits, bbs, W, H, ids, alive=al, given=given, init=init_d)
        got = preproc.vos_rle(logits, bbs, (W, H), ids, alive=al, given=given, init=init_d, cap=a + 1)
        _check(*got, lab, O, "given rows, alive %s" % (al,))
        assert (lab == 2).any() and (lab == 4).any()
        assert (lab[5:30, 10:50] == 2).all()                            # 1.0 beats every warped probability
    # two objects with identical logits and maps: the first wins, the second plane is empty
    lg2 = torch.cat([logits[:1], logits[:1], logits[2:3]])
    bb2 = [bbs[0], bbs[0], bbs[2]]
    lab = _ref_labels(lg2, bb2, W, H, ids[:3])
    per = _check(*preproc.vos_rle(lg2, bb2, (W, H), ids[:3], cap=a + 1), lab, 3, "identical objects")
    assert per[1].tolist() == [a] and per[0].size > 1 and (lab == 1).any()


# ---- 3. the state-block form ------------------------------------------------------------------------------------------------------
def test_the_device_state_form_against_vos_score_dev():
    rng = np.random.default_rng(78)
    H, W, O = 150, 200, 3
    bbs = [[-40.0, -30.0, 700.0, 520.0], [12.5, -80.25, 300.0, 225.0], [-90.0, -70.0, 250.0, 190.0]]
    inv = np.stack([preproc.invert_affine(preproc.crop_back_map(bb, (W, H))) for bb in bbs])
    logits = torch.from_numpy(rng.normal(0, 3, (O, 127 * 127)).astype(np.float32)).cuda()
    head = torch.from_numpy(rng.normal(0, 3, (O, 63 * 63, 25, 25)).astype(np.float32)).cuda()
    dyx = np.array([[0, 24], [12, 12], [24, 0]])
    ids, alive = [7, 3, 200], [True, True, False]
    gt = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    init = torch.from_numpy(rng.choice(np.array([0, 3, 7, 200], dtype=np.uint8), (H, W))).cuda()
    for slot in (0, 1):
        rec = np.zeros(O, dtype=R.STREAM_DTYPE)
        rec["inv_map"][:, slot] = inv
        rec["inv_map"][:, 1 - slot] = np.nan
        rec["delta_yx"][:, slot] = dyx
        rec["delta_yx"][:, 1 - slot] = 7
        state = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * O, np.uint8)])).cuda()
        for al in (None, alive):
            lab = torch.full((H, W), 255, dtype=torch.uint8, device="cuda")
            preproc.vos_score_dev(logits, state, slot, (W, H), gt, ids, [0.5], alive=al, seg_thr=SEG, labels_out=lab)
            got = preproc.vos_rle_dev(logits, state, slot, (W, H), ids, alive=al, seg_thr=SEG, cap=H * W + 1)
            _check(*got, lab.cpu().numpy(), O, "state block, slot %d" % slot)
            preproc.vos_score_dev(None, state, slot, (W, H), gt, ids, [0.5], alive=al, seg_thr=SEG, head=head, labels_out=lab)
            got = preproc.vos_rle_dev(None, state, slot, (W, H), ids, alive=al, seg_thr=SEG, head=head, cap=H * W + 1)
            _check(*got, lab.cpu().numpy(), O, "head column, slot %d" % slot)
            assert len(np.unique(lab.cpu().numpy())) >= 3
        # a given row through the state-block entry (the _ex scoring entry writes the reference bytes)
        L, idb, thr = _lib.lib(), np.array(ids, dtype=np.uint8), np.array([0.5])
        cnt = torch.empty((O, 1, 2), dtype=torch.int32, device="cuda")
        lab = torch.full((H, W), 255, dtype=torch.uint8, device="cuda")
        _lib.check(L.smk_vos_score_dev_ex(logits.data_ptr(), None, 0, 127, state.data_ptr(), slot, O, W, H, -1.0, gt.data_ptr(),
                                          idb.ctypes.data, 0b011, thr.ctypes.data, 1, SEG, cnt.data_ptr(), lab.data_ptr(), 0b100,
                                          init.data_ptr(), _lib.current_stream_ptr()))
        got = preproc.vos_rle_dev(logits, state, slot, (W, H), ids, alive=alive, given=[False, False, True], init=init, seg_thr=SEG,
                                  cap=H * W + 1)
        _check(*got, lab.cpu().numpy(), O, "given row, slot %d" % slot)
        assert (lab == 3).any()


# ---- 4. what is written, and what is not ---------------------------------------------------------------------------------------------
def _raw_setup(W, H, O, cap, seed=5):
    rng = np.random.default_rng(seed)
    logits, bbs = _objects(rng, O, W, H)
    ids = np.ascontiguousarray(_ids(rng, O).astype(np.uint8))
    inv = np.ascontiguousarray(np.stack([preproc.invert_affine(preproc.crop_back_map(bb, (W, H))) for bb in bbs]))
    need = _lib.lib().smk_rle_workspace(O, W, H)
    guard = 1024
    buf = lambda n: torch.full((n + 2 * guard,), 0x7F, dtype=torch.uint8, device="cuda")
    return logits, bbs, ids, inv, need, guard, buf(need), buf(O * cap * 4), buf(O * 16)


def test_nothing_is_written_beyond_the_outputs_and_two_calls_agree():
    W, H, O, cap = 130, 70, 5, 40
    L = _lib.lib()
    logits, bbs, ids, inv, need, g, ws, cnt, meta = _raw_setup(W, H, O, cap)
    assert need == (O * ((W * H + 63) // 64) * 8 + 255) // 256 * 256
    lab = _ref_labels(logits, bbs, W, H, ids, alive=[True, True, False, True, True])
    lab_d = torch.from_numpy(lab).cuda()
    snaps = []
    for form in ("fused", "fused", "bytes", "bytes"):
        if form == "fused":
            _lib.check(L.smk_vos_rle(logits.data_ptr(), 127, inv.ctypes.data, O, W, H, -1.0, ids.ctypes.data, 0b11011, SEG, 0, None, cap,
                                     ws.data_ptr() + g, need, cnt.data_ptr() + g, meta.data_ptr() + g, _lib.current_stream_ptr()))
        else:
            _lib.check(L.smk_labels_rle_encode(lab_d.data_ptr(), O, W, H, cap, ws.data_ptr() + g, need, cnt.data_ptr() + g,
                                               meta.data_ptr() + g, _lib.current_stream_ptr()))
        for t in (ws, cnt, meta):
            assert (t[:g] == 0x7F).all() and (t[-g:] == 0x7F).all(), form
        snaps.append((ws.cpu().numpy().copy(), cnt.cpu().numpy().copy(), meta.cpu().numpy().copy()))
    for a, b in zip(snaps[0], snaps[1]):                                # a second call over the filled workspace: the same bytes
        assert np.array_equal(a, b)
    for a, b in zip(snaps[0], snaps[2]):                                # the byte source: the same words, counts and meta
        assert np.array_equal(a, b)
    for a, b in zip(snaps[2], snaps[3]):
        assert np.array_equal(a, b)
    words = snaps[0][0][g:g + O * ((W * H + 63) // 64) * 8].view(np.uint64).reshape(O, -1)
    assert not words[2].any() and words[0].any()                        # the idle object's words were written as zeros
    m = snaps[0][2][g:g + O * 16].view(np.int32).reshape(O, 4)
    c = snaps[0][1][g:g + O * cap * 4].view(np.uint32).reshape(O, cap)
    want = vos_rle_ref.encode(lab, O)
    assert np.array_equal(m, vos_rle_ref.meta(lab, O))
    for o in range(O):
        n = min(m[o, 0], cap)
        assert np.array_equal(c[o, :n], want[o][:n]) and (c[o, n:] == 0x7F7F7F7F).all(), o        # elements past m are not written


def test_a_small_cap_reports_the_true_count():
    W, H, O = 130, 70, 3
    rng = np.random.default_rng(9)
    logits, bbs = _objects(rng, O, W, H)
    ids = _ids(rng, O)
    lab = _ref_labels(logits, bbs, W, H, ids)
    want = vos_rle_ref.encode(lab, O)
    cap = int(sorted(c.size for c in want)[1]) - 1                      # one short of the median: at least two planes overflow
    assert cap >= 2
    for counts, meta in (preproc.vos_rle(logits, bbs, (W, H), ids, cap=cap), preproc.labels_rle(torch.from_numpy(lab).cuda(), O, cap=cap)):
        k = counts.shape[1]
        m, c = meta.cpu().numpy(), counts.cpu().numpy().view(np.uint32)
        assert np.array_equal(m, vos_rle_ref.meta(lab, O)) and (m[:, 0] > k).any()        # m is the true count even when m > cap
        for o in range(O):
            assert np.array_equal(c[o, :min(k, m[o, 0])], want[o][:k]), o                  # the first cap counts are right


def test_refusals_leave_the_outputs_untouched():
    W, H, O, cap = 130, 70, 3, 40
    L = _lib.lib()
    logits, bbs, ids, inv, need, g, ws, cnt, meta = _raw_setup(W, H, O, cap)
    lab = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    rec = np.zeros(O, dtype=R.STREAM_DTYPE)
    rec["inv_map"][:, 0] = inv
    state = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * O, np.uint8)])).cuda()
    sp = _lib.current_stream_ptr()
    P = lambda t: t.data_ptr() + g
    order = ("O", "W", "H", "cap", "ws", "ws_bytes", "counts", "meta", "given", "init", "slot")
    good = dict(O=O, W=W, H=H, cap=cap, ws=P(ws), ws_bytes=need, counts=P(cnt), meta=P(meta), given=0, init=None, slot=0)
    assert set(good) == set(order)

    def calls(k, which=(0, 1, 2)):
        """the return codes of the entries `which` (0: the byte source, 1: kernarg maps, 2: the state block) with `k` changed"""
        a = dict(good, **k)
        entries = (
            lambda: L.smk_labels_rle_encode(lab.data_ptr(), a["O"], a["W"], a["H"], a["cap"], a["ws"], a["ws_bytes"], a["counts"],
                                            a["meta"], sp),
            lambda: L.smk_vos_rle(logits.data_ptr(), 127, inv.ctypes.data, a["O"], a["W"], a["H"], -1.0, ids.ctypes.data, 7, SEG,
                                  a["given"], a["init"], a["cap"], a["ws"], a["ws_bytes"], a["counts"], a["meta"], sp),
            lambda: L.smk_vos_rle_dev(logits.data_ptr(), None, 0, 127, state.data_ptr(), a["slot"], a["O"], a["W"], a["H"], -1.0,
                                      ids.ctypes.data, 7, SEG, a["given"], a["init"], a["cap"], a["ws"], a["ws_bytes"], a["counts"],
                                      a["meta"], sp))
        return tuple(entries[i]() for i in which)

    shared = (dict(O=0), dict(O=33), dict(W=0), dict(H=4097), dict(cap=0), dict(cap=W * H + 2), dict(ws_bytes=need - 1), dict(ws=None),
              dict(ws=P(ws) + 4), dict(counts=P(cnt) + 2), dict(meta=None), dict(O=4))
    for bad in shared:
        assert calls(bad) == (-1, -1, -1), bad
    for bad in (dict(given=8), dict(given=1), dict(given=1 << 31)):     # bits at or above n_obj; no init labels
        assert calls(bad, (1, 2)) == (-1, -1), bad
    assert calls(dict(slot=2), (2,)) == (-1,) and calls(dict(slot=-1), (2,)) == (-1,)
    torch.cuda.synchronize()
    for t in (ws, cnt, meta):
        assert (t == 0x7F).all()
    assert calls({}) == (0, 0, 0)                                       # and the good call goes through
    torch.cuda.synchronize()
    assert not (meta[g:g + O * 16] == 0x7F).all()
