"""The counts of several videos in one launch (smk_vos_score_v / smk_vos_score_dev_v, preproc.vos_score_v / vos_score_dev_v;
DESIGN.md 3.21).  The oracle is the existing smk_vos_score_ex / smk_vos_score_dev_ex called once per group at the group's own size
with the group's logits rows, maps, ids and gt gathered; the whole [B,K,2] output is compared with ==, rows of slots that are not
scored against zeros.  B = 8 slots on a 300 x 45 canvas; the groups {0, 2, 5} at 300 x 45 (two x-workgroups, the second with 44
lanes; 45 rows are no multiple of the 4 a workgroup covers), {1} at 33 x 41 (whole workgroups outside the group) and {3, 7} at
64 x 1; slots 4 and 6 are in no group; slot 7 repeats slot 0's id in another group."""
import numpy as np
import pytest
import torch

import tracker_state_ref as R
from siammask_amd import _lib, preproc, vos
from test_gpu_vos import _objects

pytestmark = pytest.mark.gpu
B, CW, CH = 8, 300, 45
GROUPS = [[0, 2, 5], [1], [3, 7]]
SIZES = [(300, 45), (33, 41), (64, 1)]                                  # (w, h)
IDLE = [4, 6]
IDS = np.array([9, 4, 200, 17, 1, 3, 2, 9])
FOREIGN = [4, 9, 200]                                                   # per group: an id of ANOTHER group's member
NOBODY = 251
_cache = {}


def _setup():
    """float32 logits [B, 127 * 127] and one back box per slot, mapped into its group's frame (test_gpu_vos._objects)"""
    if "setup" not in _cache:
        rng = np.random.default_rng(321)
        logits = torch.from_numpy(rng.normal(0, 3, (B, 127 * 127)).astype(np.float32)).cuda()
        bbs = [[0.0, 0.0, 127.0, 127.0]] * B
        for slots, (w, h) in zip(GROUPS, SIZES):
            lg, boxes = _objects(rng, len(slots), w, h)
            for r, b in enumerate(slots):
                logits[b], bbs[b] = lg[r], boxes[r]
        s = 127 / 60.0                                                  # slot 5: a 60 x 60 square at x = 235 .. 295, y = -5 .. 55 --
        bbs[5] = [-235 * s, 5 * s, 300 * s, 45 * s]                     # predictions inside the partial x-workgroup (tools/test.py:279)
        _cache["setup"] = (logits, bbs)
    return _cache["setup"]


def _maps(g, seed):
    """a label map of group g: its members' ids, an id of another group's member, an id nobody has and background"""
    w, h = SIZES[g]
    rng = np.random.default_rng(seed + g)
    vals = np.array([0, NOBODY, FOREIGN[g]] + [int(IDS[b]) for b in GROUPS[g]], dtype=np.uint8)
    assert FOREIGN[g] in IDS.tolist() and FOREIGN[g] not in IDS[GROUPS[g]].tolist() and NOBODY not in IDS.tolist()
    return torch.from_numpy(vals[rng.integers(0, len(vals), (h, w))]).cuda()


def _gt():
    if "gt" not in _cache:
        _cache["gt"] = [_maps(g, 40) for g in range(3)]
    return list(_cache["gt"])


def _init(g):
    return _maps(g, 3)


def _bits(slots, v, default):
    return default if v is None else sum(1 << r for r, b in enumerate(slots) if v[b])


def _oracle(logits, bbs, g, gt, thrs, alive, given, init):
    """smk_vos_score_ex for group g at its own size, rows / maps / ids / gt gathered -> int32 [n_g, K, 2]"""
    slots, (w, h) = GROUPS[g], SIZES[g]
    O, thr = len(slots), np.ascontiguousarray(thrs, dtype=np.float64)
    lg = logits[slots].contiguous()
    inv = np.ascontiguousarray(np.stack([preproc.invert_affine(preproc.crop_back_map(bbs[b], (w, h))) for b in slots]))
    ids = np.ascontiguousarray(IDS[slots].astype(np.uint8))
    out = torch.full((O, thr.size, 2), -7, dtype=torch.int32, device="cuda")
    gbits = _bits(slots, given, 0)
    _lib.check(_lib.lib().smk_vos_score_ex(lg.data_ptr(), 127, inv.ctypes.data, O, w, h, -1.0, gt.data_ptr(), ids.ctypes.data,
                                          _bits(slots, alive, (1 << O) - 1), thr.ctypes.data, int(thr.size), 0.35, out.data_ptr(), None,
                                          gbits, init[g].data_ptr() if gbits else None, _lib.current_stream_ptr()))
    return out.cpu().numpy()


def _prefilled(K):
    return torch.full((B, K, 8), 0xA5, dtype=torch.uint8, device="cuda").view(torch.int32)


def _want(rows, K, gt, live):
    want = np.zeros((B, K, 2), dtype=np.int32)
    for g, slots in enumerate(GROUPS):
        if gt[g] is not None and (live is None or live[g]):
            want[slots] = rows(g)
    return want


def _run(thrs=vos.THRS, alive=None, given=None, init=None, live=None, gt=None):
    logits, bbs = _setup()
    gt = _gt() if gt is None else gt
    K = len(thrs)
    out = _prefilled(K)
    args = (logits, bbs, (CW, CH), GROUPS, SIZES, gt, IDS, thrs)
    kw = dict(alive=alive, given=given, init=init, live=live, out=out)
    assert preproc.vos_score_v(*args, **kw) is out and tuple(out.shape) == (B, K, 2)
    first = out.cpu().numpy()
    preproc.vos_score_v(*args, **kw)                                    # over the counts of the first call: the same bytes
    assert np.array_equal(first, out.cpu().numpy())
    want = _want(lambda g: _oracle(logits, bbs, g, gt[g], thrs, alive, given, init), K, gt, live)
    assert np.array_equal(first, want), "counts differ at (slot, threshold, which) %s" % np.argwhere(first != want)[:8].tolist()
    assert not first[IDLE].any()                                        # a slot in no group: zeros
    return first


def _members(*on):
    return [b in on for b in range(B)]


def test_all_alive_at_the_four_thresholds():
    c = _run()
    scored = [b for s in GROUPS for b in s]
    assert (c[scored, :, 1] > 0).all() and ((c[..., 0] > 0) & (c[..., 0] < c[..., 1])).any()      # the case is not trivial
    assert (c[[0, 1, 3], 0, 0] > 0).any()
    logits, bbs = _setup()
    _, prob = preproc.paste_masks(logits[5:6].contiguous(), [bbs[5]], SIZES[0], want_prob=True)
    assert (prob[0, :, 256:] > 0.45).any() and c[5, 3, 0] > 0           # slot 5 predicts inside the second x-workgroup
    assert (CW + 255) // 256 == 2 and CW - 256 == 44 and CH % 4 != 0 and 33 < 256 and 41 < CH


def test_eight_thresholds_and_one():
    c8 = _run(thrs=np.linspace(0.1, 0.9, 8))
    assert (np.diff(c8[0, :, 1]) <= 0).all() and c8[0, 0, 1] > c8[0, 7, 1]      # a higher threshold predicts fewer pixels
    c1 = _run(thrs=[0.35])
    assert np.array_equal(c1[:, 0], _run()[:, 1])                       # vos.THRS[1] is 0.35


def test_a_threshold_equal_to_a_probability_does_not_count():
    logits, bbs = _setup()
    slots, (w, h) = GROUPS[0], SIZES[0]
    _, prob = preproc.paste_masks(logits[slots].contiguous(), [bbs[b] for b in slots], (w, h), want_prob=True)
    prob, gt0 = prob.cpu().numpy(), _gt()[0].cpu().numpy()
    # a pixel of group 0 where slot 0 wins, inside (0.3, 0.9), and not annotated with slot 0's id
    ok = (prob.argmax(axis=0) == 0) & (prob[0] > 0.3) & (prob[0] < 0.9) & (gt0 != IDS[0])
    # the paste-back and the scoring kernels are different kernels and may differ in a probability's last bit at some pixels: of
    # eight candidates keep the first at which the EXISTING scoring kernel counts what numpy counts from the read-back values
    cand = np.argwhere(ok)
    cand = cand[::max(1, len(cand) // 8)][:8]
    best, arg = prob.max(axis=0).astype(np.float64), prob.argmax(axis=0)
    numpy_union = lambda t: int(np.count_nonzero(((best > t) & (arg == 0)) | (gt0 == IDS[0])))
    at = [np.float64(prob[0, y, x]) for y, x in cand]
    below = [np.nextafter(p, -np.inf) for p in at]
    u_at, u_below = (_oracle(logits, bbs, 0, _gt()[0], t, None, None, None)[0, :, 1] for t in (at, below))
    good = [i for i in range(len(cand)) if u_at[i] == numpy_union(at[i]) and u_below[i] == numpy_union(below[i])]
    assert good, "no candidate pixel at which the paste-back's value is the scoring kernel's"
    y, x = cand[good[0]]
    p0 = np.float64(prob[0, y, x])
    thrs = [p0, np.nextafter(p0, -np.inf), np.nextafter(p0, np.inf)]
    assert np.float32(thrs[1]) == prob[0, y, x] and np.float32(thrs[2]) == prob[0, y, x]      # float32 sees three equal values
    c = _run(thrs=thrs)
    assert c[0, 0, 1] == numpy_union(thrs[0]) and c[0, 1, 1] == numpy_union(thrs[1])
    assert c[0, 1, 1] - c[0, 0, 1] >= 1                                 # the pixel is counted just below its value, not at it
    assert np.array_equal(c[:, 0], c[:, 2])


def test_a_given_member_beside_an_alive_one_and_given_wins():
    init = [_init(0), None, _init(2)]
    given = _members(2, 7)
    c = _run(alive=_members(0, 5, 1, 3), given=given, init=init)
    c2 = _run(alive=_members(0, 2, 5, 1, 3, 7), given=given, init=init)         # 'given' wins whatever alive says
    assert np.array_equal(c, c2)
    assert c[2, :, 1].min() > 0 and c[7, :, 1].min() > 0 and c[0, 0, 1] > 0 and not np.array_equal(c, _run())
    assert np.array_equal(c[2, 0], c[2, 3])                             # a given object's probability is 0 or 1: one count for every threshold


def test_a_member_neither_alive_nor_given_keeps_its_targets():
    c = _run(alive=_members(0, 2, 1, 3))
    gt = _gt()
    for b, g in ((5, 0), (7, 2)):                                       # nothing predicted: no intersection, the union is the annotation
        assert not c[b, :, 0].any() and (c[b, :, 1] == int((gt[g] == int(IDS[b])).sum())).all() and c[b, 0, 1] > 0


def test_a_group_without_gt_and_a_group_that_is_not_live():
    gt = _gt()
    full = _run()
    c = _run(gt=[gt[0], None, gt[2]])
    assert not c[1].any() and np.array_equal(c[[0, 2, 5, 3, 7]], full[[0, 2, 5, 3, 7]])
    c = _run(gt=[None, gt[1], None])
    assert not c[[0, 2, 5, 3, 7]].any() and np.array_equal(c[1], full[1])
    c = _run(live=[True, False, True])
    assert not c[1].any() and np.array_equal(c[[0, 2, 5, 3, 7]], full[[0, 2, 5, 3, 7]])
    c = _run(live=[False, True, False], gt=[gt[0], gt[1], None])
    assert not c[[0, 2, 5, 3, 7]].any() and np.array_equal(c[1], full[1])
    with pytest.raises(ValueError, match="nothing to score"):
        preproc.vos_score_v(*_setup(), (CW, CH), GROUPS, SIZES, [None, None, None], IDS, vos.THRS)


def test_two_videos_with_the_same_id_do_not_see_each_other():
    # slot 7 (group 2) has slot 0's id 9 and group 1's gt holds 9 as well: only group 0's own pixels reach slot 0, and the
    # other way round
    c, gt = _run(alive=_members()), _gt()
    assert IDS[7] == IDS[0] and int((gt[1] == 9).sum()) > 0
    assert c[0, 0, 1] == int((gt[0] == 9).sum()) and c[7, 0, 1] == int((gt[2] == 9).sum()) and c[0, 0, 1] != c[7, 0, 1]


@pytest.mark.parametrize("use_head", [False, True])
def test_the_state_block_form_against_vos_score_dev_ex(use_head):
    logits, bbs = _setup()
    rng = np.random.default_rng(78)
    S, ms = 5, 63 if use_head else 127
    head = torch.from_numpy(rng.normal(0, 3, (B, ms * ms, S, S)).astype(np.float32)).cuda() if use_head else None
    init, gt, thrs = [_init(0), None, None], _gt(), np.ascontiguousarray(vos.THRS)
    given, alive = _members(5), _members(0, 2, 1, 3)
    gt[1] = None if use_head else gt[1]
    ids8 = np.ascontiguousarray(IDS.astype(np.uint8))
    L = _lib.lib()
    for slot in (0, 1):
        rec = np.zeros(B, dtype=R.STREAM_DTYPE)
        for slots, (w, h) in zip(GROUPS, SIZES):
            for b in slots:
                rec["inv_map"][b, slot] = preproc.invert_affine(preproc.crop_back_map(bbs[b], (w, h)))
        rec["inv_map"][:, 1 - slot] = np.nan
        rec["delta_yx"][:, slot] = rng.integers(0, S, (B, 2))
        rec["delta_yx"][:, 1 - slot] = 3
        block = lambda r: torch.from_numpy(np.concatenate([r.view(np.uint8).reshape(-1), np.zeros(16 * len(r), np.uint8)])).cuda()
        out = _prefilled(4)
        preproc.vos_score_dev_v(None if use_head else logits, block(rec), slot, (CW, CH), GROUPS, gt, thrs, sizes=SIZES, object_ids=IDS,
                                alive=alive, given=given, init=init, head=head, mask_size=ms, out=out)

        def rows(g):
            slots, (w, h) = GROUPS[g], SIZES[g]
            O = len(slots)
            src = (head if use_head else logits)[slots].contiguous()
            st, o = block(rec[slots]), torch.full((O, 4, 2), -7, dtype=torch.int32, device="cuda")
            gbits, ids_g = _bits(slots, given, 0), np.ascontiguousarray(ids8[slots])
            _lib.check(L.smk_vos_score_dev_ex(None if use_head else src.data_ptr(), src.data_ptr() if use_head else None, S if use_head else 0,
                                              ms, st.data_ptr(), slot, O, w, h, -1.0, gt[g].data_ptr(), ids_g.ctypes.data,
                                              _bits(slots, alive, 0), thrs.ctypes.data, 4, 0.35, o.data_ptr(), None, gbits,
                                              init[g].data_ptr() if gbits else None, _lib.current_stream_ptr()))
            return o.cpu().numpy()
        got, want = out.cpu().numpy(), _want(rows, 4, gt, None)
        assert np.array_equal(got, want), (slot, use_head, np.argwhere(got != want)[:8].tolist())
        assert not got[IDLE].any() and got[5, 0, 0] > 0 and got[0, 0, 1] > 0 and not got[7, :, 0].any() and got[7, 0, 1] > 0
        assert bool(got[1].any()) == (not use_head)
