"""The label planes of several videos in one launch (smk_vos_rle_v / smk_vos_rle_dev_v, preproc.vos_rle_v / vos_rle_dev_v; DESIGN.md
3.20).  The oracle is the existing smk_vos_rle / smk_vos_rle_dev called once per group at the group's own size with the group's
logits rows, maps and ids gathered: the counts (first m) and the meta rows of the group's slots are compared with ==.  B = 8 slots on
a 70 x 45 canvas; the groups {0, 2, 5} at 70 x 45, {1} at 33 x 41 (a = 1353 is no multiple of 64) and {3, 7} at 64 x 1 (one word);
slots 4 and 6 are in no group."""
import numpy as np
import pytest
import torch

import tracker_state_ref as R
from siammask_amd import preproc
from test_gpu_vos import _objects

pytestmark = pytest.mark.gpu
SEG = 0.35
B, CW, CH = 8, 70, 45
GROUPS = [[0, 2, 5], [1], [3, 7]]
SIZES = [(70, 45), (33, 41), (64, 1)]                                   # (w, h)
IDLE = [4, 6]
IDS = np.array([9, 4, 200, 17, 1, 3, 2, 250])
CAP = CW * CH + 1
FILL = 0xA5
_cache = {}


def _setup():
    """random float32 logits [B, 127 * 127] and one back box per slot, mapped into its group's frame (test_gpu_vos._objects)"""
    if "setup" not in _cache:
        rng = np.random.default_rng(320)
        logits = torch.from_numpy(rng.normal(0, 3, (B, 127 * 127)).astype(np.float32)).cuda()
        bbs = [[0.0, 0.0, 127.0, 127.0]] * B
        for slots, (w, h) in zip(GROUPS, SIZES):
            for b, bb in zip(slots, _objects(rng, len(slots), w, h)[1]):
                bbs[b] = bb
        _cache["setup"] = (logits, bbs)
    return _cache["setup"]


def _init(g, seed=3):
    """init labels of group g: blocks of its members' ids, an id nobody has and background"""
    w, h = SIZES[g]
    rng = np.random.default_rng(seed + g)
    vals = np.array([0, 251] + [int(IDS[b]) for b in GROUPS[g]], dtype=np.uint8)
    return torch.from_numpy(vals[rng.integers(0, len(vals), (h, w))]).cuda()


def _outputs(cap):
    """counts [B,cap] and meta [B,4], every byte 0xA5"""
    return (torch.full((B, 4 * cap), FILL, dtype=torch.uint8, device="cuda").view(torch.int32),
            torch.full((B, 16), FILL, dtype=torch.uint8, device="cuda").view(torch.int32))


def _host(counts, meta):
    return counts.cpu().numpy().view(np.uint32), meta.cpu().numpy()


def _oracle(logits, bbs, g, alive, given, init):
    """smk_vos_rle for group g at its own size -> (counts uint32 [n_g, a_g + 1], meta [n_g, 4])"""
    slots, (w, h) = GROUPS[g], SIZES[g]
    sel = lambda v: None if v is None else [v[b] for b in slots]
    c, m = preproc.vos_rle(logits[slots].contiguous(), [bbs[b] for b in slots], (w, h), IDS[slots], alive=sel(alive), given=sel(given),
                           init=init[g] if init is not None else None, seg_thr=SEG, cap=w * h + 1)
    return _host(c, m)


def _compare(c, m, want, cap, live=(True, True, True), what=""):
    """every slot of every group against its oracle; idle rows and everything past min(m, cap) still hold the fill"""
    fill = np.uint32(0xA5A5A5A5)
    for g, slots in enumerate(GROUPS):
        wc, wm = want[g]
        for r, b in enumerate(slots):
            if not live[g]:
                assert m[b].tolist() == [0, 0, SIZES[g][1], SIZES[g][0]] and (c[b] == fill).all(), (what, b)
                continue
            assert np.array_equal(m[b], wm[r]), (what, b, m[b], wm[r])
            n = min(int(m[b, 0]), cap)
            assert np.array_equal(c[b, :n], wc[r, :n]) and (c[b, n:] == fill).all(), (what, b)
    for b in IDLE:
        assert m[b].tolist() == [0, 0, CH, CW] and (c[b] == fill).all(), (what, b)


def _run(alive=None, given=None, init=None, live=None, cap=CAP, setup=None):
    logits, bbs = setup or _setup()
    counts, meta = _outputs(cap)
    args = (logits, bbs, (CW, CH), GROUPS, SIZES, IDS)
    kw = dict(alive=alive, given=given, init=init, live=live, seg_thr=SEG, cap=cap, counts=counts, meta=meta)
    preproc.vos_rle_v(*args, **kw)
    first = _host(counts, meta)
    preproc.vos_rle_v(*args, **kw)                                      # over the filled workspace and outputs: the same bytes
    second = _host(counts, meta)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    want = [_oracle(logits, bbs, g, alive, given, init) for g in range(len(GROUPS))]
    return first, want


def _members(*on):
    return [b in on for b in range(B)]


def test_all_alive():
    (c, m), want = _run()
    _compare(c, m, want, CAP, what="all alive")
    assert (m[[0, 2, 5, 1, 3, 7], 0] >= 1).all() and (m[[0, 1, 3], 1] > 0).any()
    assert [m[b, 2:].tolist() for b in (0, 1, 3)] == [[45, 70], [41, 33], [1, 64]]
    assert (33 * 41) % 64 != 0 and (64 * 1 + 63) // 64 == 1


def test_a_given_member_beside_an_alive_one():
    init = [_init(0), None, _init(2)]
    given, alive = _members(2, 7), _members(0, 5, 1, 3)
    (c, m), want = _run(alive=alive, given=given, init=init)
    _compare(c, m, want, CAP, what="given")
    assert m[2, 1] > 0 and m[7, 1] > 0 and m[0, 1] > 0                  # the given planes and an alive one carry pixels
    # 'given' wins whatever alive says
    (c2, m2), want2 = _run(alive=_members(0, 2, 5, 1, 3, 7), given=given, init=init)
    _compare(c2, m2, want2, CAP, what="given and alive")
    assert np.array_equal(m2[2], m[2])


def test_a_member_neither_alive_nor_given_is_the_empty_code():
    (c, m), want = _run(alive=_members(0, 2, 1, 3))
    _compare(c, m, want, CAP, what="idle member")
    assert m[5].tolist() == [1, 0, 45, 70] and c[5, 0] == 45 * 70 and m[7].tolist() == [1, 0, 1, 64] and c[7, 0] == 64


def test_of_two_identical_members_the_lower_slot_wins():
    logits, bbs = _setup()
    lg = logits.clone()
    lg[2] = lg[0]
    bb = list(bbs)
    bb[2] = bb[0]
    (c, m), want = _run(setup=(lg, bb))
    _compare(c, m, want, CAP, what="identical members")
    assert m[2].tolist() == [1, 0, 45, 70] and m[0, 1] > 0


def test_a_group_that_is_not_live():
    (c, m), want = _run(live=[True, False, True])
    _compare(c, m, want, CAP, live=(True, False, True), what="group 1 not live")
    (c, m), want = _run(live=[False, True, False])
    _compare(c, m, want, CAP, live=(False, True, False), what="only group 1 live")


def test_a_small_cap_reports_the_true_count():
    (c, m), want = _run(cap=3)
    _compare(c, m, want, 3, what="cap 3")
    assert (m[:, 0] > 3).any() and tuple(c.shape) == (B, 3)


@pytest.mark.parametrize("use_head", [False, True])
def test_the_state_block_form_against_vos_rle_dev(use_head):
    logits, bbs = _setup()
    rng = np.random.default_rng(77)
    S, ms = 5, 63 if use_head else 127
    head = torch.from_numpy(rng.normal(0, 3, (B, ms * ms, S, S)).astype(np.float32)).cuda() if use_head else None
    init = [_init(0), None, None]
    given, alive = _members(5), _members(0, 2, 1, 3)
    for slot in (0, 1):
        rec = np.zeros(B, dtype=R.STREAM_DTYPE)
        for slots, (w, h) in zip(GROUPS, SIZES):
            for b in slots:
                rec["inv_map"][b, slot] = preproc.invert_affine(preproc.crop_back_map(bbs[b], (w, h)))
        rec["inv_map"][:, 1 - slot] = np.nan
        rec["delta_yx"][:, slot] = rng.integers(0, S, (B, 2))
        rec["delta_yx"][:, 1 - slot] = 3
        block = lambda r: torch.from_numpy(np.concatenate([r.view(np.uint8).reshape(-1), np.zeros(16 * len(r), np.uint8)])).cuda()
        counts, meta = _outputs(CAP)
        preproc.vos_rle_dev_v(None if use_head else logits, block(rec), slot, (CW, CH), GROUPS, SIZES, IDS, alive=alive, given=given,
                              init=init, seg_thr=SEG, head=head, mask_size=ms, cap=CAP, counts=counts, meta=meta)
        want = []
        for g, slots in enumerate(GROUPS):
            w, h = SIZES[g]
            oc, om = preproc.vos_rle_dev(None if use_head else logits[slots].contiguous(), block(rec[slots]), slot, (w, h), IDS[slots],
                                         alive=[alive[b] for b in slots], given=[given[b] for b in slots], init=init[g], seg_thr=SEG,
                                         head=head[slots].contiguous() if use_head else None, mask_size=ms, cap=w * h + 1)
            want.append(_host(oc, om))
        c, m = _host(counts, meta)
        _compare(c, m, want, CAP, what="state block, slot %d, head %s" % (slot, use_head))
        assert m[7].tolist() == [1, 0, 1, 64] and m[5, 1] > 0 and m[0, 1] > 0
