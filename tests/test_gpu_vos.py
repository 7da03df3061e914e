"""VOS scoring on the device (smk_vos_score / smk_vos_score_dev, preproc.vos_score*, DeviceTracker.run(gt=, vos=)).
The counts are integers over the very probabilities smk_paste_mask writes, so everything is compared EXACTLY: against
tests/vos_meter_ref.py applied to the read-back prob_out, against preproc.paste_labels for the label map, and -- in the
tracker -- against counts taken from the returned labels and against the same run without scoring."""
import numpy as np
import pytest
import torch

import tracker_state_ref as R
import vos_meter_ref as V
from siammask_amd import preproc, vos
from test_gpu_freerun import _frames, _model, _same, _tracker
from test_gpu_tracker import HP

pytestmark = pytest.mark.gpu
MS = 127
K8 = [0.5, 0.3, 0.45, 0.35, 0.9, 0.05, 0.4, -0.5]                      # unsorted; -0.5 is below every live probability


def _objects(rng, O, W, H, ms=MS):
    """O smooth logit maps and the boxes that paste each into a part of the W x H frame -> (logits cuda, back_boxes)"""
    yy, xx = np.mgrid[0:ms, 0:ms]
    lg, bbs = [], []
    for o in range(O):
        cx, cy, r = rng.uniform(0.45, 0.55) * ms, rng.uniform(0.45, 0.55) * ms, rng.uniform(0.25, 0.4) * ms
        lg.append(4.0 - 8.0 * (((xx - cx) / r) ** 2 + ((yy - cy) / r) ** 2) ** 0.5 + rng.normal(0, 0.3, (ms, ms)))
        side = rng.uniform(0.8, 1.6) * min(W, H)                      # the pasted square, centred somewhere inside the frame:
        x0, y0 = rng.uniform(0.3, 0.7) * W - side / 2, rng.uniform(0.3, 0.7) * H - side / 2      # part of it sticks out
        s = ms / side
        bbs.append([-x0 * s, -y0 * s, W * s, H * s])                  # tools/test.py:279
    return torch.from_numpy(np.stack(lg).reshape(O, ms * ms).astype(np.float32)).cuda(), bbs


def _ids(rng, O):
    return rng.choice(np.arange(1, 250), size=O, replace=False).astype(np.int64)      # non-contiguous, in no order


def _gt(prob, ids, rng, drop=()):
    """the annotation: every object's thresholded probability, shifted, the strongest on top; the objects in `drop` do not
    occur, and a corner holds a value no object has"""
    O, H, W = prob.shape
    sh = np.stack([np.roll(prob[o], (min(3, H - 1), -min(5, W - 1)), axis=(0, 1)) for o in range(O)])
    for o in drop:
        sh[o] = -1.0
    gt = np.where(sh.max(0) > 0.4, np.asarray(ids, dtype=np.uint8)[sh.argmax(0)], 0).astype(np.uint8)
    gt[: max(1, H // 8), : max(1, W // 8)] = 251
    return gt


CASES = [  # W, H, O, thrs, alive (None: all), objects absent from gt
    (200, 150, 3, vos.THRS, None, ()),
    (200, 150, 32, K8, "odd", (4, 9)),
    (200, 150, 1, [0.35], None, ()),
    (320, 37, 3, K8, [False, True, True], (1,)),                      # object 0 dead
    (320, 37, 32, vos.THRS, "first_dead", ()),
    (320, 37, 3, [0.45], [False, False, False], ()),                  # all dead
    (1, 1, 1, vos.THRS, None, ()),
    (1, 1, 3, K8, [True, False, True], ()),
    (257, 5, 2, [0.3, 0.31], None, ()),                               # one pixel in the second block of a row; H % 4 != 0
]


def _alive(spec, O):
    if spec is None:
        return None
    if spec == "odd":
        return np.arange(O) % 2 == 1
    if spec == "first_dead":
        return np.arange(O) != 0
    return np.asarray(spec)


@pytest.mark.parametrize("W,H,O,thrs,alive,drop", CASES)
def test_counts_equal_the_restatement_over_the_pasted_probabilities(W, H, O, thrs, alive, drop):
    rng = np.random.default_rng(W * 1000 + H * 10 + O)
    logits, bbs = _objects(rng, O, W, H)
    ids = _ids(rng, O)
    alive = _alive(alive, O)
    _, prob = preproc.paste_masks(logits, bbs, (W, H), want_prob=True)
    prob = prob.cpu().numpy()
    gt = _gt(prob, ids, rng, drop)
    want = V.counts(prob, gt, ids, thrs, alive)
    got, labels = preproc.vos_score(logits, bbs, (W, H), torch.from_numpy(gt).cuda(), ids, thrs, alive=alive, seg_thr=0.35,
                                    want_labels=True)
    assert got.dtype == torch.int32 and tuple(got.shape) == (O, len(thrs), 2)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), "counts differ at (object, threshold, which) %s" % np.argwhere(got != want)[:8].tolist()
    assert np.array_equal(labels.cpu().numpy(), V.labels(prob, 0.35, alive))
    if alive is None and min(W, H) >= 100 and O > 1:
        assert ((want[..., 0] > 0) & (want[..., 0] < want[..., 1])).any()      # the case is not trivial
    if alive is not None and not alive.any():
        assert not want[..., 0].any() and want[..., 1].any()          # nothing predicted: the union is the annotation
    for j in drop:
        assert not want[j, :, 0].any()


def test_a_frame_where_every_union_is_zero():
    rng = np.random.default_rng(3)
    W, H, O = 200, 150, 3
    logits, bbs = _objects(rng, O, W, H)
    gt = torch.full((H, W), 251, dtype=torch.uint8, device="cuda")     # matches no object
    got = preproc.vos_score(logits, bbs, (W, H), gt, [1, 2, 3], [1.0, 1.5], alive=None)      # a probability never exceeds 1
    assert not got.cpu().numpy().any()
    got = preproc.vos_score(logits, bbs, (W, H), gt, [1, 2, 3], vos.THRS, alive=[False] * 3)
    assert not got.cpu().numpy().any()
    assert (vos.mean_iou(got.cpu().numpy()[None].repeat(3, 0)) == 1.0).all()


def test_the_threshold_comparison_is_in_float64():
    """1 x 1 logit maps pasted into a 1 x 1 frame give prob = sigmoid(logit): search the float32 neighbourhood of logit(0.3) for a
    probability equal to (float)0.3 = 0.300000011920929 > 0.3 -- above in float64, not above in float32; and, whatever the search
    finds, thresholds on a read-back probability and its float64 neighbours"""
    centre = np.float32(np.log(0.3 / 0.7))
    n = 1024
    cand = centre.view(np.int32) + np.arange(-n, n + 1, dtype=np.int32)
    cand = cand.view(np.float32)
    box = [[0.0, 0.0, 1.0, 1.0]]
    lg = torch.from_numpy(cand.reshape(-1, 1)).cuda()
    _, prob = preproc.paste_masks(lg, box * len(cand), (1, 1), want_prob=True)
    prob = prob.cpu().numpy().reshape(-1)
    assert abs(float(prob[n]) - 0.3) < 1e-6
    gt = torch.full((1, 1), 9, dtype=torch.uint8, device="cuda")
    hit = np.nonzero(prob == np.float32(0.3))[0]
    if len(hit):
        i = int(hit[0])
        assert np.float64(prob[i]) > 0.3 and not prob[i] > np.float32(0.3)
        got = preproc.vos_score(lg[i:i + 1], box, (1, 1), gt, [9], [0.3, float(np.float32(0.3))]).cpu().numpy()
        assert got.tolist() == [[[1, 1], [0, 1]]], got                # above 0.3 in float64; not above the float32 value itself
    i = n
    p0 = np.float64(prob[i])
    thrs = [p0, np.nextafter(p0, -np.inf), np.nextafter(p0, np.inf)]
    assert np.float32(thrs[1]) == prob[i] and np.float32(thrs[2]) == prob[i]            # a float32 comparison sees three equal values
    got = preproc.vos_score(lg[i:i + 1], box, (1, 1), gt, [9], thrs).cpu().numpy()
    assert got.tolist() == [[[0, 1], [1, 1], [0, 1]]], got
    assert np.array_equal(got, V.counts(prob[i].reshape(1, 1, 1), np.full((1, 1), 9), [9], thrs))


def test_labels_equal_paste_labels_and_do_not_depend_on_the_thresholds():
    rng = np.random.default_rng(11)
    for (W, H, O) in ((200, 150, 3), (320, 37, 32)):
        logits, bbs = _objects(rng, O, W, H)
        ids = _ids(rng, O)
        gt = torch.from_numpy(rng.integers(0, 255, (H, W)).astype(np.uint8)).cuda()
        for seg_thr in (0.35, 0.3):
            want = preproc.paste_labels(logits, bbs, (W, H), seg_thr=seg_thr)
            _, a = preproc.vos_score(logits, bbs, (W, H), gt, ids, vos.THRS, seg_thr=seg_thr, want_labels=True)
            _, b = preproc.vos_score(logits, bbs, (W, H), gt, ids, [0.9], seg_thr=seg_thr, want_labels=True)
            assert torch.equal(a, want) and torch.equal(b, want) and want.any()


def test_the_device_state_form_gives_the_bits_of_the_host_parameter_form():
    """smk_vos_score_dev with inv_map[slot] / delta_yx[slot] in a state block (built as test_gpu_freerun.py does for the paste)
    against smk_vos_score with the same maps: Refine logits, and a column of a 63 x 63 head"""
    rng = np.random.default_rng(78)
    H, W, O = 150, 200, 3
    bbs = [[-40.0, -30.0, 700.0, 520.0], [12.5, -80.25, 300.0, 225.0], [-90.0, -70.0, 250.0, 190.0]]
    inv = np.stack([preproc.invert_affine(preproc.crop_back_map(bb, (W, H))) for bb in bbs])
    logits = torch.from_numpy(rng.normal(0, 3, (O, 127 * 127)).astype(np.float32)).cuda()
    head = torch.from_numpy(rng.normal(0, 3, (O, 63 * 63, 25, 25)).astype(np.float32)).cuda()
    dyx = np.array([[0, 24], [12, 12], [24, 0]])
    idx = torch.arange(O, device="cuda")
    col = head[idx, :, torch.as_tensor(dyx[:, 0], device="cuda"), torch.as_tensor(dyx[:, 1], device="cuda")].contiguous()
    ids, alive = [7, 3, 200], [True, True, False]
    gt = torch.from_numpy(rng.choice(np.array([0, 3, 7, 200, 9], dtype=np.uint8), (H, W))).cuda()
    for slot in (0, 1):
        rec = np.zeros(O, dtype=R.STREAM_DTYPE)
        rec["inv_map"][:, slot] = inv
        rec["inv_map"][:, 1 - slot] = np.nan
        rec["delta_yx"][:, slot] = dyx
        rec["delta_yx"][:, 1 - slot] = 7
        state = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * O, np.uint8)])).cuda()
        for al in (None, alive):
            want, wl = preproc.vos_score(logits, bbs, (W, H), gt, ids, K8, alive=al, want_labels=True)
            got, gl = preproc.vos_score_dev(logits, state, slot, (W, H), gt, ids, K8, alive=al, want_labels=True)
            assert torch.equal(got, want) and torch.equal(gl, wl) and want.any()
            want, wl = preproc.vos_score(col, bbs, (W, H), gt, ids, vos.THRS, alive=al, want_labels=True)
            got, gl = preproc.vos_score_dev(None, state, slot, (W, H), gt, ids, vos.THRS, alive=al, head=head, want_labels=True)
            assert torch.equal(got, want) and torch.equal(gl, wl) and want.any()


def test_the_output_row_is_overwritten():
    rng = np.random.default_rng(5)
    W, H, O = 200, 150, 3
    logits, bbs = _objects(rng, O, W, H)
    inv = np.stack([preproc.invert_affine(preproc.crop_back_map(bb, (W, H))) for bb in bbs])
    rec = np.zeros(O, dtype=R.STREAM_DTYPE)
    rec["inv_map"][:, 0] = inv
    state = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * O, np.uint8)])).cuda()
    gt = torch.from_numpy(rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), (H, W))).cuda()
    want = preproc.vos_score(logits, bbs, (W, H), gt, [1, 2, 3], vos.THRS)
    out = torch.full((O, 4, 2), -123456789, dtype=torch.int32, device="cuda")
    preproc.vos_score_dev(logits, state, 0, (W, H), gt, [1, 2, 3], vos.THRS, out=out)
    first = out.clone()
    preproc.vos_score_dev(logits, state, 0, (W, H), gt, [1, 2, 3], vos.THRS, out=out)
    assert torch.equal(first, want) and torch.equal(out, want) and want.any()


def test_python_entries_reject_what_the_paste_entries_reject():
    rng = np.random.default_rng(6)
    W, H, O = 40, 30, 2
    logits, bbs = _objects(rng, O, W, H)
    gt = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    ok = dict(logits=logits, back_boxes=bbs, im_wh=(W, H), gt=gt, object_ids=[1, 2], thrs=vos.THRS)
    with pytest.raises(RuntimeError):
        preproc.vos_score(**dict(ok, logits=logits.cpu()))
    with pytest.raises(RuntimeError):
        preproc.vos_score(**dict(ok, gt=gt.cpu()))
    for bad in (dict(gt=gt.float()), dict(gt=gt[:20]), dict(object_ids=[1]), dict(object_ids=[1, 300]), dict(thrs=[]),
                dict(thrs=[0.1] * 9), dict(alive=[True]), dict(back_boxes=bbs[:1])):
        with pytest.raises(ValueError):
            preproc.vos_score(**dict(ok, **bad))


# ---- the tracker ------------------------------------------------------------------------------------------------------------
def _gt_from_masks(masks, ids):
    """annotation [T,H,W] from a run's masks [T,B,H,W]: each object's mask shifted by a few pixels, later objects on top"""
    T, B = masks.shape[:2]
    gt = torch.zeros((T,) + tuple(masks.shape[2:]), dtype=torch.uint8, device=masks.device)
    for b in range(B):
        gt[torch.roll(masks[:, b], (4, -6), dims=(1, 2)) > 0] = int(ids[b])
    return gt


def test_tracker_sharp_fp32_counts_are_the_counts_of_the_returned_labels():
    B, T = 3, 4
    hp = dict(HP, seg_thr=0.375)                                       # 0.375, 0.25, 0.5: float32 and float64 comparisons agree
    m = _model("sharp", "f32", B)
    frames = _frames(T)
    plain = _tracker(m, hp, False, frames, B).run(frames[1:])
    ids = [5, 2, 9]
    gt = _gt_from_masks(plain["mask"], ids)
    tr = _tracker(m, hp, False, frames, B)
    res = tr.run(frames[1:], gt=gt, vos={"object_ids": ids, "thrs": [0.375, 0.25, 0.5]})
    _same(res, plain, "with scoring against without")
    assert set(res) - set(plain) == {"vos_counts", "labels"}
    c, labels = res["vos_counts"], res["labels"]
    assert c.dtype == np.int64 and c.shape == (T, B, 3, 2) and labels.dtype == torch.uint8 and tuple(labels.shape) == (T, 240, 320)
    assert torch.equal(labels > 0, (res["mask"] > 0).any(dim=1))
    lab, g = labels.cpu().numpy(), gt.cpu().numpy()
    for j in range(B):
        pred, tgt = lab == j + 1, g == ids[j]
        assert np.array_equal(c[:, j, 0, 0], (pred & tgt).sum(axis=(1, 2))), j
        assert np.array_equal(c[:, j, 0, 1], (pred | tgt).sum(axis=(1, 2))), j
    assert ((c[..., 0] > 0) & (c[..., 0] < c[..., 1])).any()
    assert (c[:, :, 1, 0] >= c[:, :, 0, 0]).all() and (c[:, :, 0, 0] >= c[:, :, 2, 0]).all()      # a lower threshold predicts more
    assert np.isfinite(vos.mean_iou(c)).all()
    # an object outside its lifetime on every frame predicts nothing; a later chunk without scoring returns today's keys
    tr = _tracker(m, hp, False, frames, B)
    dead = tr.run(frames[1:], gt=gt, vos={"object_ids": ids, "thrs": [0.375], "alive": [True, False, True]})
    assert not dead["vos_counts"][:, 1, :, 0].any() and not (dead["labels"] == 2).any()
    assert np.array_equal(dead["vos_counts"][:, 1, 0, 1], (g == ids[1]).sum(axis=(1, 2)))
    assert set(tr.run(frames[1:3])) == set(plain)


def test_tracker_sharp_fp16_b8_serial_and_both_pipeline_depths_agree():
    B, T = 8, 5
    frames = _frames(T)
    ids = list(range(11, 11 + B))
    spec = {"object_ids": ids, "thrs": vos.THRS}
    m = _model("sharp", "f16", B)
    plain = _tracker(m, HP, False, frames, B).run(frames[1:])
    gt = _gt_from_masks(plain["mask"], ids)
    serial = _tracker(m, HP, False, frames, B).run(frames[1:], gt=gt, vos=spec)
    _same(serial, plain, "serial with scoring")
    assert serial["vos_counts"][..., 0].any()
    mp = _model("sharp", "f16", B, "pipe")
    for depth in (1, 2):
        tr = _tracker(mp, HP, True, frames, B)
        mp.set_pipeline(depth)
        try:
            got = tr.run(frames[1:], gt=gt, vos=spec)
        finally:
            mp.set_pipeline(1)
        _same(got, serial, "pipeline depth %d" % depth)
        assert np.array_equal(got["vos_counts"], serial["vos_counts"]), depth
        assert torch.equal(got["labels"], serial["labels"]), depth


def test_tracker_errors_are_raised_before_any_launch():
    B, T = 2, 2
    m = _model("sharp", "f32", B)
    frames = _frames(T)
    tr = _tracker(m, HP, False, frames, B)
    gt = torch.zeros((T, 240, 320), dtype=torch.uint8, device="cuda")
    spec = {"object_ids": [1, 2], "thrs": vos.THRS}
    per_stream = frames[1:, None].expand(T, B, 240, 320, 3).contiguous()
    for kw in (dict(frames=per_stream), dict(want_mask=False), dict(gt=gt[:, :200]), dict(gt=gt[:1]), dict(gt=gt.float()),
               dict(gt=gt.cpu()), dict(vos=None), dict(gt=None), dict(vos={"object_ids": [1], "thrs": vos.THRS}),
               dict(vos={"object_ids": [1, 2], "thrs": [0.1] * 9}), dict(vos={"object_ids": [1, 2]}),
               dict(vos=dict(spec, alive=[True]))):
        args = dict(dict(frames=frames[1:], gt=gt, vos=spec), **kw)
        with pytest.raises(ValueError):
            tr.run(args.pop("frames"), **args)
        assert tr.collect() is None                                   # nothing was enqueued
    with pytest.raises(ValueError):
        tr.enqueue(per_stream[0], gt=gt[0], vos=spec)
    with pytest.raises(ValueError):
        tr.enqueue(frames[1], gt=gt[0][:100], vos=spec)
    assert tr.collect() is None
    tr.enqueue(frames[1])
    with pytest.raises(ValueError):                                   # a chunk is scored as a whole or not at all
        tr.enqueue(frames[2], gt=gt[0], vos=spec)
    assert tr.collect()["target_pos"].shape == (1, B, 2)
    rpn = _model("rpn", "f32", B)
    tr = _tracker(rpn, {k: v for k, v in HP.items() if k != "out_size"}, False, frames, B)
    with pytest.raises(ValueError):
        tr.run(frames[1:], gt=gt, vos=spec)
    assert tr.collect() is None
