"""Per-stream IoU counts on the device (smk_iou_score / smk_iou_score_dev, preproc.iou_score*): the per-frame part of the
reference's IouMeter.add for B independent streams, fused with the paste-back.  The counts are integers over the very
probabilities smk_paste_mask / smk_paste_mask_dev write, so everything is compared EXACTLY: against numpy on the read-back
prob_out thresholded in float64, and the mask bytes against the paste entries'.  No tolerance appears in this file."""
import numpy as np
import pytest
import torch

import tracker_state_ref as R
from siammask_amd import preproc, tune

pytestmark = pytest.mark.gpu
MS = 127
SHAPES = [(300, 37), (1, 1), (256, 4)]        # two column blocks with a ragged last one and H % 4 != 0; one pixel; exactly one block


def _thrs(K, seed):
    """K thresholds in shuffled order; 16 of them hold one below -1 (every pixel is predicted, the border's -1 included) and
    values >= 1 (nothing is)"""
    rng = np.random.default_rng(seed)
    if K == 1:
        return np.array([0.35])
    if K == 11:
        return rng.permutation(tune.THRS_VOS)
    assert K == 16
    return rng.permutation(np.concatenate([tune.THRS_VOS, [-1.5, 1.0, 1.5, 0.05, 0.999]]))


def _streams(rng, B, W, H, ms=MS):
    """B smooth logit maps and the boxes that paste each into the W x H frame, part of the patch outside the frame; with B > 1
    the LAST stream's patch lies wholly outside, so every pixel of it is the border -> (logits cuda [B, ms*ms], back_boxes)"""
    yy, xx = np.mgrid[0:ms, 0:ms]
    lg, bbs = [], []
    for b in range(B):
        cx, cy, r = rng.uniform(0.45, 0.55) * ms, rng.uniform(0.45, 0.55) * ms, rng.uniform(0.25, 0.4) * ms
        lg.append(4.0 - 8.0 * (((xx - cx) / r) ** 2 + ((yy - cy) / r) ** 2) ** 0.5 + rng.normal(0, 0.3, (ms, ms)))
        side = rng.uniform(0.8, 1.6) * max(min(W, H), 8)
        x0, y0 = rng.uniform(0.3, 0.7) * W - side / 2, rng.uniform(0.3, 0.7) * H - side / 2
        if B > 1 and b == B - 1:
            x0 = 3.0 * W + 50.0
        s = ms / side
        bbs.append([-x0 * s, -y0 * s, W * s, H * s])                  # tools/test.py:279
    return torch.from_numpy(np.stack(lg).reshape(B, ms * ms).astype(np.float32)).cuda(), bbs


def _gt(prob, form, rng):
    """annotations from the pasted probabilities [B,H,W], shifted: 'shared' [H,W] (of stream 0), 'per_stream' [B,H,W], 'zero'
    [H,W]; the target bytes are 1, 7 and 255 in stripes (the target is gt > 0, not gt == id)"""
    B, H, W = prob.shape
    if form == "zero":
        return np.zeros((H, W), dtype=np.uint8)
    val = np.array([1, 7, 255], dtype=np.uint8)[(np.arange(W)[None, :] // 3 + np.arange(H)[:, None]) % 3]
    sh = np.stack([np.roll(prob[b], (min(3, H - 1), -min(5, W - 1)), axis=(0, 1)) for b in range(B)])
    gt = np.where(sh > 0.4, val[None], 0).astype(np.uint8)
    gt[:, 0, 0] = 255                                                 # (the 1 x 1 frame has a target too)
    return gt[0] if form == "shared" else gt


def _np_counts(prob, gt, thrs):
    """[B,K,2]: IouMeter.add's two sums for every stream and threshold, float32 map against float64 threshold"""
    B = prob.shape[0]
    out = np.zeros((B, len(thrs), 2), dtype=np.int32)
    p64 = prob.astype(np.float64)
    for b in range(B):
        tgt = (gt if gt.ndim == 2 else gt[b]) > 0
        for k, thr in enumerate(thrs):
            pred = p64[b] > thr
            out[b, k] = (pred & tgt).sum(), (pred | tgt).sum()
    return out


@pytest.mark.parametrize("form", ["shared", "per_stream", "zero"])
@pytest.mark.parametrize("K", [1, 11, 16])
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("W,H", SHAPES)
def test_counts_equal_numpy_over_the_pasted_probabilities(W, H, B, K, form):
    rng = np.random.default_rng(W * 1000 + H * 10 + B)
    logits, bbs = _streams(rng, B, W, H)
    thrs = _thrs(K, W + K)
    mask, prob = preproc.paste_masks(logits, bbs, (W, H), seg_thr=0.35, want_prob=True)
    prob = prob.cpu().numpy()
    gt = _gt(prob, form, rng)
    want = _np_counts(prob, gt, thrs)
    got, gmask = preproc.iou_score(logits, bbs, (W, H), torch.from_numpy(gt).cuda(), thrs, seg_thr=0.35, want_mask=True)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, K, 2)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), "counts differ at (stream, threshold, which) %s" % np.argwhere(got != want)[:8].tolist()
    assert torch.equal(gmask, mask)                                   # the bytes of smk_paste_mask
    alone = preproc.iou_score(logits, bbs, (W, H), torch.from_numpy(gt).cuda(), thrs)        # mask_out_dev NULL: the same counts
    assert isinstance(alone, torch.Tensor) and np.array_equal(alone.cpu().numpy(), want)
    # the cases are what they are for
    if B > 1 and W * H > 1:                                           # (a 1 x 1 frame's forward map has scale 0: every box maps to texel 0)
        assert (prob[B - 1] == -1.0).all()                            # wholly outside: the border everywhere
    if K == 16:
        k_all, k_none = int(np.argmin(thrs)), int(np.argmax(thrs))
        assert (want[:, k_all, 1] == W * H).all() and not want[:, k_none, 0].any()
        tg = np.stack([(gt if gt.ndim == 2 else gt[b]) > 0 for b in range(B)]).sum(axis=(1, 2))
        assert np.array_equal(want[:, k_all, 0], tg) and np.array_equal(want[:, k_none, 1], tg)
    if form == "zero":
        assert not want[..., 0].any()
    elif (W, H) == (300, 37) and K == 11:
        assert ((want[0, :, 0] > 0) & (want[0, :, 0] < want[0, :, 1])).any() and (prob[0] == -1.0).any() and (prob[0] > 0.8).any()


def test_the_threshold_comparison_is_in_float64():
    """an integer translation (bilinear weights 1, 0, 0, 0) of logits +40 pastes the probability 1.0f exactly.  Above
    nextafter(1.0, 0.0) in float64 -- the patch is predicted; not above 1.0.  In float32 both thresholds are 1.0f"""
    W, H, ms = 300, 37, 9
    logits = torch.full((2, ms * ms), 40.0, dtype=torch.float32, device="cuda")
    bbs = [[-5.0, -3.0, W - 1.0, H - 1.0], [-260.0, -20.0, W - 1.0, H - 1.0]]         # the patch at (5, 3) and at (260, 20)
    _, prob = preproc.paste_masks(logits, bbs, (W, H), want_prob=True)
    prob = prob.cpu().numpy()
    for b, (x, y) in enumerate(((5, 3), (260, 20))):
        want = np.full((H, W), -1.0, dtype=np.float32)
        want[y:y + ms, x:x + ms] = 1.0
        assert np.array_equal(prob[b], want)
    thrs = np.array([1.0, np.nextafter(1.0, 0.0)])
    assert np.float32(thrs[1]) == np.float32(1.0)
    gt = np.zeros((H, W), dtype=np.uint8)
    gt[0:10, 0:12] = 7                                                # 120 target pixels, 7 x 7 of them under stream 0's patch
    got = preproc.iou_score(logits, bbs, (W, H), torch.from_numpy(gt).cuda(), thrs).cpu().numpy()
    assert got.tolist() == [[[0, 120], [49, 120 + 81 - 49]], [[0, 120], [0, 120 + 81]]], got
    assert np.array_equal(got, _np_counts(prob, gt, thrs))


def _state(inv, dyx, slot, B):
    rec = np.zeros(B, dtype=R.STREAM_DTYPE)
    rec["inv_map"][:, slot] = inv
    rec["inv_map"][:, 1 - slot] = np.nan
    rec["delta_yx"][:, slot] = dyx
    rec["delta_yx"][:, 1 - slot] = 7
    return torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * B, np.uint8)])).cuda()


def test_the_device_state_form_against_paste_mask_dev():
    """smk_iou_score_dev with inv_map[slot] / delta_yx[slot] of a state block, from Refine logits and from a column of a 63 x 63
    mask head at score_size 25, in both slots: numpy over smk_paste_mask_dev's prob_out, and its mask bytes"""
    rng = np.random.default_rng(78)
    H, W, B = 37, 300, 3
    bbs = [[-40.0, -30.0, 700.0, 120.0], [12.5, -80.25, 300.0, 50.0], [-90.0, -10.0, 250.0, 40.0]]
    inv = np.stack([preproc.invert_affine(preproc.crop_back_map(bb, (W, H))) for bb in bbs])
    logits = torch.from_numpy(rng.normal(0, 3, (B, 127 * 127)).astype(np.float32)).cuda()
    head = torch.from_numpy(rng.normal(0, 3, (B, 63 * 63, 25, 25)).astype(np.float32)).cuda()
    dyx = np.array([[0, 24], [12, 12], [24, 0]])
    thrs = _thrs(16, 5)
    gts = rng.choice(np.array([0, 0, 1, 7, 255], dtype=np.uint8), (B, H, W))
    for slot in (0, 1):
        state = _state(inv, dyx, slot, B)
        for kw in (dict(logits=logits), dict(logits=None, head=head)):
            mask, prob = preproc.paste_masks_dev(kw["logits"], state, slot, (W, H), seg_thr=0.3, head=kw.get("head"), want_prob=True)
            prob = prob.cpu().numpy()
            for gt in (gts[0], gts):
                want = _np_counts(prob, gt, thrs)
                got, gmask = preproc.iou_score_dev(kw["logits"], state, slot, (W, H), torch.from_numpy(gt).cuda(), thrs, seg_thr=0.3,
                                                   head=kw.get("head"), want_mask=True)
                assert np.array_equal(got.cpu().numpy(), want) and torch.equal(gmask, mask), (slot, list(kw))
                assert ((want[..., 0] > 0) & (want[..., 0] < want[..., 1])).any()
        # the host-parameter form with the same maps gives the same counts
        assert torch.equal(preproc.iou_score(logits, bbs, (W, H), torch.from_numpy(gts).cuda(), thrs),
                           preproc.iou_score_dev(logits, state, slot, (W, H), torch.from_numpy(gts).cuda(), thrs))


def test_the_output_is_defined_by_the_call():
    rng = np.random.default_rng(5)
    W, H, B = 300, 37, 4
    logits, bbs = _streams(rng, B, W, H)
    gt = torch.from_numpy(rng.choice(np.array([0, 1, 7, 255], dtype=np.uint8), (H, W))).cuda()
    want = preproc.iou_score(logits, bbs, (W, H), gt, tune.THRS_VOS)
    out = torch.full((B, 11, 2), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    preproc.iou_score(logits, bbs, (W, H), gt, tune.THRS_VOS, out=out)
    first = out.clone()
    preproc.iou_score(logits, bbs, (W, H), gt, tune.THRS_VOS, out=out)
    assert torch.equal(first, want) and torch.equal(out, want) and want.any()


def test_python_entries_reject_bad_arguments():
    rng = np.random.default_rng(6)
    W, H, B = 40, 30, 2
    logits, bbs = _streams(rng, B, W, H)
    gt = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    ok = dict(logits=logits, back_boxes=bbs, im_wh=(W, H), gt=gt, thrs=tune.THRS_VOS)
    with pytest.raises(RuntimeError):
        preproc.iou_score(**dict(ok, logits=logits.cpu()))
    with pytest.raises(RuntimeError):
        preproc.iou_score(**dict(ok, gt=gt.cpu()))
    for bad in (dict(gt=gt.float()), dict(gt=gt[:20]), dict(gt=gt[None]), dict(thrs=[]), dict(thrs=[0.1] * 17),
                dict(back_boxes=bbs[:1]), dict(out=torch.zeros((B, 11, 2), device="cuda")),
                dict(mask_out=torch.zeros((B, H, W + 1), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            preproc.iou_score(**dict(ok, **bad))
