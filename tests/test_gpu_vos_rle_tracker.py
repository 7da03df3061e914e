"""The VOS loop with vos['rle'] (the fused label map as per-object COCO run lengths, no mask and no label byte) on the synthetic
model and the 240 x 320 lifetime scene of tests/test_gpu_start.py: the decoded planes are the label maps of the run without the
key byte for byte, the counts and the track are the same to the bit, in every way of running the same frames; gt may be None; the
refusals come before any launch."""
import numpy as np
import pytest
import torch

import tracker_state_ref as R
from siammask_amd import rle, vos
from siammask_amd.tracker import DeviceTracker
from test_gpu_freerun import _frames, _model, _same
from test_gpu_start import _video
from test_gpu_tracker import HP

pytestmark = pytest.mark.gpu
B, T, H, W = 3, 7, 240, 320
IDS = [1, 2, 3]
START, END = {1: 0, 2: 2, 3: 0}, {"1": 6, "2": 5, "3": 3}              # object 2 starts late, 2 and 3 end early
SPEC = {"object_ids": IDS, "thrs": vos.THRS, "start": START, "end": END}


def _reserved(m, pipeline=False):
    tr = DeviceTracker(m, HP, pipeline=pipeline)
    tr.reserve(B, H, W)
    if not pipeline and getattr(m, "_pipeline", 0):
        m.set_pipeline(False)
    return tr


@pytest.fixture(scope="module")
def scene():
    """the video, its annotation, and the lifetime run without the key: the reference of every test (computed once)"""
    m = _model("sharp", "f32", B)
    frames = _frames(T - 1)                                             # T frames, indexed as the dictionaries index them
    gt = torch.from_numpy(_video(T)).cuda()
    plain = _reserved(m).run(frames, gt=gt, vos=SPEC)
    lab = plain["labels"].cpu().numpy()
    assert len(np.unique(lab)) == 4 and plain["alive"].any() and not plain["alive"].all()
    return {"m": m, "frames": frames, "gt": gt, "plain": plain, "labels": lab}


def _decodes_to(r, lab, what, cap=None):
    """res['label_rle'] decodes to labels[t] == o + 1 for every (t, o), start frames and idle objects included"""
    cap = rle.default_cap(H, W) if cap is None else cap
    assert r["size"] == (H, W) and r["cap"] == cap and r["counts"].dtype == torch.int32 and tuple(r["counts"].shape) == (T, B, cap)
    assert r["n"].dtype == np.int32 and r["n"].shape == (T, B) and r["area"].shape == (T, B)
    assert np.array_equal(r["area"], np.stack([[(lab[t] == o + 1).sum() for o in range(B)] for t in range(T)])), what
    per = rle.to_host(r)
    for t in range(T):
        assert all(p is not None for p in per[t]), (what, t)
        for o in range(B):
            assert per[t][o].size == r["n"][t, o] and np.array_equal(rle.decode(per[t][o], H, W), lab[t] == o + 1), (what, t, o)
        assert np.array_equal(rle.labels_decode(per[t], H, W), lab[t]), (what, t)
    return per


def _same_run(a, plain, what, masks=False, labels=False, counts=True):
    """a run with the key against the one without: scalars, counts, alive and events bit for bit; mask / labels None or equal"""
    if not masks:
        assert a["mask"] is None, what
    _same(dict(a, mask=a["mask"] if masks else plain["mask"]), plain, what)
    assert np.array_equal(R.bits(a["crop_box"]), R.bits(plain["crop_box"])), what
    assert np.array_equal(a["alive"], plain["alive"]) and len(a["events"]) == len(plain["events"]), what
    for e, f in zip(a["events"], plain["events"]):
        assert e["t"] == f["t"] and e["streams"] == f["streams"] and np.array_equal(e["started"], f["started"]), what
        assert np.array_equal(R.bits(e["target_pos"]), R.bits(f["target_pos"])) and np.array_equal(R.bits(e["target_sz"]), R.bits(f["target_sz"]))
    if counts:
        assert a["vos_counts"].dtype == plain["vos_counts"].dtype and np.array_equal(a["vos_counts"], plain["vos_counts"]), what
    else:
        assert "vos_counts" not in a, what
    if labels:
        assert torch.equal(a["labels"], plain["labels"]), what
    else:
        assert a["labels"] is None, what


def _same_counts(r, s, what):
    assert np.array_equal(r["n"], s["n"]) and np.array_equal(r["area"], s["area"]), what
    for pr, ps in zip(rle.to_host(r), rle.to_host(s)):
        for x, y in zip(pr, ps):
            assert x is not None and np.array_equal(x, y), what


def test_lifetime_run_with_the_key_equals_the_run_without(scene):
    m, frames, gt, plain, lab = (scene[k] for k in ("m", "frames", "gt", "plain", "labels"))
    tr = _reserved(m)
    a = tr.run(frames, gt=gt, vos=dict(SPEC, rle=True))
    assert set(a) - set(plain) == {"label_rle"} and tr.state["mask"] is None
    _same_run(a, plain, "vos['rle']")
    per = _decodes_to(a["label_rle"], lab, "vos['rle']")
    # start frames (the init mask itself) and idle objects ([a]) come out of the kernel
    assert np.array_equal(rle.decode(per[0][0], H, W), gt[0].cpu().numpy() == 1) and per[0][1].tolist() == [H * W]
    assert np.array_equal(rle.decode(per[2][1], H, W) != 0, (gt[2].cpu().numpy() == 2) & (lab[2] == 2)) and per[2][1].size > 1
    assert per[4][2].tolist() == [H * W] and per[6][1].tolist() == [H * W]
    assert np.array_equal(a["label_rle"]["n"] > 1, a["label_rle"]["area"] > 0)
    coco = rle.labels_to_coco(per[2], H, W, object_ids=IDS)
    assert [d["object_id"] for d in coco] == [IDS[o] for o in range(B) if (lab[2] == o + 1).any()] and coco[0]["size"] == [H, W]
    # gt=None: the same planes, nothing scored; vos['init'] is required then
    init = gt[:3].clone()
    init[1] = 0                                                         # (only frames 0 and 2 start objects)
    full = torch.zeros_like(gt)
    full[:3] = init
    b = _reserved(m).run(frames, vos={"object_ids": IDS, "start": START, "end": END, "init": full, "rle": True})
    _same_run(b, plain, "gt=None", counts=False)
    _same_counts(b["label_rle"], a["label_rle"], "gt=None")
    # a cap of the caller's
    c = _reserved(m).run(frames, vos={"object_ids": IDS, "start": START, "end": END, "init": full, "rle": {"cap": 900}})
    _decodes_to(c["label_rle"], lab, "cap 900", cap=900)


def test_masks_polygon_and_labels_on_request(scene):
    m, frames, gt, plain, lab = (scene[k] for k in ("m", "frames", "gt", "plain", "labels"))
    fused = _reserved(m).run(frames, gt=gt, vos=dict(SPEC, rle=True))["label_rle"]
    k = _reserved(m).run(frames, gt=gt, vos=dict(SPEC, rle={"masks": True}))
    _same_run(k, plain, "'masks': True", masks=True)
    _same_counts(k["label_rle"], fused, "'masks': True")
    out = torch.full((T, B, H, W), 9, dtype=torch.uint8, device="cuda")
    k = _reserved(m).run(frames, gt=gt, vos=dict(SPEC, rle=True), mask_out=out)
    assert k["mask"] is out
    _same_run(k, plain, "mask_out=", masks=True)
    g = _reserved(m).run(frames, gt=gt, vos=dict(SPEC, rle={"labels": True}))
    _same_run(g, plain, "'labels': True", labels=True)
    _decodes_to(g["label_rle"], lab, "'labels': True")
    _same_counts(g["label_rle"], fused, "the byte source against the fused one")
    poly = _reserved(m).run(frames, gt=gt, vos=SPEC, want_polygon=True)
    p = _reserved(m).run(frames, gt=gt, vos=dict(SPEC, rle=True), want_polygon=True)
    _same(p, poly, "want_polygon")
    assert torch.equal(p["mask"], plain["mask"]) and p["labels"] is None and np.array_equal(p["vos_counts"], plain["vos_counts"])
    _same_counts(p["label_rle"], fused, "want_polygon")


def test_plain_run_and_enqueue_without_lifetimes(scene):
    """run(gt=, vos=) with 'alive' / 'given' rows, and frame by frame through enqueue() / collect(); a later chunk without the key
    returns what it always did"""
    m, frames, gt = scene["m"], scene["frames"], scene["gt"]
    alive = np.ones((T, B), dtype=bool)
    alive[:, 2] = False
    alive[3:, 1] = False
    base = {"object_ids": IDS, "thrs": vos.THRS, "alive": alive}

    def started():
        tr = _reserved(m)
        tr.start(frames[0], [0, 1, 2], labels=gt[0], object_ids=IDS)
        return tr
    plain = started().run(frames, gt=gt, vos=base)
    lab = plain["labels"].cpu().numpy()
    assert lab.any() and not (lab == 3).any() and not (lab[3:] == 2).any()
    a = started().run(frames, gt=gt, vos=dict(base, rle=True))
    assert a["mask"] is None and a["labels"] is None and np.array_equal(a["vos_counts"], plain["vos_counts"])
    _same(dict(a, mask=plain["mask"]), plain, "run(gt=, vos=)")
    _decodes_to(a["label_rle"], lab, "run(gt=, vos=)")
    b = started().run(frames, vos={"object_ids": IDS, "alive": alive, "rle": True})
    assert "vos_counts" not in b and b["mask"] is None and b["labels"] is None
    _same_counts(b["label_rle"], a["label_rle"], "run(vos=) without gt")
    tr = started()
    for t in range(T):
        tr.enqueue(frames[t], vos={"object_ids": IDS, "alive": alive[t], "rle": {"cap": 700}})
    e = tr.collect()
    assert e["mask"] is None and e["labels"] is None and "vos_counts" not in e
    _decodes_to(e["label_rle"], lab, "enqueue()", cap=700)
    later = tr.run(frames[1:3], gt=gt[1:3], vos={"object_ids": IDS, "thrs": vos.THRS})
    assert "label_rle" not in later and later["labels"] is not None and later["mask"] is not None


def test_serial_and_both_pipeline_depths_agree(scene):
    frames, gt = scene["frames"], scene["gt"]
    mp = _model("sharp", "f16", B, "pipe")
    runs = {}
    for depth in (0, 1, 2):
        for key in (None, True, {"masks": True}):
            tr = _reserved(mp, pipeline=depth > 0)
            if depth:
                mp.set_pipeline(depth)
            try:
                runs[depth, str(key)] = tr.run(frames, gt=gt, vos=SPEC if key is None else dict(SPEC, rle=key))
            finally:
                if depth:
                    mp.set_pipeline(1)
    plain = runs[0, "None"]
    lab = plain["labels"].cpu().numpy()
    for depth in (0, 1, 2):
        what = "pipeline depth %d" % depth
        _same_run(dict(runs[depth, "None"], labels=None), plain, what + ", no key", masks=True)
        assert torch.equal(runs[depth, "None"]["labels"], plain["labels"])
        _same_run(runs[depth, "True"], plain, what)
        _same_run(runs[depth, "{'masks': True}"], plain, what + ", masks", masks=True)
        _decodes_to(runs[depth, "True"]["label_rle"], lab, what)
        _same_counts(runs[depth, "{'masks': True}"]["label_rle"], runs[0, "True"]["label_rle"], what)


def test_refusals_come_before_any_launch(scene):
    m, frames, gt = scene["m"], scene["frames"], scene["gt"]
    tr = _reserved(m)
    tr.start(frames[0], [0, 1, 2], labels=gt[0], object_ids=IDS)
    tr.collect()
    q = tr._fr
    torch.cuda.synchronize()
    before = q.dev.clone()
    ok = {"object_ids": IDS, "thrs": vos.THRS}
    bad = (dict(vos=dict(ok, rle={"cap": 0})), dict(vos=dict(ok, rle={"cap": H * W + 2})), dict(vos=dict(ok, rle={"size": 3})),
           dict(vos=dict(ok, rle=5)), dict(vos=dict(ok, rle={"labels": True})),                      # the label map needs gt
           dict(vos=dict(ok, rle=True), want_mask=False), dict(vos=ok),                              # without the key gt is required
           dict(vos=dict(ok, rle=True), rle=True), dict(gt=gt, vos=dict(ok, rle=True), rle=True),    # the top-level rle= stays refused
           dict(vos=dict(SPEC, rle=True)),                                                           # lifetimes without gt: vos['init']
           dict(gt=gt, vos=dict(SPEC, rle={"cap": -1})), dict(gt=gt[:2], vos=dict(ok, rle=True)))
    for kw in bad:
        with pytest.raises(ValueError):
            tr.run(frames, **kw)
        assert q.chunk.pending == 0 and not q.chunk.events and q.chunk.label_rle is None and tr.collect() is None, kw
    with pytest.raises(ValueError, match="own sizes"):                   # B videos of their own sizes
        tr.run([frames] * B, vos=dict(ok, rle=True))
    with pytest.raises(ValueError, match="own sizes"):
        tr.enqueue([frames[1]] * B, vos=dict(ok, rle=True))
    with pytest.raises(ValueError, match="shared"):                      # per-stream frames
        tr.enqueue(frames[:B], vos=dict(ok, rle=True))
    assert q.chunk.pending == 0 and q.chunk.label_rle is None and tr.collect() is None
    torch.cuda.synchronize()
    assert torch.equal(q.dev, before)                                   # the state block: nothing was launched
    # a chunk carries the key on every frame, at one cap, scored or not as its first frame is
    tr.enqueue(frames[1], vos=dict(ok, rle=True))
    torch.cuda.synchronize()
    after_one = q.dev.clone()
    for kw in (dict(), dict(vos=dict(ok, rle={"cap": 7})), dict(gt=gt[2], vos=dict(ok, rle=True)), dict(gt=gt[2], vos=ok)):
        with pytest.raises(ValueError):
            tr.enqueue(frames[2], **kw)
        assert q.chunk.pending == 1 and len(q.chunk.label_rle) == 1
    torch.cuda.synchronize()
    assert torch.equal(q.dev, after_one)
    assert tr.collect()["label_rle"]["n"].shape == (1, B)
    tr.enqueue(frames[2], gt=gt[2], vos=ok)
    torch.cuda.synchronize()
    after_two = q.dev.clone()
    for kw in (dict(gt=gt[3], vos=dict(ok, rle=True)), dict(vos=dict(ok, rle=True))):
        with pytest.raises(ValueError):
            tr.enqueue(frames[3], **kw)
    torch.cuda.synchronize()
    assert q.chunk.pending == 1 and q.chunk.label_rle is None and torch.equal(q.dev, after_two)
    assert "label_rle" not in tr.collect()
    # the rpn variant has no mask branch
    tp = DeviceTracker(_model("rpn", "f32", B), {k: v for k, v in HP.items() if k != "out_size"})
    tp.reserve(B, H, W)
    with pytest.raises(ValueError, match="mask branch"):
        tp.run(frames, vos=dict(ok, rle=True))
    assert tp.collect() is None
