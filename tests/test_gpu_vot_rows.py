"""smk_vot_step_rows_dev (preproc.vot_step_rows) against its host twin, BIT for bit: the two recorded pair sets of
tests/golden/vot_overlap.npz as one dataset of 24 videos of 29 frames that move through B = 1, 3 and 32 slots at different local
frames, the bounds of a slot read from its state record (two sizes); the fallback polygons; the refusals."""
import numpy as np
import pytest
import torch

import tracker_state_ref as R
from siammask_amd import _lib, preproc
from test_vot_host import BOUNDS, same_bits
from test_vot_rows_host import NV, SENT_CNT, SENT_CODE, SENT_OV, SENT_POLY, SENT_START, SKIP, T, cut, host_step, tables

pytestmark = pytest.mark.gpu
V, N = 2 * NV, 2 * NV * T
KEYS = ("vstate", "code", "poly", "overlap", "counts")


def _dataset():
    a, b = cut("%dx%d" % BOUNDS[0]), cut("%dx%d" % BOUNDS[1])
    wh = np.array([BOUNDS[0]] * NV + [BOUNDS[1]] * NV, dtype=np.int32)           # per video
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]]), wh


def _schedule(B):
    """slot b runs videos b, b + B, ... back to back behind b % 4 idle steps -> int [G,B,2] = (video, frame), -1 where idle"""
    cols = []
    for b in range(B):
        col = [(-1, -1)] * (b % 4)
        for v in range(b, V, B):
            col += [(v, t) for t in range(1, T)]
        cols.append(col)
    G = max(len(c) for c in cols)
    return np.array([c + [(-1, -1)] * (G - len(c)) for c in cols]).transpose(1, 0, 2)


def _state(im_wh):
    rec = np.zeros(len(im_wh), dtype=R.STREAM_DTYPE)
    rec["im_w"], rec["im_h"] = np.asarray(im_wh)[:, 0], np.asarray(im_wh)[:, 1]
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()


def _dev_tables(tab):
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in tab.items()}


def _step(dev, pred, gt_dev, state, row, vid, t, live, skip=SKIP, adv=None, start_out=None, counts=True):
    t64 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    return preproc.vot_step_rows(t64(pred), gt_dev, state, row, vid, t, live, skip, dev["vstate"], dev["code"], dev["poly"], dev["overlap"],
                                 dev["start_out"] if start_out is None else start_out, adv_rows=t64(adv),
                                 counts=dev["counts"] if counts else None)


@pytest.mark.parametrize("B", [1, 3, 32])
def test_entry_equals_the_host_twin(B):
    gt, pred, ov, wh = _dataset()
    sched = _schedule(B)
    G = sched.shape[0]
    want, dev = tables(N, V, B), _dev_tables(tables(N, V, B))
    gt_dev = torch.from_numpy(gt).cuda()
    starts = torch.full((G, B), SENT_START, dtype=torch.int32, device="cuda")
    want_starts = np.full((G, B), SENT_START, np.int32)
    states = {}
    for g in range(G):
        live = sched[g, :, 0] >= 0
        vid, t = np.where(live, sched[g, :, 0], 0), np.where(live, sched[g, :, 1], 1)
        row = np.where(live, T * vid + t, 0)                            # (a slot that is not live addresses row 0)
        im_wh = np.where(live[:, None], wh[vid], (17, 9)).astype(np.int32)
        key = im_wh.tobytes()
        if key not in states:
            states[key] = _state(im_wh)
        want["start_out"] = want_starts[g]
        assert host_step(pred[row], gt, im_wh, row, vid, t, live, want) == 0, _lib.lib().smk_last_error()
        _step(dev, pred[row], gt_dev, states[key], row, vid, t, live, start_out=starts[g])
    got = {k: dev[k].cpu().numpy() for k in KEYS}
    for k in ("vstate", "code", "counts"):
        assert np.array_equal(got[k], want[k]), k
    assert same_bits(got["overlap"], want["overlap"]) and np.array_equal(got["poly"].view(np.uint64), want["poly"].view(np.uint64))
    assert np.array_equal(starts.cpu().numpy(), want_starts)
    # what the twin left untouched is untouched: frame 0 of every video, the rows of skipped / init frames, idle slots' rows
    code = got["code"].reshape(V, T)
    assert (code[:, 0] == SENT_CODE).all() and (code[:, 1:] != SENT_CODE).all()
    off = ~np.isin(got["code"], (-1, 2))
    assert (got["poly"][off] == SENT_POLY).all() and (got["overlap"][off] == SENT_OV).all() and (got["counts"][off] == SENT_CNT).all()
    assert (want_starts == SENT_START).any() == (B != 1) and len(states) >= 2
    # both sizes were really read from the records: the recorded overlaps of both sets, and losses in both
    on = ~off
    assert same_bits(got["overlap"][on], ov[on]) and (got["vstate"][:NV, 1] > 0).any() and (got["vstate"][NV:, 1] > 0).any()
    assert set(got["counts"][on, 3].tolist()) == {0, 1, 2, 3, 4} and np.isnan(got["overlap"][on]).any()


def test_fallback_polygons_and_no_prediction():
    W, H, n = 64, 48, 6
    gt, pred, _, _ = _dataset()
    rng = np.random.default_rng(11)
    rows = np.zeros((n, 12))
    rows[:, :8], rows[:, 9] = pred[1:1 + n], [1, 0, 1, -1, 0, 1]
    adv = rng.uniform(0, 40, (n, 16))
    adv[:, 10:12], adv[:, 2:4] = rng.uniform(4.5, 30, (n, 2)), np.round(rng.uniform(10, 30, (n, 2)))
    row, vid, one, live = T * np.arange(n) + 1, np.arange(n), [1] * n, [True] * n
    state, gt_dev = _state([(W, H)] * n), torch.from_numpy(gt).cuda()
    for p, a, cnt in ((rows, adv, True), (None, adv, True), (rows, None, False), (rows[:, :8].reshape(n, 4, 2), None, True)):
        want, dev = tables(N, V, n), _dev_tables(tables(N, V, n))
        p_host = None if p is None else p.reshape(n, -1)
        assert host_step(p_host, gt, [(W, H)] * n, row, vid, one, live, want, adv=a, counts=cnt) == 0
        _step(dev, p, gt_dev, state, row, vid, one, live, adv=a, counts=cnt)
        for k in KEYS + ("start_out",):
            assert np.array_equal(dev[k].cpu().numpy().view(np.uint8), want[k].view(np.uint8)), k


def test_refusals_leave_the_outputs_unchanged():
    gt, pred, _, _ = _dataset()
    gt_dev, state = torch.from_numpy(gt).cuda(), _state([BOUNDS[0]] * 2)
    dev = _dev_tables(tables(N, V, 2))
    ref = {k: v.clone() for k, v in dev.items()}
    ok = dict(row=[1, 30], vid=[0, 1], t=[1, 1], live=[True, True], skip=SKIP)

    def call(**bad):
        kw = dict(ok, **bad)
        _step(dev, pred[[1, 30]], gt_dev, state, kw["row"], kw["vid"], kw["t"], kw["live"], skip=kw["skip"])

    for bad in (dict(row=[N, 30]), dict(row=[-1, 30]), dict(vid=[V, 1]), dict(vid=[-1, 1]), dict(t=[0, 1]), dict(t=[1, -2]),
                dict(vid=[1, 1]), dict(row=[30, 30]), dict(skip=0), dict(skip=65536)):
        with pytest.raises(_lib.SmkError):
            call(**bad)
        assert b"smk_vot_step_rows_dev" in _lib.lib().smk_last_error()
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    args = lambda **k: dict(dict(pred=f64(2, 8), gt=gt_dev, state=state, row=[1, 30], vid=[0, 1], t=[1, 1], live=[True, True], skip=SKIP,
                                 vstate=dev["vstate"], code=dev["code"], poly=dev["poly"], overlap=dev["overlap"],
                                 start_out=dev["start_out"]), **k)
    for bad in (dict(row=[1]), dict(row=list(range(33)), vid=list(range(33)), t=[1] * 33, live=[True] * 33), dict(pred=f64(3, 8)),
                dict(pred=f64(2, 9)), dict(pred=None), dict(gt=f64(N, 4)), dict(state=state[:8]), dict(code=dev["code"][:-1]),
                dict(poly=dev["poly"][:, :4]), dict(overlap=dev["overlap"].double()), dict(start_out=dev["start_out"][:1]),
                dict(vstate=dev["vstate"].reshape(-1)), dict(counts=dev["counts"][:5]), dict(adv_rows=f64(2, 12))):
        with pytest.raises(ValueError):
            preproc.vot_step_rows(**args(**bad))
    torch.cuda.synchronize()
    assert all(torch.equal(dev[k], ref[k]) for k in dev)
    # no live slot: accepted, nothing written; then the valid call writes
    call(live=[False, False])
    torch.cuda.synchronize()
    assert all(torch.equal(dev[k], ref[k]) for k in dev)
    call()
    assert (dev["code"][[1, 30]] != SENT_CODE).all().item() and (dev["start_out"] != SENT_START).all().item()
