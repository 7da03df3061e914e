"""The label maps of a VOS dataset as PNG files (dataset.run_vos(png=True)) on the synthetic set of
test_gpu_vos_dataset.py: its videos 1, 2 and 3 -- three videos of two sizes, 1, 3 and 1 objects -- through B = 4 slots with a chunk
boundary inside the run.  Every file decodes to the label map the video's run-length codes decode to, everything else of the run
equals the run without png= exactly, and a cap below a frame's size drops exactly the frames that exceed it.  The private _png_out of
enqueue() is refused without _vos_v and with rows of the wrong kind, before anything is launched."""
import numpy as np
import pytest

from siammask_amd import dataset, png, rle
from test_gpu_vos_dataset import B, CAP, _dataset, _same, _tracker

pytestmark = pytest.mark.gpu
CHUNK = 3
_cache = {}


def _videos():
    return _dataset()[1:4]


def _runs():
    if "runs" not in _cache:
        plain = dataset.run_vos(_tracker(), _videos(), B=B, order="given", cap=CAP, chunk=CHUNK)
        assert plain["steps"] > CHUNK                                   # a chunk boundary lies inside the run
        _cache["runs"] = (plain, dataset.run_vos(_tracker(), _videos(), B=B, order="given", cap=CAP, chunk=CHUNK, png=True,
                                                 png_cap=png.worst_cap(200, 264)))  # (the canvas: no stream can be cut)
    return _cache["runs"]


def test_every_file_decodes_to_the_label_map_of_the_codes():
    plain, res = _runs()
    assert len(set(d["size"] for d in res["videos"])) == 2 and len(res["videos"]) == 3
    labelled = 0
    for v, d in enumerate(res["videos"]):
        h, w = d["size"]
        T = len(d["label_rle"])
        assert len(d["label_png"]) == T and d["png_bytes"].dtype == np.int32 and d["png_bytes"].shape == (T,)
        for t in range(T):
            f = d["label_png"][t]
            assert isinstance(f, bytes) and f[:8] == png.SIGNATURE, (v, t)
            lab = rle.labels_decode(d["label_rle"][t], h, w)
            assert np.array_equal(png.decode(f), lab), (v, t)
            assert d["png_bytes"][t] == len(png.encode_host(lab)), (v, t)
            labelled += int((lab > 0).sum())
    assert labelled > 0                                                 # the maps are not all background
    assert "label_png" not in plain["videos"][0] and "png_bytes" not in plain["videos"][0]


def test_the_rest_of_the_run_is_the_run_without_png():
    plain, res = _runs()
    _same(res["videos"], plain["videos"], "png=True")
    assert res["steps"] == plain["steps"] and res["efficiency"] == plain["efficiency"]
    strip = lambda ev: [{k: (np.asarray(x).tolist() if hasattr(x, "shape") else x) for k, x in e.items()} for e in ev]
    assert strip(res["events"]) == strip(plain["events"])
    for a, b in zip(res["videos"], plain["videos"]):
        assert a["slots"] == b["slots"] and a["first_step"] == b["first_step"] and a["size"] == b["size"]


def test_a_small_cap_drops_exactly_the_frames_that_exceed_it_and_a_palette_makes_indexed_files():
    _, res = _runs()
    sizes = np.concatenate([d["png_bytes"] for d in res["videos"]])
    cap = int(np.sort(sizes)[sizes.size // 2])                          # the median: some frames fit, some do not
    assert sizes.min() <= cap < sizes.max()
    pal = png.davis_palette()
    small = dataset.run_vos(_tracker(), _videos(), B=B, order="given", cap=CAP, chunk=CHUNK, png=True, png_cap=cap, png_palette=pal)
    dropped = 0
    for d, full in zip(small["videos"], res["videos"]):
        assert np.array_equal(d["png_bytes"], full["png_bytes"])
        for t, f in enumerate(d["label_png"]):
            assert (f is None) == (d["png_bytes"][t] > cap), t
            if f is None:
                dropped += 1
                continue
            m, got_pal = png.decode(f, want_palette=True)
            assert np.array_equal(got_pal, pal) and np.array_equal(m, png.decode(full["label_png"][t]))
    assert 0 < dropped < sizes.size


def test_the_rules_of_the_private_png_out():
    import torch
    vids = _videos()
    tr = _tracker()
    tr.reserve(B, 200, 264)
    f = [vids[0]["frames"][0], vids[1]["frames"][0]]
    tr.start(f, [0, 1], pos=[(236, 176), (70, 52)], sz=[(64, 46), (48, 36)])
    fed = [vids[0]["frames"][1], vids[1]["frames"][1]] + [torch.zeros((200, 264, 3), dtype=torch.uint8, device="cuda")] * 2
    rows = lambda cap, dt=torch.uint8: (torch.empty((B, cap), dtype=dt, device="cuda"), torch.empty((B, 4), dtype=torch.int32, device="cuda"))
    vv = (200 * 264 + 1, [[0], [1]], [(264, 200), (131, 97)], [5, 1, 0, 0], None, None, None, None)     # (no code can be cut)
    with pytest.raises(ValueError, match="_png_out"):                   # only with _vos_v
        tr.enqueue(fed, _png_out=rows(64))
    for bad in (rows(0), rows(png.worst_cap(200, 264) + 1), rows(64, torch.int32), (rows(64)[0], rows(64)[0]), rows(64)[:1],
                (rows(64)[0].cpu(), rows(64)[1]), (torch.empty((B + 1, 64), dtype=torch.uint8, device="cuda"), rows(64)[1])):
        with pytest.raises(ValueError, match="_png_out"):
            tr.enqueue(fed, _vos_v=vv, _png_out=bad)
    out, meta = rows(png.worst_cap(200, 264))
    assert tr.enqueue(fed, _vos_v=vv, _png_out=(out, meta)) == 0        # nothing above was enqueued
    res = tr.collect()
    r, m = res["label_rle"], meta.cpu().numpy()
    assert m[2:, 0].tolist() == [0, 0] and m[:2, 2:].tolist() == [[200, 264], [97, 131]]
    for b, (h, w) in enumerate(((200, 264), (97, 131))):
        c = r["counts"][0, b, :int(r["n"][0, b])].cpu().numpy().view(np.uint32).astype(np.int64)
        lab = rle.labels_decode([c], h, w)
        assert np.array_equal(png.decode(png.to_png(out[b, :m[b, 0]].cpu().numpy(), h, w)), lab), b
