"""Frames enter as JPEG, the device half: preproc.jpeg_decode -- one memset and three launches for N files of mixed
sizes and samplings -- against the pixels PIL (libjpeg-turbo) decoded (tests/golden/jpeg_cases.npz), into pitched views of a
pre-filled canvas; a damaged file beside good ones; jpeg.Video and jpeg.videos under dataset.run_videos against the same run from
pre-decoded tensors.  Every comparison is ==."""
import hashlib

import numpy as np
import pytest
import torch

from siammask_amd import dataset, jpeg, preproc
from siammask_amd.tracker import DeviceTracker
from test_gpu_freerun import _model
from test_gpu_tracker import HP
from test_jpeg_host import CUT_CASE, CUT_K, FILES, G, NAMES, PIX

pytestmark = pytest.mark.gpu
FILL = 0xA5
_cache = {}


def _canvas_views():
    """one buffer pre-filled with 0xA5 and, per case, a pitched view [h,w,3] into it at an odd address with a gap behind every row
    and every image -> (buffer, views, a bool mask of the bytes that belong to a view)"""
    offs, pos = [], 1
    for p in PIX:
        h, w = p.shape[:2]
        pitch = 3 * w + 5 + (h % 3)
        offs.append((pos, pitch))
        pos += h * pitch + 11
    buf = torch.full((pos,), FILL, dtype=torch.uint8, device="cuda")
    inside = np.zeros(pos, dtype=bool)
    views = []
    for p, (o, pitch) in zip(PIX, offs):
        h, w = p.shape[:2]
        views.append(torch.as_strided(buf, (h, w, 3), (pitch, 3, 1), storage_offset=o))
        for y in range(h):
            inside[o + y * pitch:o + y * pitch + 3 * w] = True
    return buf, views, inside


def test_all_cases_in_one_call_into_pitched_views():
    buf, views, inside = _canvas_views()
    frames, meta = preproc.jpeg_decode(FILES, out=views)
    assert len(frames) == 112 and all(f is v for f, v in zip(frames, views))
    m = meta.cpu().numpy()
    assert m.shape == (112, 4) and m.dtype == np.int32
    assert (m[:, 0] == 0).all(), "status of %s" % [NAMES[i] for i in np.flatnonzero(m[:, 0])]
    assert (m[:, 1:3] == np.asarray([p.shape[:2] for p in PIX])).all()
    assert (m[:, 3] == [jpeg.parse(f).desc[jpeg.NSEG] for f in FILES]).all() and m[:, 3].max() == 15
    bad = [NAMES[i] for i, (v, p) in enumerate(zip(views, PIX)) if not (v.cpu().numpy() == p).all()]
    assert not bad, "%d images differ from their fixtures: %s" % (len(bad), bad[:8])
    first = buf.cpu().numpy()
    assert (first[~inside] == FILL).all(), "bytes outside the images were written"
    # a second call over the same buffers (the workspace holds the first call's coefficients and status words): the same bytes
    frames, meta2 = preproc.jpeg_decode(FILES, out=views)
    assert (buf.cpu().numpy() == first).all() and (meta2.cpu().numpy() == m).all()


def test_frames_of_one_allocation_and_the_tennis_hashes():
    files = [G["tennis0"].tobytes(), G["tennis1"].tobytes(), FILES[NAMES.index("17x23_noise_422_q80")]]
    frames, meta = preproc.jpeg_decode(files)
    assert (meta[:, 0] == 0).all().item()
    for k in range(2):
        f = frames[k]
        assert f.is_cuda and f.dtype == torch.uint8 and f.is_contiguous() and tuple(f.shape) == tuple(G["tennis_hw"]) + (3,)
        got = f.cpu().numpy()
        y, x = (int(v) for v in G["tennis_crop_yx"])
        assert (got[y:y + 64, x:x + 64] == G["tennis_crop"][k]).all()              # (the crop is there for diagnosis)
        assert hashlib.sha256(got.tobytes()).hexdigest() == str(G["tennis_sha256"][k])
    assert (frames[2].cpu().numpy() == PIX[NAMES.index("17x23_noise_422_q80")]).all()
    assert frames[0].untyped_storage().data_ptr() == frames[2].untyped_storage().data_ptr()      # views of one allocation
    _cache["tennis"] = [frames[0].clone(), frames[1].clone()]


def test_a_damaged_file_reports_its_status_and_disturbs_nothing():
    i, j, c = NAMES.index("31x15_noise_420_rst1"), NAMES.index("9x33_smooth_444_q100"), NAMES.index(CUT_CASE)
    cut = FILES[c][:len(FILES[c]) * CUT_K // 17]                      # (the sanitizer program of test_jpeg_host.py has run this one)
    _, want = jpeg.decode_host(cut, want_meta=True)
    assert want[0] == jpeg.ST_CUT
    frames, meta = preproc.jpeg_decode([FILES[i], cut, FILES[j]])
    m = meta.cpu().numpy()
    assert m[:, 0].tolist() == [0, int(want[0]), 0] and m[1, 1:3].tolist() == [40, 72]
    assert (frames[0].cpu().numpy() == PIX[i]).all() and (frames[2].cpu().numpy() == PIX[j]).all()
    assert tuple(frames[1].shape) == (40, 72, 3)
    with pytest.raises(jpeg.Unsupported):
        preproc.jpeg_decode([FILES[i], G["progressive"].tobytes()])
    with pytest.raises(ValueError):
        preproc.jpeg_decode([FILES[i]], out=[torch.empty((15, 31, 3), dtype=torch.uint8, device="cuda").permute(1, 0, 2)])
    with pytest.raises(ValueError):
        preproc.jpeg_decode([])


def test_video_window_equals_the_batch_decode():
    files = [FILES[NAMES.index("40x72_%s_%s" % (k, e))] for k, e in (("noise", "444_q80"), ("smooth", "422_q80"), ("noise", "420_q80"),
                                                                    ("smooth", "420_rst1"), ("noise", "420_opt_q30"), ("smooth", "444_q100"),
                                                                    ("noise", "grey_q85"))]
    batch, _ = preproc.jpeg_decode(files)
    v = jpeg.Video(files, window=3)
    assert len(v) == 7
    for t in range(7):
        assert torch.equal(v[t], batch[t]), t
    assert v.stats == {"calls": 3, "frames": 7}
    assert torch.equal(v[1], batch[1]) and v.stats["calls"] == 4      # outside the two resident windows: decoded again


def _videos():
    """three tiny videos as files and as the pixels PIL decoded: the two tennis frames alternating (854 x 480), four 40 x 72
    fixtures of four encodings, and the tennis frames again"""
    t = [G["tennis0"].tobytes(), G["tennis1"].tobytes()]
    small = [i for i, n in enumerate(NAMES) if n.startswith("40x72_smooth")][:4]
    files = [[t[0], t[1], t[0]], [FILES[i] for i in small], [t[1], t[0]]]
    tp = _cache.get("tennis") or preproc.jpeg_decode(t)[0]
    pix = [[tp[0], tp[1], tp[0]], [torch.from_numpy(PIX[i].copy()).cuda() for i in small], [tp[1], tp[0]]]
    return files, pix


def test_run_videos_from_jpeg_equals_the_run_from_tensors():
    files, pix = _videos()
    for k in range(2):                                                # (the tensors of the tennis frames are the checked pixels)
        assert hashlib.sha256(pix[0][k].cpu().numpy().tobytes()).hexdigest() == str(G["tennis_sha256"][k])
    pos = np.array([[430.0, 250.0], [36.0, 20.0], [430.0, 250.0]])
    sz = np.array([[90.0, 120.0], [24.0, 16.0], [90.0, 120.0]])
    B = 2
    want = dataset.run_videos(DeviceTracker(_model("sharp", "f16", B), HP), pix, pos, sz, B=B)
    loaders = jpeg.videos(files, B, order="longest", window=2)
    got = dataset.run_videos(DeviceTracker(_model("sharp", "f16", B), HP), loaders, pos, sz, B=B)
    assert loaders[0].stats["misses"] == 0 and loaders[0].stats["frames"] == 9
    assert got["steps"] == want["steps"] and len(got["videos"]) == 3
    for v, (a, b) in enumerate(zip(got["videos"], want["videos"])):
        assert a["size"] == b["size"] == tuple(pix[v][0].shape[:2]) and a["slot"] == b["slot"]
        for k in ("target_pos", "target_sz", "score", "best_id", "n", "area"):
            assert a[k].tobytes() == b[k].tobytes(), "video %d: %s" % (v, k)
        assert len(a["rle"]) == len(b["rle"]) == len(files[v]) - 1
        for t, (x, y) in enumerate(zip(a["rle"], b["rle"])):
            assert x is not None and y is not None and np.array_equal(x, y), "video %d frame %d: counts" % (v, t + 1)
