"""Label maps deflated on the device (smk_png_encode / smk_vos_png_v / smk_vos_png_dev_v, preproc.png_encode / vos_png_v /
vos_png_dev_v).  Everything is compared with ==.  The byte source against its CPU twin (png.encode_host_v, which
tests/test_png_host.py pins against zlib) on that file's shapes and contents, B = 3 planes per call, plus one shape whose scan
takes two chunks of 1024 words.  The fused forms against png.encode_host over the label map that the codes of the existing
preproc.vos_rle_v decode to: a 96 x 80 canvas, B = 4 slots, the groups {0, 1} at 70 x 48 and {2} at 33 x 65, slot 3 in no group."""
import numpy as np
import pytest
import torch

import tracker_state_ref as R
from siammask_amd import png, preproc, rle
from test_gpu_vos import _objects
from test_png_host import CONTENTS, SHAPES, make_map

pytestmark = pytest.mark.gpu
FILL = 0xA5
TWO_CHUNKS = (300, 260)                                                  # N = 300 * 261 = 78300 positions: 1224 words
CALLS = (("zero", "random", "rows"), ("boxes", "rows", "random"))


def _filled(B, cap):
    return (torch.full((B, cap), FILL, dtype=torch.uint8, device="cuda"),
            torch.full((B, 16), FILL, dtype=torch.uint8, device="cuda").view(torch.int32))


@pytest.mark.parametrize("kinds", CALLS)
def test_png_encode_equals_the_host_twin(kinds):
    assert set(k for c in CALLS for k in c) == set(CONTENTS)
    for h, w in SHAPES + [TWO_CHUNKS]:
        maps = np.stack([make_map(h, w, k) for k in kinds])
        cap = png.worst_cap(h, w)
        want, wmeta = png.encode_host_v(maps, cap=cap)
        out, meta = _filled(3, cap)
        preproc.png_encode(torch.from_numpy(maps).cuda(), cap=cap, out=out, meta=meta)
        got, gmeta = out.cpu().numpy(), meta.cpu().numpy()
        assert np.array_equal(gmeta, wmeta), (h, w, gmeta, wmeta)
        for b in range(3):
            n = int(wmeta[b, 0])
            assert np.array_equal(got[b, :n], want[b, :n]) and (got[b, n:] == FILL).all(), (h, w, kinds[b])
        preproc.png_encode(torch.from_numpy(maps).cuda(), cap=cap, out=out, meta=meta)      # over the filled workspace: the same bytes
        assert np.array_equal(out.cpu().numpy(), got) and np.array_equal(meta.cpu().numpy(), gmeta)
        # a cap one byte under the longest stream: its row ends at cap, the next row's first byte is its own, meta tells the truth
        short = int(wmeta[:, 0].max()) - 1
        if short >= 1:
            out2, meta2 = _filled(3, short)
            preproc.png_encode(torch.from_numpy(maps).cuda(), cap=short, out=out2, meta=meta2)
            got2 = out2.cpu().numpy()
            assert np.array_equal(meta2.cpu().numpy(), wmeta), (h, w)
            for b in range(3):
                n = min(int(wmeta[b, 0]), short)
                assert np.array_equal(got2[b, :n], want[b, :n]) and (got2[b, n:] == FILL).all(), (h, w, kinds[b], "short")
    assert (TWO_CHUNKS[0] * (TWO_CHUNKS[1] + 1) + 63) // 64 > 1024


def test_png_encode_takes_a_single_map_and_the_default_cap():
    m = make_map(48, 70, "boxes")
    out, meta = preproc.png_encode(torch.from_numpy(m).cuda())
    assert tuple(out.shape) == (1, png.default_cap(48, 70)) and meta.cpu().numpy()[0].tolist()[2:] == [48, 70]
    n = int(meta[0, 0])
    assert out[0, :n].cpu().numpy().tobytes() == png.encode_host(m)
    assert np.array_equal(png.decode(png.to_png(out[0, :n].cpu().numpy(), 48, 70, png.davis_palette())), m)
    mask = (m > 0).astype(np.uint8) * 255                               # a 0 / 255 mask is another use of it
    out, meta = preproc.png_encode(torch.from_numpy(mask).cuda())
    assert out[0, :int(meta[0, 0])].cpu().numpy().tobytes() == png.encode_host(mask)
    with pytest.raises(ValueError, match="cap"):
        preproc.png_encode(torch.from_numpy(m).cuda(), cap=png.worst_cap(48, 70) + 1)
    with pytest.raises(ValueError, match="cap"):
        preproc.png_encode(torch.from_numpy(m).cuda(), cap=0)


# ---- the fused forms ---------------------------------------------------------------------------------------------------------------------
SEG = 0.35
B, CW, CH = 4, 96, 80
GROUPS = [[0, 1], [2]]
SIZES = [(70, 48), (33, 65)]                                            # (w, h)
IDS = np.array([9, 200, 4, 17])
CAP = png.worst_cap(CH, CW)
_cache = {}


def _setup():
    if "setup" not in _cache:
        rng = np.random.default_rng(322)
        logits = torch.from_numpy(rng.normal(0, 3, (B, 127 * 127)).astype(np.float32)).cuda()
        bbs = [[0.0, 0.0, 127.0, 127.0]] * B
        for slots, (w, h) in zip(GROUPS, SIZES):
            for b, bb in zip(slots, _objects(rng, len(slots), w, h)[1]):
                bbs[b] = bb
        _cache["setup"] = (logits, bbs)
    return _cache["setup"]


def _init(g, seed=5):
    w, h = SIZES[g]
    rng = np.random.default_rng(seed + g)
    vals = np.array([0, 251] + [int(IDS[b]) for b in GROUPS[g]], dtype=np.uint8)
    return torch.from_numpy(vals[rng.integers(0, len(vals), (h, w))]).cuda()


def _want(kw):
    """per group the stream of the label map the codes of vos_rle_v decode to, or None for a group that is not live"""
    logits, bbs = _setup()
    c, m = preproc.vos_rle_v(logits, bbs, (CW, CH), GROUPS, SIZES, IDS, seg_thr=SEG, cap=CW * CH + 1, **kw)
    c, m = c.cpu().numpy().view(np.uint32), m.cpu().numpy()
    live = kw.get("live") or [True] * len(GROUPS)
    want = []
    for g, slots in enumerate(GROUPS):
        w, h = SIZES[g]
        if not live[g]:
            want.append(None)
            continue
        lab = rle.labels_decode([c[b, :m[b, 0]].astype(np.int64) for b in slots], h, w)
        want.append((png.encode_host(lab), lab))
    return want


def _compare(out, meta, want, cap=CAP, what=""):
    got, gm = out.cpu().numpy(), meta.cpu().numpy()
    lead = {min(s): g for g, s in enumerate(GROUPS)}
    for b in range(B):
        g = lead.get(b)
        if g is None or want[g] is None:
            size = next(([SIZES[k][1], SIZES[k][0]] for k, s in enumerate(GROUPS) if b in s), [CH, CW])
            assert gm[b].tolist() == [0, 0] + size and (got[b] == FILL).all(), (what, b, gm[b])
            continue
        z, lab = want[g]
        w, h = SIZES[g]
        n = min(len(z), cap)
        assert gm[b, 0] == len(z) and gm[b, 2:].tolist() == [h, w], (what, b, gm[b], len(z))
        assert got[b, :n].tobytes() == z[:n] and (got[b, n:] == FILL).all(), (what, b)
        if len(z) <= cap:
            assert np.array_equal(png.decode(png.to_png(got[b, :n], h, w)), lab)
    return gm


def _members(*on):
    return [b in on for b in range(B)]


def test_vos_png_v_equals_the_host_twin_over_the_decoded_label_planes():
    logits, bbs = _setup()
    args = (logits, bbs, (CW, CH), GROUPS, SIZES, IDS)
    cases = [("all alive", {}),
             ("one object given", dict(alive=_members(0, 2), given=_members(1), init=[_init(0), None])),
             ("group 1 not live", dict(live=[True, False])),
             ("group 0 not live", dict(live=[False, True]))]
    for what, kw in cases:
        want = _want(kw)
        out, meta = _filled(B, CAP)
        preproc.vos_png_v(*args, seg_thr=SEG, cap=CAP, out=out, meta=meta, **kw)
        gm = _compare(out, meta, want, what=what)
        if what == "all alive":
            assert all(len(np.unique(lab)) >= 2 for _, lab in want)     # no map is one value
            assert gm[0, 1] > 48 and gm[2, 1] > 65                      # more runs than rows: objects cut the rows
            first = (out.cpu().numpy(), gm)
            preproc.vos_png_v(*args, seg_thr=SEG, cap=CAP, out=out, meta=meta, **kw)          # over the filled workspace: the same bytes
            assert np.array_equal(out.cpu().numpy(), first[0]) and np.array_equal(meta.cpu().numpy(), first[1])
            short = int(gm[:, 0].max()) - 1                             # one byte short of the longest stream
            out2, meta2 = _filled(B, short)
            preproc.vos_png_v(*args, seg_thr=SEG, cap=short, out=out2, meta=meta2)
            assert np.array_equal(_compare(out2, meta2, want, cap=short, what="short cap"), gm)
        if what == "one object given":
            assert (want[0][1] == 2).any()                              # the given object carries pixels


@pytest.mark.parametrize("use_head", [False, True])
def test_the_state_block_form_equals_the_host_map_form(use_head):
    logits, bbs = _setup()
    rng = np.random.default_rng(78)
    S, ms = 5, 63 if use_head else 127
    init = [_init(0), None]
    given, alive = _members(1), _members(0, 2)
    for slot in (0, 1):
        rec = np.zeros(B, dtype=R.STREAM_DTYPE)
        for slots, (w, h) in zip(GROUPS, SIZES):
            for b in slots:
                rec["inv_map"][b, slot] = preproc.invert_affine(preproc.crop_back_map(bbs[b], (w, h)))
        rec["inv_map"][:, 1 - slot] = np.nan
        dyx = rng.integers(0, S, (B, 2))
        rec["delta_yx"][:, slot] = dyx
        rec["delta_yx"][:, 1 - slot] = 3
        block = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * B, np.uint8)])).cuda()
        if use_head:
            head = torch.from_numpy(rng.normal(0, 3, (B, ms * ms, S, S)).astype(np.float32)).cuda()
            rows = torch.stack([head[b, :, dyx[b, 0], dyx[b, 1]] for b in range(B)]).contiguous()
        else:
            head, rows = None, logits
        out, meta = _filled(B, CAP)
        preproc.vos_png_dev_v(None if use_head else logits, block, slot, (CW, CH), GROUPS, SIZES, IDS, alive=alive, given=given,
                              init=init, seg_thr=SEG, head=head, mask_size=ms, cap=CAP, out=out, meta=meta)
        out2, meta2 = _filled(B, CAP)
        preproc.vos_png_v(rows, bbs, (CW, CH), GROUPS, SIZES, IDS, alive=alive, given=given, init=init, seg_thr=SEG, cap=CAP,
                          out=out2, meta=meta2)
        assert torch.equal(meta, meta2) and torch.equal(out, out2), (slot, use_head)
        gm = meta.cpu().numpy()
        assert gm[0, 0] > 0 and gm[2, 0] > 0 and gm[1, 0] == 0 and gm[3].tolist() == [0, 0, CH, CW]
        # ... and decodes to the planes of the existing state-block entry
        c, m = preproc.vos_rle_dev_v(None if use_head else logits, block, slot, (CW, CH), GROUPS, SIZES, IDS, alive=alive, given=given,
                                     init=init, seg_thr=SEG, head=head, mask_size=ms, cap=CW * CH + 1)
        c, m = c.cpu().numpy().view(np.uint32), m.cpu().numpy()
        for slots, (w, h) in zip(GROUPS, SIZES):
            lab = rle.labels_decode([c[b, :m[b, 0]].astype(np.int64) for b in slots], h, w)
            n = int(gm[min(slots), 0])
            assert np.array_equal(png.decode(png.to_png(out[min(slots), :n].cpu().numpy(), h, w)), lab)
