"""COCO run lengths on the device: smk_rle_encode (preproc.rle_encode) and smk_paste_rle_dev (preproc.paste_rle) against the numpy
restatement of the pinned semantics (tests/rle_ref.py, held against the reference's maskApi.c by tools/make_rle_golden.py).
Counts, m and area are integers: everything is compared EXACTLY, no tolerance appears in this file.  Both byte-source forms of
smk_rle_encode (smk_test_rle_encode chooses one) are held to the same counts."""
import numpy as np
import pytest
import torch

import rle_ref
from siammask_amd import preproc, rle
from test_gpu_iou import _state, _streams

pytestmark = pytest.mark.gpu
# 257 x 300 = 77 100 px > 65 536: rle_scan takes a second chunk of 1024 words; 63 x 65 and 37 x 300: a ragged last word and a ragged
# last block of 64 columns; 64 x 1 / 1 x 64: exactly one word; 4 x 256: a % 64 == 0 with many columns per word
SHAPES = [(1, 1), (1, 64), (64, 1), (63, 65), (37, 300), (4, 256), (257, 300)]


def _ellipse(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return ((((y - 0.47 * h) / max(0.3 * h, 0.6)) ** 2 + ((x - 0.55 * w) / max(0.35 * w, 0.6)) ** 2) <= 1.0).astype(np.uint8)


def _at(h, w, js):
    """the mask whose transitions are exactly at the column-major positions js (those below a)"""
    f = np.zeros(h * w, dtype=np.uint8)
    for j in js:
        if j < h * w:
            f[j:] ^= 1
    return np.ascontiguousarray(f.reshape(w, h).T)


def _masks(h, w):
    """name -> uint8 [h,w] of 0 / 1"""
    first, last = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    first[0, 0], last[-1, -1] = 1, 1
    return {"empty": np.zeros((h, w), np.uint8), "full": np.ones((h, w), np.uint8), "first": first, "last": last,
            "checker": (np.add.outer(np.arange(h), np.arange(w)) % 2 == 0).astype(np.uint8), "ellipse": _ellipse(h, w),
            "at_words": _at(h, w, (63, 64, 65535, 65536)), "at_63": _at(h, w, (63,)), "at_64": _at(h, w, (64,))}


@pytest.fixture(scope="module")
def want():
    """(h, w, name) -> (mask, counts int64, area): the reference, computed once"""
    out = {}
    for h, w in SHAPES:
        for name, m in _masks(h, w).items():
            out[h, w, name] = (m, rle_ref.encode(m), rle_ref.area(m))
    return out


def _check(counts, meta, cap, expect, H, W):
    """counts int32 CUDA [B,cap] / meta [B,4] against [(mask, counts, area)] per stream"""
    c, mt = counts.cpu().numpy().view(np.uint32), meta.cpu().numpy()
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (len(expect), cap) and tuple(meta.shape) == (len(expect), 4)
    for b, (_, ref, ar) in enumerate(expect):
        assert mt[b].tolist() == [ref.size, ar, H, W], "meta of stream %d: %s, expected m %d area %d" % (b, mt[b].tolist(), ref.size, ar)
        k = min(ref.size, cap)
        assert np.array_equal(c[b, :k], ref[:k]), "counts of stream %d differ first at %s" % (b, np.flatnonzero(c[b, :k] != ref[:k])[:4])


@pytest.mark.parametrize("form", [None, 0, 1])       # the product entry (the LDS tiles), and the test entry with either byte source
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("H,W", SHAPES)
def test_encode_equals_the_reference(want, H, W, B, form):
    a = H * W
    names = list(_masks(1, 1))
    # the cases are what they are for
    assert want[H, W, "empty"][1].tolist() == [a] and want[H, W, "full"][1].tolist() == [0, a]
    assert want[H, W, "checker"][1].size == a + 1 or H % 2 == 0
    assert want[H, W, "last"][1].tolist() == ([0, 1] if a == 1 else [a - 1, 1])
    for i in range(0, len(names), B):
        pick = [names[(i + b) % len(names)] for b in range(B)]
        expect = [want[H, W, n] for n in pick]
        for scale in (1, 255):                                            # bytes 0 / 1 and bytes 0 / 255: the same counts
            m = torch.from_numpy(np.stack([e[0] for e in expect]) * np.uint8(scale)).cuda()
            counts, meta = preproc.rle_encode(m, cap=a + 1, _form=form)
            _check(counts, meta, a + 1, expect, H, W)
            if scale == 1:                                                # the host side reads them back into the same mask
                n = meta[:, 0].cpu().numpy()
                for b in range(B):
                    got = counts[b, :n[b]].cpu().numpy()
                    assert np.array_equal(rle.decode(got, H, W), expect[b][0]) and rle.area(got) == expect[b][2]


def test_cases_cover_both_tails_and_the_second_chunk(want):
    assert (4 * 256) % 64 == 0 and (64 * 1) % 64 == 0 and (37 * 300) % 64 != 0 and (63 * 65) % 64 != 0       # last pixel, both ways
    assert 257 * 300 > 65536 + 1 and want[257, 300, "at_words"][1].tolist() == [63, 1, 65535 - 64, 1, 257 * 300 - 65536]
    assert want[63, 65, "at_words"][1].tolist() == [63, 1, 63 * 65 - 64] and want[1, 64, "at_63"][1].tolist() == [63, 1]
    assert want[257, 300, "checker"][1].size == 257 * 300 + 1                 # every word of both chunks holds 64 transitions


@pytest.mark.parametrize("form", [None, 0])
def test_overflow_is_reported_and_nothing_beyond_cap_is_written(form):
    H, W, B, cap = 37, 300, 3, 5
    m = np.zeros((B, H, W), dtype=np.uint8)
    m[0, 5:20, 10] = m[0, 5:20, 40] = m[0, 3:9, 200] = m[0, 30:36, 299] = 1             # four runs inside the mask: eight transitions, m = 9
    m[1, 2:4, 7] = 1                                                                    # m = 3 < cap: counts[3:5] stay
    m[2] = m[0]
    ref = [rle_ref.encode(x) for x in m]
    assert ref[0].size == 9 and ref[1].size == 3
    big = torch.full((B * cap + 64,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")     # the nominal buffer and 64 elements beyond it
    meta = torch.full((B, 4), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    preproc.rle_encode(torch.from_numpy(m).cuda(), cap=cap, counts=big[:B * cap].view(B, cap), meta=meta, _form=form)
    first = big.clone()
    preproc.rle_encode(torch.from_numpy(m).cuda(), cap=cap, counts=big[:B * cap].view(B, cap), meta=meta, _form=form)
    assert torch.equal(first, big)                                      # a second call on the written output: the same bytes
    got, mt = big.cpu().numpy(), meta.cpu().numpy()
    assert mt[:, 0].tolist() == [9, 3, 9] and mt[:, 1].tolist() == [int(x.sum()) for x in m]
    rows = got[:B * cap].reshape(B, cap)
    assert rows[0].tolist() == ref[0][:5].tolist() and rows[2].tolist() == ref[2][:5].tolist()
    assert rows[1, :3].tolist() == ref[1].tolist() and (rows[1, 3:] == 0x7F7F7F7F).all()              # beyond m: untouched
    assert (got[B * cap:] == 0x7F7F7F7F).all()                                                         # beyond the buffer's end
    per = rle.to_host({"counts": big[:B * cap].view(1, B, cap), "n": mt[None, :, 0], "cap": cap})
    assert per[0][0] is None and per[0][2] is None and per[0][1].tolist() == ref[1].tolist()


def test_python_entries_reject_bad_arguments():
    m = torch.zeros((2, 30, 40), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        preproc.rle_encode(m.cpu())
    for bad in (dict(mask=m.float()), dict(mask=m[None]), dict(cap=0), dict(cap=30 * 40 + 2),
                dict(counts=torch.zeros((2, 9), dtype=torch.int32, device="cuda")),
                dict(meta=torch.zeros((2, 4), dtype=torch.int64, device="cuda")),
                dict(mask=torch.zeros((1, 4097, 2), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            preproc.rle_encode(**dict(dict(mask=m, cap=8), **bad))
    c, mt = preproc.rle_encode(m[0])                                    # [H,W]: one mask, the default cap
    assert tuple(c.shape) == (1, rle.default_cap(30, 40)) and mt.cpu().numpy().tolist() == [[1, 0, 30, 40]]
    for w in range(1, preproc._RLE_WS_MAX + 4):                         # the workspace cache is bounded: sizes that come and go
        preproc.rle_encode(m[:, :, :w])
    assert len(preproc._rle_ws) == preproc._RLE_WS_MAX and list(preproc._rle_ws)[-1][2:] == (2, w, 30)


# ---- the fused entry: the counts of the bytes smk_paste_mask_dev writes for the same arguments ----------------------------------
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("W,H", [(300, 37), (1, 1), (256, 4)])
def test_paste_rle_equals_the_encoding_of_the_pasted_mask(W, H, B):
    rng = np.random.default_rng(W * 1000 + H * 10 + B)
    logits, bbs = _streams(rng, B, W, H)                                # with B > 1 the last stream's patch lies wholly outside
    inv = np.stack([preproc.invert_affine(preproc.crop_back_map(bb, (W, H))) for bb in bbs])
    head = torch.from_numpy(rng.normal(0, 3, (B, 63 * 63, 25, 25)).astype(np.float32)).cuda()
    dyx = np.stack([rng.integers(0, 25, B), rng.integers(0, 25, B)], axis=1)
    a = W * H
    varied = False
    for slot in (0, 1):
        state = _state(inv, dyx, slot, B)
        for kw in (dict(logits=logits), dict(logits=None, head=head)):
            mask = preproc.paste_masks_dev(kw["logits"], state, slot, (W, H), seg_thr=0.35, head=kw.get("head")).cpu().numpy()
            expect = [(x, rle_ref.encode(x), rle_ref.area(x)) for x in mask]
            counts, meta = preproc.paste_rle(kw["logits"], state, slot, (W, H), seg_thr=0.35, head=kw.get("head"), cap=a + 1)
            _check(counts, meta, a + 1, expect, H, W)
            varied = varied or any(1 < e[1].size for e in expect)
            if "head" not in kw and B > 1 and a > 1:
                assert expect[B - 1][1].tolist() == [a]                 # wholly outside the frame: the empty mask
            # the byte entry on those very bytes gives the same rows, element for element up to m
            c2, m2 = preproc.rle_encode(torch.from_numpy(mask).cuda(), cap=a + 1)
            assert torch.equal(m2, meta)
    assert varied or a == 1
    if (W, H) == (300, 37):
        lg_mask = preproc.paste_masks_dev(logits, _state(inv, dyx, 0, B), 0, (W, H), seg_thr=0.35).cpu().numpy()
        assert 2 < rle_ref.encode(lg_mask[0]).size and 0 < lg_mask[0].sum() < a
