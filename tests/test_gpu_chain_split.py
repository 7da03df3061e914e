"""Refine chain on S workgroups per stream (row bands of post1, h0.0, h0.2, post2: csrc/chain_rows.h, refine_chain_body.inc) against
the unsplit chain, smk_tune chain_split = 1.  A pixel's arithmetic does not depend on the band it is computed in, so every logit
has to be the unsplit chain's BITS:
  * stand-alone launch (track_refine) at B = 1 and B = 3, S = 2 and 4, at refine positions that include both corners of the 25x25
    position range (the feature windows are clipped at the borders there);
  * B = 17 stand-alone under the rule (chain_split = 0);
  * fused step at B = 2, serial and pipelined (depth 1), S = 4 against S = 1, two frames with a result ring: refine, mask, box and
    the ring's rows and frame counter (the completion counter counts B * S arrivals and is reset by the last one)."""
import numpy as np
import pytest
import torch

from siammask_amd import _lib, synth

pytestmark = pytest.mark.gpu

CORNERS = [(0, 0), (24, 24), (0, 24), (12, 5)]
_MODELS = {}


def _tracked_model(B):
    """an eager fp16 model with track_mask done, shared by the stand-alone cases of one batch size"""
    if B not in _MODELS:
        from siammask_amd.custom import build
        m = build("sharp", dtype="f16", graph=False, max_batch=B)
        m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
        m = m.eval().cuda()
        m.template(torch.from_numpy(synth.smooth_image_batch(B, 127, stream0=410)).cuda())
        m.track_mask(torch.from_numpy(synth.smooth_image_batch(B, 255, stream0=417)).cuda())
        _MODELS[B] = m
    return _MODELS[B]


def _positions(B):
    """per-stream (y, x): B = 1 takes the corners one after the other, larger batches hold them side by side"""
    if B == 1:
        return [np.array([c], np.int32) for c in CORNERS[:2]]
    return [np.array([CORNERS[i % len(CORNERS)] for i in range(B)], np.int32)]


def _refine(m, pos, split):
    _lib.tune(chain_split=split)
    out = m.track_refine(pos).clone()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B", [1, 3])
def test_standalone_bands_are_the_unsplit_bits(B):
    m = _tracked_model(B)
    old = _lib.tune_get("chain_split")
    try:
        for pos in _positions(B):
            want = _refine(m, pos, 1)
            assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0.0
            for S in (2, 4):
                got = _refine(m, pos, S)
                diff = got != want
                assert torch.equal(got, want), "S = %d, pos %s: %d of %d logits differ, first at %s" % (
                    S, pos.tolist(), int(diff.sum()), got.numel(), tuple(int(v) for v in diff.nonzero()[0]))
    finally:
        _lib.tune(chain_split=old)


def test_standalone_rule_at_17_streams():
    m = _tracked_model(17)
    old = _lib.tune_get("chain_split")
    try:
        pos = _positions(17)[0]
        want = _refine(m, pos, 1)
        got = _refine(m, pos, 0)
        assert float(want.abs().max()) > 0.0 and torch.equal(got, want)
    finally:
        _lib.tune(chain_split=old)


def _step_outputs(B, frames, depth, split, rows=2):
    from siammask_amd.custom import build
    _lib.tune(chain_split=split)
    m = build("sharp", dtype="f16", graph=True, max_batch=B)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    m = m.eval().cuda()
    z = torch.from_numpy(synth.smooth_image_batch(B, 127, stream0=421)).cuda()
    xs = [torch.from_numpy(synth.smooth_image_batch(B, 255, stream0=421 + 7 * i)).cuda() for i in range(frames)]
    twh = torch.from_numpy(np.random.Generator(np.random.PCG64(421)).uniform(40.0, 110.0, size=(B, 2))).cuda()
    m.template(z)
    m.set_pipeline(depth)
    box, ref = m.set_result_ring(rows, batch=B)
    outs = []
    for i, x in enumerate(xs):
        o = m.track_step(x, twh, refine=True, stage=False)
        if depth:
            m.pipeline_join()
        torch.cuda.synchronize()
        d = {k: o[k].clone() for k in ("box", "refine", "mask")}
        d["ring_box"], d["ring_refine"], d["frames"] = box.clone(), ref.clone(), m.result_ring_frames()
        assert d["frames"] == i + 1
        outs.append(d)
    assert m.seq_status()[1] == 0
    return outs


@pytest.mark.parametrize("depth", [0, 1])
def test_fused_step_equals_the_unsplit_step(depth):
    old = _lib.tune_get("chain_split")
    try:
        want = _step_outputs(2, 2, depth, 1)
        got = _step_outputs(2, 2, depth, 4)
    finally:
        _lib.tune(chain_split=old)
    for f, (g, w) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(g["refine"]).all()) and float(g["refine"].abs().max()) > 0.0
        assert torch.equal(g["ring_refine"][f % 2], g["refine"].half()), f
        for k in ("refine", "mask", "box", "ring_box", "ring_refine"):
            assert torch.equal(g[k], w[k]), (f, k)
        assert g["frames"] == w["frames"] == f + 1
