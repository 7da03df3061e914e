"""The 63x63 mask head on stationary pixels (csrc/mask_head_tile.inc: C^T = W x A^T, NCHW logits stored straight from the MFMA
accumulators) against the generic implicit-GEMM tiles it replaces (conv_igemm_body<f16, 128x128x128, s2, nchw>).

The routine multiplies the same fp16 products in the same k order and adds the bias behind the K loop as the generic epilogue
does, so the logits have to be the generic path's BITS; the oracle gate is the fp16 one of tests/test_gpu_ops.py.
  * stand-alone launch (smk_op_conv2d_ex algo 7) at B = 1 (625 pixels: four full 128-pixel tiles and a 113-row remainder) and
    B = 3 (image boundaries inside the 32-lane store segments, 15 pixel tiles): bit-equal to algo 2 on 128x128 tiles, and within
    the fp16 tolerance of oracle/np_oracle.py;
  * channel tail: Cout = 3969 = 124 x 32 + 1 and a synthetic Cout = 33 -- the lone channel of the last block is right, and
    nothing is written in front of or behind the tensor (guard rows on both sides, NaN-filled output);
  * fused form: the B = 2 frame step, serial and pipelined (depth 1), with the mask half of chain_mask_kernel on the new tile
    against the same step with smk_tune chain_mask = 2 (the generic tiles): every output bit-equal."""
import numpy as np
import pytest
import torch

from helpers import rel_err
from oracle import np_oracle as O
from siammask_amd import _lib, synth

pytestmark = pytest.mark.gpu

TOL_F16 = 2e-3                         # tests/test_gpu_ops.py TOL["f16"]
HW = 25
_CACHE = {}


def _q(a):
    return a.astype(np.float16).astype(np.float64)


def _case(B, cout):
    """inputs, the generic path's logits and the oracle's, computed once per shape and left read-only"""
    if (B, cout) not in _CACHE:
        from siammask_amd import ops
        g = np.random.Generator(np.random.PCG64(1000 * B + cout))
        x = g.standard_normal((B, 256, HW, HW)).astype(np.float32)
        w = (g.standard_normal((cout, 256, 1, 1)) / 16.0).astype(np.float32)
        b = g.standard_normal(cout).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        generic = ops.conv2d(xd, w, b, dtype="f16", algo="mfma_nchw", tile=(128, 128))
        oracle = O.conv2d(_q(x), _q(w), b.astype(np.float64), 1, 0, 1)
        for a in (x, w, b, oracle):
            a.setflags(write=False)
        _CACHE[B, cout] = (xd, w, b, generic, oracle)
    return _CACHE[B, cout]


@pytest.mark.parametrize("B", [1, 3])
def test_logits_are_the_generic_tiles_bits(B):
    from siammask_amd import ops
    xd, w, b, generic, oracle = _case(B, 3969)
    y = ops.conv2d(xd, w, b, dtype="f16", algo="mask_head")
    torch.cuda.synchronize()
    assert rel_err(generic.cpu().numpy(), oracle) <= TOL_F16           # the reference arm itself
    diff = (y != generic)
    assert not bool(diff.any()), "%d of %d logits differ from the generic tiles, first at %s" % (
        int(diff.sum()), y.numel(), tuple(int(v) for v in diff.nonzero()[0]))
    assert rel_err(y.cpu().numpy(), oracle) <= TOL_F16


@pytest.mark.parametrize("B,cout", [(2, 3969), (2, 33)])
def test_channel_tail_and_guard_rows(B, cout):
    from siammask_amd import ops
    xd, w, b, generic, oracle = _case(B, cout)
    guard, n = 4 * HW * HW, B * cout * HW * HW                       # four channel planes of guard on either side
    buf = torch.full((n + 2 * guard,), 12345.0, dtype=torch.float32, device="cuda")
    out = buf[guard:guard + n].view(B, cout, HW, HW)
    out.fill_(float("nan"))                                            # a logit the routine does not write stays NaN
    y = ops.conv2d(xd, w, b, dtype="f16", algo="mask_head", out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    assert bool((buf[:guard] == 12345.0).all()), "wrote in front of the tensor"
    assert bool((buf[guard + n:] == 12345.0).all()), "wrote behind the tensor"
    assert torch.equal(y[:, cout - 1], generic[:, cout - 1]), "the lone channel of the last block"
    assert torch.equal(y, generic)
    assert rel_err(y.cpu().numpy(), oracle) <= TOL_F16


def test_ineligible_geometry_is_an_error():
    """no quiet change of kernel: a shape the routine does not cover is refused by the entry point"""
    from siammask_amd import ops
    x = torch.zeros((1, 128, 5, 5), device="cuda")
    with pytest.raises(RuntimeError):
        ops.conv2d(x, np.zeros((40, 128, 1, 1), np.float32), dtype="f16", algo="mask_head")


def _step_outputs(B, frames, depth, chain_mask):
    from siammask_amd.custom import build
    _lib.tune(chain_mask=chain_mask)
    m = build("sharp", dtype="f16", graph=True, max_batch=B)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    m = m.eval().cuda()
    z = torch.from_numpy(synth.smooth_image_batch(B, 127, stream0=321)).cuda()
    xs = [torch.from_numpy(synth.smooth_image_batch(B, 255, stream0=321 + 7 * i)).cuda() for i in range(frames)]
    twh = torch.from_numpy(np.random.Generator(np.random.PCG64(321)).uniform(40.0, 110.0, size=(B, 2))).cuda()
    m.template(z)
    m.set_pipeline(depth)
    outs = []
    for x in xs:
        o = m.track_step(x, twh, refine=True, stage=False)
        if depth:
            m.pipeline_join()
        torch.cuda.synchronize()
        outs.append({k: o[k].clone() for k in ("box", "cls", "loc", "refine", "mask")})
    assert m.seq_status()[1] == 0
    return outs


@pytest.mark.parametrize("depth", [0, 1])
def test_fused_step_equals_the_step_on_generic_tiles(depth):
    old = _lib.tune_get("chain_mask")
    try:
        want = _step_outputs(2, 3, depth, 2)
        got = _step_outputs(2, 3, depth, 1)
    finally:
        _lib.tune(chain_mask=old)
    for f, (g, w) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(g["mask"]).all())
        for k in ("mask", "refine", "box", "cls", "loc"):
            assert torch.equal(g[k], w[k]), (f, k)
