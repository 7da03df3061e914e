"""GPU parity of conv_seq_kernel -- the persistent per-XCD convolution sequence that runs ResNet layer2 / layer3 /
adjust at B = 8 (experiments/siammask_sharp/resnet.py:64-103,159-165) -- through its own C-ABI entry smk_op_conv_seq.

Every layer of every sequence is held to the per-op gate of tests/test_gpu_ops.py (fp16: 2e-3 of max|ref|, exact sums in
the oracle) ONE LAYER DEEP: the reference of layer i is the oracle convolution of the tensors the device itself handed to
layer i (its fp16 outputs are exactly representable), so an error cannot hide behind the error of an earlier layer.
Covered: the five workgroup-tile configurations (+ the deep-ring measurement variant), residual before the ReLU,
independent members without a barrier between them, several images per team, several tiles per workgroup, the K-loop
stagger, and the failure path (a sequence that cannot complete raises instead of returning garbage)."""
import numpy as np
import pytest
import torch

from oracle import np_oracle as O
from helpers import rel_err, seq_bottleneck as _bottleneck, seq_chain as _chain, seq_weight as _w

pytestmark = pytest.mark.gpu
TOL = 2e-3
TILES = [(64, 256), (64, 128), (64, 64), (128, 256), (128, 128), (128, 64), "deep"]


def _ops():
    from siammask_amd import ops
    return ops


def _q(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float64)


def _check(x, layers, outs, what):
    """layer-by-layer: oracle conv of the DEVICE's own inputs of that layer"""
    got = [o.cpu().numpy().astype(np.float64) for o in outs]
    srcs = [_q(x)] + got
    errs = {}
    for i, l in enumerate(layers):
        a = srcs[l.get("src", i - 1) + 1]
        ref = O.conv2d(a, _q(l["w"]), None if l.get("b") is None else l["b"].astype(np.float64),
                       l.get("stride", 1), l.get("pad", 0), l.get("dil", 1))
        if "res" in l and l.get("res_mode", 1) == 1:
            ref = ref + srcs[l["res"] + 1]
        if l.get("relu"):
            ref = np.maximum(ref, 0)
        if "res" in l and l.get("res_mode", 1) == 2:
            ref = ref + srcs[l["res"] + 1]
        errs[i] = rel_err(got[i], ref)
    bad = {i: e for i, e in errs.items() if not e <= TOL}
    assert not bad, "%s: layers %s over %.0e (all %s)" % (what, bad, TOL, errs)
    return errs


@pytest.mark.parametrize("kstag", [0, 1])
@pytest.mark.parametrize("tile", TILES)
def test_conv_seq_every_tile_configuration(tile, kstag):
    """a Bottleneck (1x1 -> dilated 3x3 -> 1x1 + residual) forced onto each workgroup tile; B = 3 (three teams work, five
    idle through every barrier), 23x23 = 529 rows per image: ragged last tile for 64- and 128-row tiles"""
    if tile == (128, 64) or tile == "deep":
        _needs_measure_build("the %s sequence tile (layer1 inside a sequence / the deep-ring measurement variant)" % (tile,))
    ops = _ops()
    rng = np.random.default_rng(11 + TILES.index(tile) + 100 * kstag)
    x = rng.uniform(-1, 1, size=(3, 256, 23, 23)).astype(np.float32)
    layers = _bottleneck(rng, 256, 128, tile=tile, kstag=kstag)
    outs, _, _ = ops.conv_seq(torch.from_numpy(x).cuda(), layers)
    _check(x, layers, outs, "tile %s kstag %d" % (tile, kstag))


def test_conv_seq_independent_members_and_strided_shortcut():
    """layer2.0 / layer3.0 shape of the engine's list: the shortcut convolution (3x3 stride 2 pad 0) and conv1 both read the
    block input and carry NO barrier between them; conv3 adds the shortcut's output; a second block follows"""
    ops = _ops()
    rng = np.random.default_rng(21)
    cin, planes = 128, 64
    x = rng.uniform(-1, 1, size=(2, cin, 31, 31)).astype(np.float32)
    layers = [
        dict(w=_w(rng, planes * 4, cin, 3), b=rng.uniform(-1, 1, planes * 4).astype(np.float32), stride=2, src=-1, sync=False),
        dict(w=_w(rng, planes, cin, 1), relu=True, src=-1),
        dict(w=_w(rng, planes, planes, 3), relu=True, stride=2, src=1),
        dict(w=_w(rng, planes * 4, planes, 1), relu=True, src=2, res=0, res_mode=1),
    ]
    blk = _bottleneck(rng, planes * 4, planes, dil=1)      # a second block on the first one's output
    blk[2]["res"] = 3
    layers += blk
    outs, _, _ = ops.conv_seq(torch.from_numpy(x).cuda(), layers)
    _check(x, layers, outs, "independent members")


def test_conv_seq_two_images_per_team_and_two_rounds_of_tiles():
    """B = 10: teams 0 and 1 own two images each (b, b + 8); 47x47 = 2209 rows per image = 35 tiles of 64 rows x 2 column
    tiles = 70 tiles for the 32 workgroups of a team (three rounds, the last one partial)"""
    ops = _ops()
    rng = np.random.default_rng(31)
    x = rng.uniform(-1, 1, size=(10, 64, 47, 47)).astype(np.float32)
    layers = [
        dict(w=_w(rng, 128, 64, 1), b=rng.uniform(-1, 1, 128).astype(np.float32), relu=True, tile=(64, 64)),
        dict(w=_w(rng, 64, 128, 3), pad=1, relu=True, tile=(64, 64)),
        dict(w=_w(rng, 64, 64, 1), relu=True, res=-1, res_mode=2, tile=(128, 128)),
    ]
    outs, _, _ = ops.conv_seq(torch.from_numpy(x).cuda(), layers)
    _check(x, layers, outs, "B=10")


def test_conv_seq_real_layer3_block_engine_choice():
    """the real shapes of a layer3 identity Bottleneck at the bench's batch (B = 8, 31x31, 1024 -> 256 -> 256 d2 -> 1024 +
    residual) and of layer3.0's long-K shortcut (3x3 512 -> 1024), with the tile and stagger rule the engine uses"""
    ops = _ops()
    rng = np.random.default_rng(41)
    x = rng.uniform(-1, 1, size=(8, 1024, 31, 31)).astype(np.float32)
    layers = _bottleneck(rng, 1024, 256)
    outs, us, clk = ops.conv_seq(torch.from_numpy(x).cuda(), layers, iters=3)
    _check(x, layers, outs, "layer3 block")
    assert us > 0 and clk.shape == (3, 2)
    x2 = rng.uniform(-1, 1, size=(8, 512, 31, 31)).astype(np.float32)
    l2 = [dict(w=_w(rng, 1024, 512, 3), b=rng.uniform(-1, 1, 1024).astype(np.float32), pad=1)]
    outs, _, _ = ops.conv_seq(torch.from_numpy(x2).cuda(), l2)
    _check(x2, l2, outs, "layer3.0 shortcut")


# ---- 3x3 layers on whole-row tiles with the activation patch shared by the nine taps: wreg_halo_tile.inc ------------------------
@pytest.mark.parametrize("kstag", [0, 1])
@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("tile,planes", [("halo128", 256), ("halo128", 128), ("halo64", 128)])
def test_conv_seq_patch_sharing_tiles(tile, planes, dil, kstag):
    """a Bottleneck whose conv2 (3x3, dilation 1 / 2, `planes` channels = two or four 64-channel chunks) is forced onto the
    patch-sharing tile: 23 x 23 images (five whole rows = 115 pixels per 128-pixel tile, the last tile has three; two rows = 46
    pixels per 64-pixel tile, the last tile has one), B = 3 (idle teams pass every barrier), chunk stagger off / on"""
    ops = _ops()
    rng = np.random.default_rng(91 + planes + dil + 10 * kstag + (tile == "halo64"))
    x = rng.uniform(-1, 1, size=(3, 256, 23, 23)).astype(np.float32)
    layers = _bottleneck(rng, 256, planes, dil=dil, kstag=kstag)
    layers[1]["tile"] = tile
    outs, _, _ = ops.conv_seq(torch.from_numpy(x).cuda(), layers)
    _check(x, layers, outs, "%s planes %d dil %d kstag %d" % (tile, planes, dil, kstag))


def test_conv_seq_patch_sharing_engine_choice_and_several_images_per_team():
    """the engine's own rule (smk_tune "seq_halo", default on) on the bench's shapes: layer3's conv2 (256 channels, dilation 2,
    31 x 31: 8 x 4 tiles of 128 pixels) and layer2's (128 channels, dilation 1: 16 x 2 tiles of 64 pixels) at B = 10 (two
    images on two of the teams), the 15 x 15 template shape, against the im2col tiles (seq_halo 0): fp16 summation order only"""
    from siammask_amd import _lib
    ops = _ops()
    rng = np.random.default_rng(95)
    for (B, S, cin, planes, dil) in ((10, 31, 1024, 256, 2), (8, 31, 512, 128, 1), (8, 15, 1024, 256, 2)):
        x = rng.uniform(-1, 1, size=(B, cin, S, S)).astype(np.float32)
        layers = _bottleneck(rng, cin, planes, dil=dil)
        xd = torch.from_numpy(x).cuda()
        assert _lib.tune_get("seq_halo") == 1
        outs, us, clk = ops.conv_seq(xd, layers, iters=3)
        _check(x, layers, outs, "engine choice B %d S %d planes %d" % (B, S, planes))
        try:
            _lib.tune(seq_halo=0)
            plain, us0, clk0 = ops.conv_seq(xd, layers, iters=3)
        finally:
            _lib.tune(seq_halo=1)
        assert torch.equal(outs[0], plain[0])
        assert not torch.equal(outs[1], plain[1]) or planes == 0      # another kernel, another summation order
        for i in (1, 2):
            assert rel_err(outs[i].cpu().numpy(), plain[i].cpu().numpy().astype(np.float64)) <= 1.5e-3, i
        print("B %d S %d planes %d: conv2 tiles %.2f us (im2col tiles %.2f us)" % (B, S, planes, clk[1, 0], clk0[1, 0]))


# ---- the fused (conv3, next 1x1) pairs: c3c1_tile.inc ------------------------------------------------------------------------
def _two_blocks(rng, cin, planes, tail_relu=True):
    """Bottleneck -> Bottleneck's conv1 (or, with tail_relu False, `adjust`: 1x1 + BN without ReLU, custom.py:19-25): the pair
    (layer 2, layer 3) is what the engine's lists hold between two identity blocks"""
    blk = _bottleneck(rng, cin, planes)
    blk.append(dict(w=_w(rng, planes, cin, 1), b=rng.uniform(-1, 1, planes).astype(np.float32), relu=tail_relu))
    return blk


@pytest.mark.parametrize("shape", [(1024, 256), (512, 128)])
@pytest.mark.parametrize("B,S", [(3, 23), (8, 31), (10, 15)])
def test_conv_seq_fused_conv3_conv1_pairs(shape, B, S):
    """layer3's (256 -> 1024 + residual, ReLU -> 256) and layer2's (128 -> 512 -> 128) pairs as ONE tile routine on 32-row
    tiles: ragged last tile (23 x 23 = 529 = 16.5 tiles), idle teams (B = 3), the bench's shape (B = 8, 31 x 31: 31 tiles for
    32 workgroups), two images on two of the teams (B = 10); both outputs of the pair -- conv3's (the next residual) and
    the 1x1's -- are held to the per-op gate one layer deep, and the unfused list computes the same tensors"""
    from siammask_amd import _lib
    ops = _ops()
    cin, planes = shape
    rng = np.random.default_rng(71 + cin + B)
    x = rng.uniform(-1, 1, size=(B, cin, S, S)).astype(np.float32)
    tail = _bottleneck(rng, planes, planes // 2, dil=1)      # a block behind the pair: its 3x3 reads the 1x1's output across the team barrier
    tail[2]["res"] = 3
    layers = _two_blocks(rng, cin, planes) + tail
    xd = torch.from_numpy(x).cuda()
    info = {}
    old = _lib.tune_get("seq_fuse")
    assert old == 1
    try:
        outs, _, _ = ops.conv_seq(xd, layers, info=info)
        assert info["fused_pairs"] == 1, info
        _lib.tune(seq_fuse=0)
        plain, _, _ = ops.conv_seq(xd, layers, info=info)
    finally:
        _lib.tune(seq_fuse=old)
    assert info["fused_pairs"] == 0
    _check(x, layers, outs, "fused pair %s B=%d S=%d" % (shape, B, S))
    # conv1 / conv2 / conv3 see the same inputs either way; conv3 differs by summation order only (then fp16 rounding)
    for i in (0, 1):
        assert torch.equal(outs[i], plain[i]), i
    for i in (2, 3):
        assert rel_err(outs[i].cpu().numpy(), plain[i].cpu().numpy().astype(np.float64)) <= 1e-3, i


def _needs_measure_build(what):
    """round 5: the arms that measured a wash (pair split over two CUs, triples) left the product library; they are compiled by
    `make MEASURE=1` only (HISTORY.md 3.1l, 3.1o) -- their parity tests run against such a build and are skipped otherwise"""
    from siammask_amd import _lib
    if not _lib.tune_get("measure_build"):
        pytest.skip("%s is only in a library built with `make MEASURE=1`" % what)



@pytest.mark.parametrize("shape", [(1024, 256), (512, 128)])
@pytest.mark.parametrize("B,S", [(3, 23), (8, 31), (10, 15), (8, 47)])
def test_conv_seq_pair_split_over_two_cus(shape, B, S):
    """the same pairs as a 2-D split over a PAIR of CUs (c3c1p_tile.inc, smk_tune seq_pair2d): 64-row tiles, each CU half of conv3's
    channels and the matching K half of the second convolution, fp32 partial sums exchanged through the pair's slabs.  Ragged
    tiles and idle pairs (23 x 23 = 529 rows -> 16 tiles of 34; B = 3: idle teams), the bench's shape (961 rows -> 16 tiles of 61),
    two images on two of the teams (B = 10: consecutive exchanges of a pair, both slab sets), several rounds of tiles per pair
    (47 x 47 = 2209 rows -> 35 tiles of 64 on 16 pairs: the last round has idle pairs).  Both outputs of the pair one layer deep;
    against the one-CU routine: conv1 / conv2 bit-equal, the pair within summation-order noise; 5 launches bit-identical."""
    _needs_measure_build("the pair split over two CUs (seq_pair2d)")
    from siammask_amd import _lib
    ops = _ops()
    cin, planes = shape
    rng = np.random.default_rng(171 + cin + B + S)
    x = rng.uniform(-1, 1, size=(B, cin, S, S)).astype(np.float32)
    tail = _bottleneck(rng, planes, planes // 2, dil=1)
    tail[2]["res"] = 3
    layers = _two_blocks(rng, cin, planes) + tail
    xd = torch.from_numpy(x).cuda()
    info = {}
    assert _lib.tune_get("seq_fuse") == 1
    old = _lib.tune_get("seq_pair2d")
    try:
        _lib.tune(seq_pair2d=1)
        outs, _, _ = ops.conv_seq(xd, layers, info=info)
        assert info["fused_pairs"] == 1, info
        again, _, _ = ops.conv_seq(xd, layers, iters=5, info=info)
        _lib.tune(seq_pair2d=0)
        one_cu, _, _ = ops.conv_seq(xd, layers, info=info)
        assert info["fused_pairs"] == 1
    finally:
        _lib.tune(seq_pair2d=old)
    _check(x, layers, outs, "pair split %s B=%d S=%d" % (shape, B, S))
    for u, v in zip(outs, again):
        assert torch.equal(u, v), "repeated launches of the pair-split list differ"
    for i in (0, 1):
        assert torch.equal(outs[i], one_cu[i]), i
    for i in (2, 3):      # (the K-loop stagger starts a tile's k-steps elsewhere: another fp32 summation order, then fp16 rounding)
        assert rel_err(outs[i].cpu().numpy(), one_cu[i].cpu().numpy().astype(np.float64)) <= 1e-3, i


def test_conv_seq_pair_split_chain_of_layer3_blocks_and_adjust():
    """three identity Bottlenecks of layer3 + adjust at the bench's batch with every pair split over two CUs: three exchanges per
    pair and launch (slab sets 0, 1, 0), each pair's residual is the previous pair's conv3 output (written in two channel halves
    by two CUs)"""
    _needs_measure_build("the pair split over two CUs (seq_pair2d)")
    from siammask_amd import _lib
    ops = _ops()
    rng = np.random.default_rng(181)
    x = rng.uniform(-1, 1, size=(8, 1024, 31, 31)).astype(np.float32)
    layers = []
    for b in range(3):
        blk = _bottleneck(rng, 1024, 256)
        if b:
            blk[0]["src"] = len(layers) - 1
            blk[2]["res"] = len(layers) - 1
        layers += blk
    layers.append(dict(w=_w(rng, 256, 1024, 1), b=rng.uniform(-1, 1, 256).astype(np.float32), relu=False))
    info = {}
    xd = torch.from_numpy(x).cuda()
    old = _lib.tune_get("seq_pair2d")
    try:
        _lib.tune(seq_pair2d=1)
        outs, us, clk = ops.conv_seq(xd, layers, iters=5, info=info)
        assert info["fused_pairs"] == 3, info
        again, _, _ = ops.conv_seq(xd, layers, info=info)
        _lib.tune(seq_pair2d=0)
        _, us1, clk1 = ops.conv_seq(xd, layers, iters=5, info=info)
    finally:
        _lib.tune(seq_pair2d=old)
    _check(x, layers, outs, "layer3 chain, pair split")
    for u, v in zip(outs, again):
        assert torch.equal(u, v)
    print("layer3 chain: pair split %.1f us per launch (per layer %s) vs one CU per 32 rows %.1f us (%s)" % (
        us, np.round(clk[:, 0], 1).tolist(), us1, np.round(clk1[:, 0], 1).tolist()))


def test_conv_seq_fused_chain_of_layer3_blocks_and_adjust():
    """three identity Bottlenecks of layer3 + adjust at the bench's batch: conv1, conv2, [conv3 + conv1], conv2, [conv3 + conv1],
    conv2, [conv3 + adjust (no ReLU)] -- every fused pair's residual is the previous pair's conv3 output, written from LDS"""
    ops = _ops()
    rng = np.random.default_rng(81)
    x = rng.uniform(-1, 1, size=(8, 1024, 31, 31)).astype(np.float32)
    layers = []
    for b in range(3):
        blk = _bottleneck(rng, 1024, 256)
        if b:
            blk[0]["src"] = len(layers) - 1
            blk[2]["res"] = len(layers) - 1
        layers += blk
    layers.append(dict(w=_w(rng, 256, 1024, 1), b=rng.uniform(-1, 1, 256).astype(np.float32), relu=False))
    for i, l in enumerate(layers):               # absolute residual sources (the helper's default is relative to the block)
        if "res" in l and l["res"] == -1 and i > 2:
            raise AssertionError("residual source not set")
    info = {}
    xd = torch.from_numpy(x).cuda()
    outs, us, clk = ops.conv_seq(xd, layers, iters=5, info=info)
    assert info["fused_pairs"] == 3, info
    _check(x, layers, outs, "layer3 chain")
    again, _, _ = ops.conv_seq(xd, layers, info=info)
    for u, v in zip(outs, again):
        assert torch.equal(u, v)
    print("fused layer3 chain: %.1f us per launch; per layer (tiles us): %s" % (us, np.round(clk[:, 0], 1).tolist()))


def test_conv_seq_pair_is_not_fused_across_a_pending_barrier():
    """c3c1_tile prefetches the residual BEFORE its hoist-point wait.  The barrier pending there is the one behind
    the last sync layer in front of the pair -- with an independent sync = 0 member in between, that is the barrier behind the
    residual's own writer, and the pair must stay two layers.  (t: conv3's input; R: the residual, written one barrier later;
    u: an independent member without a barrier.)  Either way every layer is right one layer deep."""
    ops = _ops()
    rng = np.random.default_rng(97)
    B, S = 8, 31
    x = rng.uniform(-1, 1, size=(B, 256, S, S)).astype(np.float32)
    bias = lambda n: rng.uniform(-1, 1, n).astype(np.float32)
    t = dict(w=_w(rng, 256, 256, 1), b=bias(256), relu=True, src=-1)                       # 0: conv3's input, barrier behind it
    R = dict(w=_w(rng, 1024, 256, 1), b=bias(1024), relu=True, src=-1)                     # 1: the residual, barrier behind it
    u = dict(w=_w(rng, 256, 256, 1), b=bias(256), relu=True, src=-1, sync=False)           # 2: independent member, NO barrier
    c3 = dict(w=_w(rng, 1024, 256, 1), b=bias(1024), relu=True, src=0, res=1, res_mode=1)  # 3: conv3(t) + R
    c1 = dict(w=_w(rng, 256, 1024, 1), b=bias(256), relu=True)                             # 4: the next block's conv1
    xd = torch.from_numpy(x).cuda()
    info = {}
    outs, _, _ = ops.conv_seq(xd, [t, R, u, c3, c1], info=info)
    assert info["fused_pairs"] == 0, "the pair was fused although the barrier behind its residual's writer is still pending"
    _check(x, [t, R, u, c3, c1], outs, "pending barrier, unfused")
    # control: the residual written one barrier EARLIER than conv3's input is safe to prefetch -> fused
    outs, _, _ = ops.conv_seq(xd, [R, t, u, dict(c3, src=1, res=0), c1], info=info)
    assert info["fused_pairs"] == 1, info
    _check(x, [R, t, u, dict(c3, src=1, res=0), c1], outs, "passed barrier, fused")


def test_conv_seq_repeated_launches_leave_the_counters_clean():
    """the team counters reset themselves: 20 launches in a row (iters) and a second call give the same bits"""
    ops = _ops()
    rng = np.random.default_rng(51)
    x = rng.uniform(-1, 1, size=(8, 128, 15, 15)).astype(np.float32)
    layers = _bottleneck(rng, 128, 64, dil=1)
    xd = torch.from_numpy(x).cuda()
    a, _, _ = ops.conv_seq(xd, layers, iters=20)
    b, _, _ = ops.conv_seq(xd, layers, iters=1)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    _check(x, layers, a, "repeated")


def test_conv_seq_measurement_build_gives_the_same_bits(monkeypatch, capfd):
    """SMK_SEQ_CLK=2 selects conv_seq_kernel<4, 1> (phase stamps inside the first tile of every layer): a separate
    instantiation that ships in the library -- it must compute exactly what the default build computes"""
    ops = _ops()
    rng = np.random.default_rng(61)
    x = rng.uniform(-1, 1, size=(8, 128, 15, 15)).astype(np.float32)
    layers = _bottleneck(rng, 128, 64, dil=1)
    xd = torch.from_numpy(x).cuda()
    a, _, _ = ops.conv_seq(xd, layers)
    monkeypatch.setenv("SMK_SEQ_CLK", "2")
    b, _, _ = ops.conv_seq(xd, layers)
    monkeypatch.delenv("SMK_SEQ_CLK")
    err = capfd.readouterr().err
    assert "[seq clk2]" in err and "K loop" in err
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ---- failure must be loud and safe (the kernel needs all 256 workgroups resident at once) ---------------------------------
def _model(B):
    from siammask_amd import synth
    from siammask_amd.custom import build
    m = build("sharp", dtype="f16", graph=True, max_batch=B)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    return m.eval().cuda()


def _step_inputs(B, stream0):
    from siammask_amd import synth
    z = torch.from_numpy(synth.smooth_image_batch(B, 127, stream0=stream0)).cuda()
    x = torch.from_numpy(synth.smooth_image_batch(B, 255, stream0=stream0)).cuda()
    twh = torch.tensor([[60.0, 80.0]] * B, dtype=torch.float64).cuda()
    return z, x, twh


def _safe_step(m, z, x, twh, want, what):
    """one frame step that must be EITHER correct OR raise; after a raise the context has fallen back to the per-layer kernels
    and the re-submitted template + frame must be correct.  Returns True when the failure path was taken."""
    from siammask_amd import _lib
    raised = False
    try:
        out = {k: v.clone() for k, v in m.track_step(x, twh, refine=True).items() if v is not None}
        torch.cuda.synchronize()
        grid, err = m.seq_status()                    # raises when the work that has just drained reported a failure
    except _lib.SmkError as e:
        raised = True
        assert "conv_seq_kernel reported" in str(e), e
        m.template(z)                                 # the failure report invalidates the cached template as well
        out = {k: v.clone() for k, v in m.track_step(x, twh, refine=True).items() if v is not None}
        torch.cuda.synchronize()
        try:
            m.seq_status()
        except _lib.SmkError as e2:                   # sticky report of the earlier failure: sequences are off now
            assert "persistent sequences are off" in str(e2), e2
    for k in ("cls", "loc", "mask", "refine"):
        e = rel_err(out[k].cpu().numpy(), want[k])
        assert e <= 5e-3, "%s: %s differs from the solo run by %.2e (failure path taken: %s)" % (what, k, e, raised)
    return raised


def test_injected_sequence_failure_is_repaired_inside_the_same_call():
    """VERDICT r3 item 7 / ADVICE r3 (medium): a sequence failure used to surface at the NEXT entry point, after a drop-in caller
    (tools/test.py:205 `.cpu()`) had consumed the invalid frame.  Now template / track_mask / track_refine check the kernel's
    flag behind the call (smk_seq_sync_check) and re-run the frame on the per-layer kernels: with the flag raised by hand
    (smk_debug_seq_inject: the next sequence launch returns at once, leaving garbage) every call still returns correct
    tensors, never raises, and the context ends with sequences off."""
    from siammask_amd import _lib
    B = 8
    z, x, twh = _step_inputs(B, 540)
    pos = torch.tensor([[12, 11]] * B, dtype=torch.int32).cuda()
    ref = _model(B)
    ref.template(z)
    wc, wl, wm = [t.clone() for t in ref.track_mask(x)]
    wr = ref.track_refine(pos).clone()
    torch.cuda.synchronize()
    assert ref.seq_status()[0] > 0 and ref.seq_recovered == 0
    del ref
    for where in ("template", "track", "refine"):
        m = _model(B)
        if where == "template":
            m._ensure(z, B, grow=True)                # context + weights exist before the first template
            _lib.check(_lib.lib().smk_debug_seq_inject(m._ctx, 2))
        m.template(z)
        if where == "track":
            _lib.check(_lib.lib().smk_debug_seq_inject(m._ctx, 2))
        cls, loc, mask = m.track_mask(x)
        if where == "refine":
            # a failure that is only noticed at refine's entry (e.g. left behind by an unguarded asynchronous track_step)
            _lib.check(_lib.lib().smk_debug_seq_inject(m._ctx, 1))
        r = m.track_refine(pos)
        torch.cuda.synchronize()
        assert m.seq_recovered == 1, (where, m.seq_recovered)
        for name, got, want in (("cls", cls, wc), ("loc", loc, wl), ("mask", mask, wm), ("refine", r, wr)):
            e = rel_err(got.cpu().numpy(), want.cpu().numpy().astype(np.float64))
            assert e <= 5e-3, "failure injected before %s: %s differs by %.2e" % (where, name, e)
        g = ctypes_int_pair(m)
        assert g == 0, "sequences must be off after a reported failure (grid %d)" % g
        del m


def ctypes_int_pair(m):
    import ctypes
    from siammask_amd import _lib
    g, e = ctypes.c_int(0), ctypes.c_int(0)
    _lib.lib().smk_seq_status(m._ctx, ctypes.byref(g), ctypes.byref(e))      # (non-zero rc: the sticky report -- expected here)
    return g.value


def test_two_contexts_on_two_streams_stay_correct_or_raise():
    """two contexts stepping concurrently on two streams: each launch of conv_seq_kernel needs every CU, so the two can
    starve each other of co-residency.  Whatever the dispatcher does, every step is either correct or reported."""
    B = 8
    z, x, twh = _step_inputs(B, 500)
    ref = _model(B)
    ref.template(z)
    want = {k: v.cpu().numpy() for k, v in ref.track_step(x, twh, refine=True).items() if v is not None}
    torch.cuda.synchronize()
    del ref
    ms = [_model(B), _model(B)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for m, st in zip(ms, streams):
        with torch.cuda.stream(st):
            m.template(z)
    torch.cuda.synchronize()
    raised = 0
    for it in range(6):
        for m, st in zip(ms, streams):
            with torch.cuda.stream(st):
                raised += _safe_step(m, z, x, twh, want, "two contexts, round %d" % it)
    print("two contexts: failure path taken %d times of 12" % raised)


def test_side_stream_work_during_a_step_stays_correct_or_raises():
    """a side stream keeps the CUs busy with large GEMMs (what an RCCL gather or another model would do) while the fused
    B = 8 step with its persistent launch runs: correct, or reported and correct after the fall-back"""
    B = 8
    z, x, twh = _step_inputs(B, 520)
    m = _model(B)
    m.template(z)
    want = {k: v.cpu().numpy() for k, v in m.track_step(x, twh, refine=True).items() if v is not None}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a = torch.randn(8192, 8192, device="cuda", dtype=torch.float16)
    raised = 0
    for it in range(4):
        with torch.cuda.stream(side):
            for _ in range(6):
                a = (a @ a).clamp_(-1, 1)
        raised += _safe_step(m, z, x, twh, want, "side stream, round %d" % it)
    torch.cuda.synchronize()
    print("side stream: failure path taken %d times of 4" % raised)


@pytest.mark.parametrize("shape,dil", [((1024, 256), 2), ((1024, 256), 1), ((512, 128), 1)])
@pytest.mark.parametrize("B,S", [(8, 31), (3, 29), (10, 31)])
def test_conv_seq_fused_triples(shape, dil, B, S):
    """round 4: [conv2 3x3, conv3 + residual + ReLU, the next 1x1] of a Bottleneck as ONE tile routine on image-row tiles (c3c1_tile.inc,
    FRONT = 1; smk_tune seq_fuse3) -- conv2's output never reaches memory and the barrier between conv2 and conv3 is gone.  A chain of
    three identity blocks + adjust: the first triple's residual is the list input (requested in front of the wait), the later ones' is
    the previous triple's conv3 output written by the SAME workgroup; dilation 1 and 2 (33 / 35-pixel padded rows), both layers'
    shapes, idle teams (B = 3), two images on two of the teams (B = 10), 29-pixel rows.  Against the unfused list (itself held to the
    oracle one layer deep): conv3's and the 1x1's outputs within fp16 summation-order noise; run twice: bit-identical."""
    _needs_measure_build("the triple routine (seq_fuse3)")
    from siammask_amd import _lib
    ops = _ops()
    cin, planes = shape
    rng = np.random.default_rng(131 + cin + B + dil)
    x = rng.uniform(-1, 1, size=(B, cin, S, S)).astype(np.float32)
    layers = _chain(rng, cin, planes, 3, dil)
    xd = torch.from_numpy(x).cuda()
    info = {}
    keep = [i for i in range(len(layers)) if i % 3 != 1 or i == len(layers) - 1]       # every record but the conv2s (never stored:
    old = _lib.tune_get("seq_fuse3")                                                    # a conv2 output read back keeps its triple off)
    try:
        _lib.tune(seq_fuse3=1)
        outs, _, _ = ops.conv_seq(xd, layers, want_outputs=keep, info=info)
        assert info["fused_pairs"] == 3 and _lib.tune_get("seq_fused3_last") == 3, (info, _lib.tune_get("seq_fused3_last"))
        again, _, _ = ops.conv_seq(xd, layers, want_outputs=keep, info=info)
        _lib.tune(seq_fuse3=0)
        plain, _, _ = ops.conv_seq(xd, layers, info=info)
        assert _lib.tune_get("seq_fused3_last") == 0
    finally:
        _lib.tune(seq_fuse3=old)
    _check(x, layers, plain, "unfused chain %s" % (shape,))
    for i in keep:
        assert torch.equal(outs[i], again[i]), "layer %d differs between two launches" % i
        e = rel_err(outs[i].cpu().numpy(), plain[i].cpu().numpy().astype(np.float64))
        assert e <= 3e-3, "%s dil %d B=%d S=%d: layer %d differs from the unfused list by %.2e" % (shape, dil, B, S, i, e)


def test_conv_seq_triples_leave_short_rows_and_shared_conv2_outputs_alone():
    """the template's 15 x 15 images keep the pairs (one image row would fill half a tile), and a conv2 whose output somebody else
    reads as well must reach memory: no triple"""
    _needs_measure_build("the triple routine (seq_fuse3)")
    from siammask_amd import _lib
    ops = _ops()
    rng = np.random.default_rng(151)
    old = _lib.tune_get("seq_fuse3")
    try:
        _lib.tune(seq_fuse3=1)
        x = rng.uniform(-1, 1, size=(8, 1024, 15, 15)).astype(np.float32)
        layers = _chain(rng, 1024, 256, 2, 2)
        info = {}
        outs, _, _ = ops.conv_seq(torch.from_numpy(x).cuda(), layers, info=info)
        assert info["fused_pairs"] == 2 and _lib.tune_get("seq_fused3_last") == 0
        _check(x, layers, outs, "15 x 15: pairs")
        x = rng.uniform(-1, 1, size=(8, 1024, 31, 31)).astype(np.float32)
        layers = _chain(rng, 1024, 256, 1, 2)
        layers.append(dict(w=_w(rng, 256, 256, 1), b=rng.uniform(-1, 1, 256).astype(np.float32), relu=True, src=1))      # reads conv2's output too
        outs, _, _ = ops.conv_seq(torch.from_numpy(x).cuda(), layers, info=info)
        assert _lib.tune_get("seq_fused3_last") == 0
        _check(x, layers, outs, "conv2 read twice: no triple")
    finally:
        _lib.tune(seq_fuse3=old)


@pytest.mark.parametrize("B", [8, 12])
def test_scalar_path_poll_gives_the_same_bits_and_clean_counters(B):
    """round 4: the team barrier's poll through the scalar memory path (s_load_dword glc; smk_tune seq_spoll, default on) against the
    vector sc1 load: only HOW a workgroup learns that the barrier is complete changes -- every output of the fused step bit-identical,
    no failure reported, over several frames (the counters return to zero between launches either way)"""
    from siammask_amd import _lib
    old = _lib.tune_get("seq_spoll")
    assert old == 1
    outs = {}
    try:
        for v in (1, 0):
            _lib.tune(seq_spoll=v)
            m = _model(B)
            z, x, twh = _step_inputs(B, 520)
            m.template(z)
            for _ in range(3):
                o = m.track_step(x, twh, refine=True)
            torch.cuda.synchronize()
            grid, err = m.seq_status()
            assert grid == 256 and err == 0, (grid, err)
            outs[v] = {k: t.clone() for k, t in o.items() if t is not None}
            del m
    finally:
        _lib.tune(seq_spoll=old)
    for k in outs[1]:
        assert torch.equal(outs[1][k], outs[0][k]), k


@pytest.mark.parametrize("shape,B,S", [((1024, 256), 8, 31), ((1024, 256), 3, 15), ((512, 128), 8, 31), ((512, 128), 5, 15)])
def test_conv_seq_resident_trunk_gives_the_same_bits(shape, B, S):
    """Round 6 (smk_tune "seq_yres"): with one image per team the fused pairs of a ResNet layer run on the same 32 rows in the same
    workgroup, Bottleneck after Bottleneck (resnet.py:80-103), so the second pair finds its residual -- the Y image the first one
    built -- still in LDS: no re-fetch, no store of a tensor nobody else reads, the 3x3 convolution in between works in the LDS
    behind the image (its 128-row accumulator hand-over in two halves).  Nothing about the arithmetic changes: every output must be
    BIT-identical to the list without the marks, with every tensor read back (Y stored) and with only the last one (Y never
    leaves the CUs); at B = 10 (two images on some teams) nothing may be marked."""
    from siammask_amd import _lib
    ops = _ops()
    cin, planes = shape
    rng = np.random.default_rng(606 + S + cin)
    x = rng.uniform(-1, 1, size=(B, cin, S, S)).astype(np.float32)
    layers = _chain(rng, cin, planes, 3, 2 if cin == 1024 else 1)
    xd = torch.from_numpy(x).cuda()
    old = _lib.tune_get("seq_yres")
    try:
        _lib.tune(seq_yres=0)
        ref, _, _ = ops.conv_seq(xd, layers)
        assert _lib.tune_get("seq_yres_last") == 0
        _check(x, layers, ref, "chain without the marks")
        _lib.tune(seq_yres=1)
        info = {}
        got, us, clk = ops.conv_seq(xd, layers, iters=3, info=info)
        assert info["fused_pairs"] == 3 and _lib.tune_get("seq_yres_last") == 2, (info, _lib.tune_get("seq_yres_last"))
        for i, (u, v) in enumerate(zip(ref, got)):
            assert torch.equal(u, v), (i, float((u - v).abs().max()))
        last = len(layers) - 1
        only, _, _ = ops.conv_seq(xd, layers, iters=3, want_outputs=(last,))
        assert _lib.tune_get("seq_yres_last") == 2
        assert torch.equal(only[last], ref[last]), float((only[last] - ref[last]).abs().max())
        # two images on a team: a workgroup owns two tiles per pair, Y cannot stay
        x10 = rng.uniform(-1, 1, size=(10, cin, 15, 15)).astype(np.float32)
        a10, _, _ = ops.conv_seq(torch.from_numpy(x10).cuda(), layers, want_outputs=(last,))
        assert _lib.tune_get("seq_yres_last") == 0
        _lib.tune(seq_yres=0)
        b10, _, _ = ops.conv_seq(torch.from_numpy(x10).cuda(), layers, want_outputs=(last,))
        assert torch.equal(a10[last], b10[last])
    finally:
        _lib.tune(seq_yres=old)
    print("resident trunk %s B=%d S=%d: %.1f us per launch; per layer (tiles us): %s" % (shape, B, S, us, np.round(clk[:, 0], 1).tolist()))
