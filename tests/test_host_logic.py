"""CPU tests of the host logic of libsiammask_hip.so (no GPU needed):
the C-ABI library loads and exports every declared symbol, and the weight packing order +
the kernels' own row/tap decode + gather-offset functions (shared host/device code in
siammask_amd/csrc/smk_kernels.h), walked on the host by smk_host_conv2d_ex, reproduce the
oracle's conv2d for every geometry class on the path, including the Refine windows
(custom.py:133-135), the template centre crop (custom.py:21-24) and nearest upsampling
(custom.py:150-152)."""
import ctypes
import re
import os

import numpy as np
import pytest

from oracle import np_oracle as O
from siammask_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    declared = set()
    for h in ("siammask_hip.h", "siammask_hip_test.h"):         # product ABI + test / measurement entry points
        hdr = open(os.path.join(REPO, "include", h)).read()
        hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)        # (prose in comments mentions entry points of the other header)
        declared |= set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", hdr))
    declared.discard("smk_ctx")
    product = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "siammask_hip.h")).read(), flags=re.S)))
    assert not {"smk_tune", "smk_profile", "smk_bench_conv", "smk_op_conv2d_ex", "smk_debug_read"} & product    # the product header stays free of them
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    L = _lib.lib()
    for s in declared:
        assert hasattr(L, s), s
    assert L.smk_version() >> 16 == 1


def test_every_declared_function_resolves():
    """The entry points are defined in several translation units.  A definition that does not see its extern "C" declaration gets
    a mangled name, and ctypes would notice only when that one function is first called -- for most of them inside a GPU test.
    Here every function either header declares is looked up in the loaded library, whatever _lib.SYMBOLS lists."""
    L = _lib.lib()
    for header in ("siammask_hip.h", "siammask_hip_test.h"):
        hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
        names = sorted(set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", hdr)))
        assert names, header
        unresolved = []
        for name in names:
            try:
                getattr(L, name)
            except AttributeError:
                unresolved.append(name)
        assert not unresolved, "%s declares functions the library does not export: %s" % (header, unresolved)


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _lib.lib()
    ctx = ctypes.c_void_p()
    rc = L.smk_create(ctypes.byref(ctx), 0, 0, 2, 1)
    assert rc == -5 and b"no HIP device" in L.smk_last_error()
    with pytest.raises(_lib.SmkError):
        _lib.check(rc)


def _fp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def host_conv(x, w, b=None, res=None, pos=None, **kw):
    g = _lib.ConvGeom()
    B, Cin, H, W = x.shape
    g.B, g.Cin, g.H, g.W = B, Cin, H, W
    g.Cout, g.k = w.shape[0], w.shape[2]
    g.stride, g.pad, g.dil = kw.get("stride", 1), kw.get("pad", 0), kw.get("dil", 1)
    for f in ("relu", "res_mode", "win", "ups", "Hl", "Wl", "org_y", "org_x", "pos_mul", "pos_add",
              "cin_off", "cin_len"):
        setattr(g, f, kw.get(f, 0))
    Hl = g.Hl if (g.win or g.ups) else H
    Wl = g.Wl if (g.win or g.ups) else W
    Ho = (Hl + 2 * g.pad - g.dil * (g.k - 1) - 1) // g.stride + 1
    Wo = (Wl + 2 * g.pad - g.dil * (g.k - 1) - 1) // g.stride + 1
    y = np.zeros((B, g.Cout, Ho, Wo), dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float32)
    res = None if res is None else np.ascontiguousarray(res, dtype=np.float32)
    pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.int32)
    _lib.check(_lib.lib().smk_host_conv2d_ex(ctypes.byref(g), _fp(x), _fp(w), _fp(b), _fp(res), _fp(pos), _fp(y)))
    return y


RNG = np.random.default_rng(7)


@pytest.mark.parametrize("cin,cout,k,stride,pad,dil,hw", [
    (3, 16, 7, 2, 0, 1, 31),      # stem class: 7x7 s2 p0, Cin=3 padded to 8
    (16, 24, 1, 1, 0, 1, 9),      # 1x1
    (16, 16, 3, 1, 1, 1, 9),      # 3x3 s1 p1
    (16, 8, 3, 2, 0, 1, 13),      # 3x3 s2 p0 (layer2.0)
    (8, 8, 3, 1, 2, 2, 11),       # 3x3 d2 p2 (layer3.1-5)
    (8, 12, 3, 1, 0, 1, 9),       # 3x3 p0 (conv_search / conv_kernel)
    (4, 1, 3, 1, 1, 1, 10),       # Refine tail: Cin=4 (padded to 8), Cout=1
])
def test_host_walk_matches_oracle_conv(cin, cout, k, stride, pad, dil, hw):
    x = RNG.normal(size=(2, cin, hw, hw)).astype(np.float32)
    w = RNG.normal(size=(cout, cin, k, k)).astype(np.float32)
    b = RNG.normal(size=(cout,)).astype(np.float32)
    ref = O.conv2d(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), stride, pad, dil)
    got = host_conv(x, w, b, stride=stride, pad=pad, dil=dil)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() < 1e-4
    res = RNG.normal(size=ref.shape).astype(np.float32)
    got = host_conv(x, w, b, res=res, stride=stride, pad=pad, dil=dil, relu=1, res_mode=1)
    assert np.abs(got - np.maximum(ref + res, 0)).max() < 1e-4
    got = host_conv(x, w, b, res=res, stride=stride, pad=pad, dil=dil, relu=1, res_mode=2)
    assert np.abs(got - (np.maximum(ref, 0) + res)).max() < 1e-4


def test_refine_window_and_positions():
    """F.pad(f, n)[..., m*y:m*y+S, m*x:m*x+S] then conv3x3 p1 (custom.py:133-135)."""
    w = RNG.normal(size=(16, 8, 3, 3)).astype(np.float32)
    pos = np.array([[0, 24], [12, 12], [24, 3]], dtype=np.int32)
    for mul, padn, S, F in ((1, 4, 15, 31), (2, 8, 31, 63)):
        f = RNG.normal(size=(3, 8, F, F)).astype(np.float32)
        fp = np.pad(f, ((0, 0), (0, 0), (padn, padn), (padn, padn))).astype(np.float64)
        ref = np.concatenate([
            O.conv2d(fp[b:b + 1, :, mul * y:mul * y + S, mul * x:mul * x + S], w.astype(np.float64), None, 1, 1, 1)
            for b, (y, x) in enumerate(pos)])
        got = host_conv(f, w, pos=pos, pad=1, win=1, Hl=S, Wl=S, pos_mul=mul, pos_add=-padn)
        assert np.abs(got - ref).max() < 1e-4


def test_template_centre_crop_and_gather():
    """ResDownS crop x[:, :, 4:-4, 4:-4] folded into the 1x1 conv (custom.py:21-24) and the
    corr_feature[:, :, y, x] gather of Refine (custom.py:145) as a 1x1 window."""
    x = RNG.normal(size=(2, 16, 15, 15)).astype(np.float32)
    w = RNG.normal(size=(8, 16, 1, 1)).astype(np.float32)
    ref = O.conv2d(x.astype(np.float64), w.astype(np.float64))[:, :, 4:-4, 4:-4]
    got = host_conv(x, w, win=1, Hl=7, Wl=7, org_y=4, org_x=4)
    assert np.abs(got - ref).max() < 1e-4
    pos = np.array([[3, 9], [14, 0]], dtype=np.int32)
    ref = np.stack([O.conv2d(x[b:b + 1, :, y:y + 1, xx:xx + 1].astype(np.float64), w.astype(np.float64))[0]
                    for b, (y, xx) in enumerate(pos)])
    got = host_conv(x, w, pos=pos, win=1, Hl=1, Wl=1, pos_mul=1)
    assert np.abs(got - ref).max() < 1e-4


def test_nearest_upsample_folded_into_conv():
    x = RNG.normal(size=(2, 8, 15, 15)).astype(np.float32)
    w = RNG.normal(size=(4, 8, 3, 3)).astype(np.float32)
    for size in (31, 61):
        ref = O.conv2d(O.upsample_nearest(x.astype(np.float64), size), w.astype(np.float64), None, 1, 1, 1)
        got = host_conv(x, w, pad=1, ups=1, Hl=size, Wl=size)
        assert np.abs(got - ref).max() < 1e-4


def test_channel_slice():
    x = RNG.normal(size=(1, 24, 6, 6)).astype(np.float32)
    w = RNG.normal(size=(5, 8, 1, 1)).astype(np.float32)
    ref = O.conv2d(x[:, 8:16].astype(np.float64), w.astype(np.float64))
    got = host_conv(x, w, cin_off=8, cin_len=8)
    assert np.abs(got - ref).max() < 1e-4


def test_upsample_map_equals_torch():
    """F.upsample(mode='nearest') index map == (dst*in)//out for the three sizes used."""
    import torch
    import torch.nn.functional as F
    for hin, hout in ((15, 31), (31, 61), (61, 127)):
        t = torch.arange(hin, dtype=torch.float32).view(1, 1, hin, 1).expand(1, 1, hin, hin).contiguous()
        up = F.interpolate(t, size=(hout, hout), mode="nearest")[0, 0, :, 0].numpy().astype(int)
        assert (up == (np.arange(hout) * hin) // hout).all()


def test_pack_cache_key_follows_the_checkpoint(tmp_path):
    """the packed-weight cache is keyed on (state dict, dtype, variant, ABI)."""
    import numpy as np
    from siammask_amd.custom import build
    a = build("rpn", dtype="f16", pack_cache=str(tmp_path))
    sd = [("w", np.arange(6, dtype=np.float32).reshape(2, 3)), ("b", np.zeros(2, dtype=np.float32))]
    p0 = a._pack_path(sd)
    assert p0 == a._pack_path([(n, v.copy()) for n, v in sd])
    sd2 = [("w", sd[0][1] + 1e-3), sd[1]]
    assert a._pack_path(sd2) != p0
    b = build("rpn", dtype="f32", pack_cache=str(tmp_path))
    assert b._pack_path(sd) != p0
    c = build("base", dtype="f16", pack_cache=str(tmp_path))
    assert c._pack_path(sd) != p0


def test_tuning_knobs_read_back():
    """smk_tune / smk_tune_get need no GPU: a knob reads back what was set, unknown names and out-of-range values are errors,
    and the defaults are the measured ones (four producer waves, the layer rule fitted with them, 128-row sequence tiles)."""
    from siammask_amd import _lib
    # the defaults are process-wide state that earlier tests of the same process may have moved (seq_fused_last records the
    # last sequence launched): read them in a fresh interpreter
    import json
    import subprocess
    import sys
    code = ("import json; from siammask_amd import _lib; print(json.dumps([_lib.tune_get(k) for k in "
            "('npw', 'wreg_policy', 'seq_tall', 'a_stage', 'seq_fuse', 'seq_fused_last')]))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    npw, wreg_policy, seq_tall, a_stage, seq_fuse, seq_fused_last = json.loads(r.stdout.strip().splitlines()[-1])
    assert (npw, wreg_policy, seq_tall, a_stage) == (4, 1, 2, 0)
    assert seq_fuse == 1 and seq_fused_last == 0      # conv3 + next conv1 pairs fused; nothing launched
    old = _lib.tune_get("npw")
    try:
        _lib.tune(npw=2)
        assert _lib.tune_get("npw") == 2
        with pytest.raises(RuntimeError):
            _lib.tune(npw=3)
        assert _lib.tune_get("npw") == 2
    finally:
        _lib.tune(npw=old)
    with pytest.raises(RuntimeError):
        _lib.tune_get("no_such_knob")
    with pytest.raises(RuntimeError):
        _lib.tune(no_such_knob=1)
    # one table drives smk_tune and smk_tune_get: every knob takes back what it reads, in a fresh interpreter (the defaults)
    src = open(os.path.join(REPO, "siammask_amd", "csrc", "tune.cpp")).read()
    table = src[src.index("static const Knob KNOBS[] = {"):]
    table = table[:table.index("};")]
    names = re.findall(r'\{"(\w+)", &\w+(?:\.\w+)?, "', table)            # (read-only diagnostics have no accepted values)
    assert len(names) == 56 and "npw" in names and "seq_fused_last" not in names
    code = ("import json; from siammask_amd import _lib\n"
            "for k in %r: _lib.tune(**{k: _lib.tune_get(k)})\n"
            "_lib.tune(seq_spoll=5, seq_kstag_mask=15)\n"
            "print(json.dumps([_lib.tune_get('seq_spoll'), _lib.tune_get('seq_kstag_mask'), _lib.tune_get('measure_build')]))" % (names,))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    spoll, kstag_mask, measure_build = json.loads(r.stdout.strip().splitlines()[-1])
    assert (spoll, kstag_mask) == (1, 7)
    if not measure_build:
        with pytest.raises(RuntimeError):
            _lib.tune(seq_fuse3=1)                    # a measured alternative: only in `make MEASURE=1` libraries
    old = _lib.tune_get("rf_wreg")
    try:
        with pytest.raises(RuntimeError):
            _lib.tune(rf_wreg=(9 << 4) | 1)           # tile code 9: past conv_wreg_kernel's eight shapes
        assert _lib.tune_get("rf_wreg") == old
    finally:
        _lib.tune(rf_wreg=old)


@pytest.mark.parametrize("name", ["pipe_join", "pipe_sig", "pipe_eager", "pipe_two_form", "pipe_prio", "concurrency", "mask_overlap"])
def test_settled_pipeline_knobs_are_gone(name):
    """the measured and dropped forms of the pipelined step (cross-queue event join, event / hipStreamWaitValue32 start of the tail,
    eager parts, depth-2 forms 0 / 2, a side-stream priority; profiles/r05a_*, r05e_*, r05f_*, r05j_*, r05o_*, r06z_*) left the library
    with their knobs: no kind of build sets or reads them any more.  So did the two modes that captured graphs with parallel branches:
    fork / join between independent launches and the mask head on a side stream (both measured slower, HISTORY.md round 1, profiles/r06q_*)"""
    from siammask_amd import _lib
    for value in (0, 1, 2):
        with pytest.raises(RuntimeError):
            _lib.tune(**{name: value})
    with pytest.raises(RuntimeError):
        _lib.tune_get(name)


# elements per image, one plane, of a context's activation arena at pipeline depth 0 (the sum of the allocations of smk_create)
ARENA_ELEMS = {"sharp": {"f16": 15263800, "f32": 9589432, "f16x3": 9589432},
               "base": {"f16": 14904584, "f32": 9230216, "f16x3": 9230216},
               "rpn": {"f16": 14362888, "f32": 8688520, "f16x3": 8688520}}


@pytest.mark.parametrize("variant", ["sharp", "base", "rpn"])
@pytest.mark.parametrize("dtype", ["f16", "f32", "f16x3"])
def test_arena_sizes(variant, dtype):
    """the engine's table of arena tensors sums to what the allocations summed to before there was a table; only f16 contexts (the
    persistent sequence's) hold the stage-private buffers of layer2 / layer3, the others alias them; pipelined steps add second
    copies of p0 / p1 / p2 (depth 1) and of head0 (depth 2)"""
    from siammask_amd import _lib

    def elems(depth):
        n = ctypes.c_uint64(0)
        _lib.check(_lib.lib().smk_host_arena_elems(_lib.DTYPE[dtype], _lib.VARIANT[variant], depth, ctypes.byref(n)))
        return n.value

    base = ARENA_ELEMS[variant][dtype]
    assert elems(0) == base
    assert elems(1) == base + 125 * 125 * 64 + 63 * 63 * 256 + 31 * 31 * 512 == base + 2508096
    assert elems(2) == elems(1) + 25 * 25 * 256 * (2 if variant == "rpn" else 3)
    n = ctypes.c_uint64(0)
    for bad in ((3, 2, 0), (1, 3, 0), (1, 2, 3), (1, 2, -1)):
        assert _lib.lib().smk_host_arena_elems(*bad, ctypes.byref(n)) != 0


def test_arena_tensors_are_stated_once():
    """every launch takes its view of an arena tensor from the engine's one table (act / ACT with a table id): no tensor is looked up by
    name, and none restates a shape beside a name -- in any host translation unit"""
    csrc = os.path.join(REPO, "siammask_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".cpp"))
    assert src.count("static const ArenaRow ARENA[T_COUNT] = {") == 1
    assert not re.findall(r'\b(?:act|ACT)\([^\n;]*"', src)             # a call of act / ACT with a string literal among its arguments
    assert "buf.at(" not in src and "buf.find(" not in src


def _plan(B, cin, hw, cout, k, stride=1, pad=0, dil=1, res=False, win=None, dtype="f16"):
    g = _lib.ConvGeom()
    g.B, g.Cin, g.H, g.W = B, cin, hw, hw
    g.Cout, g.k, g.stride, g.pad, g.dil = cout, k, stride, pad, dil
    g.relu = 1
    if win is not None:
        g.win, g.Hl, g.Wl = 1, win, win
    out = [ctypes.c_int(0) for _ in range(4)]
    _lib.check(_lib.lib().smk_host_plan_conv(ctypes.byref(g), _lib.DTYPE[dtype], int(res), *[ctypes.byref(o) for o in out]))
    kernel, bm, bn, cfg = [o.value for o in out]
    return ("igemm", "halo", "wreg", "pp")[kernel], (bm, bn), cfg


def test_layer_rules_are_the_measured_ones():
    """The kernel / workgroup-shape choice per layer is fitted to measurements (profiles/r02_producer_waves_2_vs_4.txt,
    r02_producer_waves_layers_b1_b64.json, r02b_seq_layer_clocks.txt).  smk_host_plan_conv exposes it without a GPU, so a
    change of the rule shows up here instead of as a silent slowdown.  (kernel, workgroup shape, tile code inside a
    persistent sequence or -1)."""
    # B = 8 (headline): layer2 / layer3 / adjust run inside the sequences -> the sequence tile code is what counts
    assert _plan(8, 1024, 31, 256, 1)[2] == 1                                  # l3.c1   64x128
    assert _plan(8, 256, 31, 256, 3, pad=2, dil=2)[2] == 24                    # l3.c2   128 pixels (4 whole rows) x 64, patch shared by the taps
    assert _plan(8, 256, 31, 256, 3, pad=1)[2] == 24                           # l3.0.c2 (dilation 1)
    assert _plan(8, 256, 15, 256, 3, pad=2, dil=2)[2] == 25                    # ... on the 15x15 template: 64 pixels (4 rows) x 64
    assert _plan(8, 256, 31, 1024, 1, res=True)[2] == 3                        # l3.c3   128x256 (two 64-row rounds otherwise)
    assert _plan(8, 512, 31, 1024, 3, pad=1)[2] == 3                           # l3.0.ds 128x256 (long K too, seq_tall = 2)
    assert _plan(8, 256, 63, 512, 3, stride=2)[2] == 0                         # l2.0.ds 64x256 (one round)
    assert _plan(8, 256, 63, 128, 1)[2] == 4                                   # l2.0.c1 on the 63x63 input: 128x128
    assert _plan(8, 128, 31, 128, 3, pad=1)[2] == 25                           # l2.c2   64 pixels (2 whole rows) x 64, patch shared
    assert _plan(8, 128, 31, 512, 1, res=True)[2] == 0                         # l2.c3   64x256
    # B = 8 per launch
    assert _plan(8, 256, 31, 768, 3)[:2] == ("wreg", (96, 256))                # conv_search (N-fused 768): 213 tiles of 96 rows = ONE round (128 rows: 159 tiles
                                                                               # on 256 CUs, each a third longer; round 5, profiles/r05d_wreg96_ab.txt)
    assert _plan(8, 64, 63, 64, 3, pad=1)[0] == "halo"                         # l1.c2: short-K 3x3 stays on the patch kernel
    assert _plan(8, 64, 63, 256, 1, res=True)[:2] == ("igemm", (128, 128))     # l1.c3: large M, short K
    assert _plan(8, 256, 63, 64, 1)[0] == "igemm"                              # l1.c1
    assert _plan(8, 3, 255, 64, 7, stride=2)[0] == "igemm"                     # stem
    assert _plan(8, 512, 31, 128, 3, pad=1, win=15)[:2] == ("wreg", (32, 64))  # Refine v2.0 on its own: 58 tiles of 64 rows -> 114 of 32 (round 6, wreg32)
    # B = 1: almost everything on the register-fed kernel, 64x64 tiles -- 32x64 (round 6, profiles/r06w_wreg_32_row_tiles.txt) where fewer than 140 of those exist
    for args, tile in (((1024, 31, 256, 1), (32, 64)), ((256, 31, 1024, 1), (64, 64)), ((512, 31, 128, 1), (32, 64)), ((256, 63, 64, 1), (32, 64))):
        assert _plan(1, *args)[:2] == ("wreg", tile), args
    assert _plan(1, 256, 31, 256, 3, pad=2, dil=2)[:2] == ("wreg", (32, 64))   # l3.c2: 64 tiles of 64 rows
    assert _plan(2, 256, 31, 256, 3, pad=2, dil=2)[:2] == ("wreg", (32, 64))   # ... 124 at B = 2
    assert _plan(3, 256, 31, 256, 3, pad=2, dil=2)[:2] == ("wreg", (64, 64))   # ... 184 at B = 3
    assert _plan(1, 128, 31, 128, 3, pad=1)[0] == "halo"                       # l2.c2 (K = 1152)
    # B = 64: wide / long-K layers on 128x256 register-fed tiles, narrow short-K ones on LDS-staged 128-row tiles
    assert _plan(64, 1024, 31, 256, 1)[:2] == ("wreg", (128, 256))             # l3.c1
    # ... and from round 6 the long-K 3x3 layers whose 256 x 256 tiles fill whole rounds on conv_pp_kernel (profiles/r06a_pp_first_contact.txt)
    assert _plan(64, 256, 31, 256, 3, pad=2, dil=2)[:2] == ("pp", (256, 256))  # l3.c2: 241 tiles = 0.94 of one round
    assert _plan(64, 512, 31, 1024, 3, pad=1)[:2] == ("pp", (256, 256))        # l3.0.ds: 964 tiles = 0.94 of four rounds
    assert _plan(64, 256, 63, 512, 3, stride=2)[:2] == ("pp", (256, 256))      # l2.0.ds
    assert _plan(32, 256, 31, 256, 3, pad=2, dil=2)[0] != "pp"                 # B = 32: 121 tiles, a partial round of long tiles
    assert _plan(64, 256, 31, 1024, 1, res=True)[:2] == ("wreg", (128, 256))   # l3.c3
    assert _plan(64, 256, 31, 768, 3)[:2] == ("wreg", (128, 256))              # conv_search: 633 tiles of 256 x 256 = 2.47 rounds (0.82 of three): stays
    assert _plan(64, 512, 31, 128, 1)[0] == "igemm"                            # l2.c1
    assert _plan(64, 256, 63, 64, 1)[0] == "igemm"                             # l1.c1
    assert _plan(64, 128, 31, 128, 3, pad=1)[0] == "halo"                      # l2.c2
    # Refine's h* / post* layers (fp16 3x3 stride 1 on 32 / 16 / 4 channels): no halo pack (channels not a multiple of 64), conv_igemm
    for B in (1, 8, 64):
        for cin, hw, cout in ((32, 15, 32), (32, 31, 16), (16, 31, 16), (16, 61, 4), (4, 61, 4), (4, 127, 1)):
            assert _plan(B, cin, hw, cout, 3, pad=1)[0] == "igemm", (B, cin, hw, cout)
    # fp32: no register-fed kernel, no sequences
    assert _plan(8, 1024, 31, 256, 1, dtype="f32")[0] == "igemm" and _plan(8, 1024, 31, 256, 1, dtype="f32")[2] == -1


# ---- persistent sequences: the marks plan_seq puts on a recorded list (smk_host_plan_seq) ----------------------------------
SEQ_PAIR_L3, SEQ_PAIR_L2, SEQ_PAIR_2ND = 20, 21, 22                 # smk_kernels.h SEQ_CFG_C3C1_*
SEQ_TRIPLE_L3, SEQ_TRIPLE_L2, SEQ_TRIPLE_MID = 28, 29, 30           # SEQ_CFG_C2C3C1_*
YRES_IN, YRES_NOSTORE, LDS_HI = 2, 4, 8                             # SEQ_YRES_IN, SEQ_YRES_NOSTORE, SEQ_LDS_HI


class _knobs:
    """smk_tune for the duration of a with-block, then back to what was there"""
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: _lib.tune_get(k) for k in self.kw}
        _lib.tune(**self.kw)

    def __exit__(self, *exc):
        _lib.tune(**self.old)


def _plan_seq(B, S, layers, want_outputs=True):
    from siammask_amd import ops
    return ops.plan_seq((B, layers[0]["w"].shape[1], S, S), layers, want_outputs)


@pytest.mark.parametrize("shape,B,S", [((1024, 256), 8, 31), ((1024, 256), 3, 15), ((512, 128), 8, 31), ((512, 128), 5, 15)])
def test_seq_plan_resident_trunk(shape, B, S):
    """The lists of tests/test_gpu_seq.py test_conv_seq_resident_trunk_gives_the_same_bits: three Bottlenecks + adjust fuse into
    three pairs, and the second and third pair find their residual resident (the conv2 between them works above it in LDS).
    The first two pairs skip the store of their output only while nobody reads it back; with two images on a team (B = 10) or
    smk_tune seq_yres 0 nothing is marked."""
    from helpers import seq_chain
    cin, planes = shape
    layers = seq_chain(np.random.default_rng(0), cin, planes, 3, 2 if cin == 1024 else 1)
    last = len(layers) - 1
    pair = SEQ_PAIR_L3 if cin == 1024 else SEQ_PAIR_L2
    every = _plan_seq(B, S, layers)
    cfg = [c for c, _, _ in every]
    assert [cfg[i] for i in (2, 3, 5, 6, 8, 9)] == [pair, SEQ_PAIR_2ND] * 3, cfg
    assert cfg.count(SEQ_PAIR_2ND) == 3
    marks = {i: a for i, (_, _, a) in enumerate(every) if a}
    assert marks == {4: LDS_HI, 5: YRES_IN, 7: LDS_HI, 8: YRES_IN}, marks
    only = {i: a for i, (_, _, a) in enumerate(_plan_seq(B, S, layers, want_outputs=(last,))) if a}
    assert only == {2: YRES_NOSTORE, 4: LDS_HI, 5: YRES_IN | YRES_NOSTORE, 7: LDS_HI, 8: YRES_IN}, only
    first = {i: a for i, (_, _, a) in enumerate(_plan_seq(B, S, layers, want_outputs=(2, last))) if a}
    assert first == {4: LDS_HI, 5: YRES_IN | YRES_NOSTORE, 7: LDS_HI, 8: YRES_IN}, first
    assert not any(a for _, _, a in _plan_seq(10, 15, layers, want_outputs=(last,)))
    with _knobs(seq_yres=0):
        plain = _plan_seq(B, S, layers, want_outputs=(last,))
    assert [c for c, _, _ in plain] == cfg and not any(a for _, _, a in plain)


def test_seq_plan_no_pairs_without_seq_fuse():
    """smk_tune seq_fuse 0: no pairs, hence nothing resident; planning on the host leaves the "..._last" diagnostics alone"""
    from helpers import seq_chain
    layers = seq_chain(np.random.default_rng(1), 1024, 256, 3, 2)
    last = [_lib.tune_get(k) for k in ("seq_fused_last", "seq_fused3_last", "seq_yres_last")]
    with _knobs(seq_fuse=0):
        got = _plan_seq(8, 31, layers)
    assert not {SEQ_PAIR_L3, SEQ_PAIR_L2, SEQ_PAIR_2ND} & {c for c, _, _ in got} and not any(a for _, _, a in got), got
    assert _plan_seq(8, 31, layers)[2][0] == SEQ_PAIR_L3
    assert [_lib.tune_get(k) for k in ("seq_fused_last", "seq_fused3_last", "seq_yres_last")] == last


def test_seq_plan_reader_in_a_later_launch_keeps_the_store():
    """A list longer than one launch (36 records): twelve layer2 Bottlenecks + adjust, then a 1x1 convolution in the second launch
    that reads the output of the first pair.  That pair's Y must reach memory; without the late reader it need not.  Pairs stay
    inside their launch: the last Bottleneck's conv3 (record 35) and adjust (record 36) are not fused."""
    from helpers import seq_chain, seq_weight
    rng = np.random.default_rng(2)
    layers = seq_chain(rng, 512, 128, 12, 1)
    assert len(layers) == 37
    alone = _plan_seq(8, 31, layers, want_outputs=(36,))
    late = layers + [dict(w=seq_weight(rng, 128, 512, 1), relu=True, src=2)]
    got = _plan_seq(8, 31, late, want_outputs=(37,))
    for plan in (alone, got):
        cfg = [c for c, _, _ in plan]
        assert [i for i, c in enumerate(cfg) if c == SEQ_PAIR_L2] == list(range(2, 33, 3)), cfg
        assert cfg[35] != SEQ_PAIR_L2 and cfg[36] != SEQ_PAIR_2ND
        assert [i for i, (_, _, a) in enumerate(plan) if a & YRES_IN] == list(range(5, 33, 3))
    assert [i for i, (_, _, a) in enumerate(alone) if a & YRES_NOSTORE] == list(range(2, 30, 3))
    assert [i for i, (_, _, a) in enumerate(got) if a & YRES_NOSTORE] == list(range(5, 30, 3))


def _needs_measure_build():
    if not _lib.tune_get("measure_build"):
        pytest.skip("the triple routine (seq_fuse3) is only in a library built with `make MEASURE=1`")


@pytest.mark.parametrize("shape,dil", [((1024, 256), 2), ((1024, 256), 1), ((512, 128), 1)])
@pytest.mark.parametrize("B,S", [(8, 31), (3, 29), (10, 31)])
def test_seq_plan_triples(shape, dil, B, S):
    """The lists of tests/test_gpu_seq.py test_conv_seq_fused_triples: with seq_fuse3 every Bottleneck's [conv2, conv3, next 1x1]
    is one triple, without a barrier behind conv2, each residual in front of the wait (the list input, then the previous triple's
    conv3 on the same rows).  A conv2 output that is read back keeps its triple off."""
    _needs_measure_build()
    from helpers import seq_chain
    cin, planes = shape
    layers = seq_chain(np.random.default_rng(3), cin, planes, 3, dil)
    keep = [i for i in range(len(layers)) if i % 3 != 1 or i == len(layers) - 1]
    code = SEQ_TRIPLE_L3 if cin == 1024 else SEQ_TRIPLE_L2
    with _knobs(seq_fuse3=1):
        got = _plan_seq(B, S, layers, want_outputs=keep)
        read_back = _plan_seq(B, S, layers)
    assert [c for c, _, _ in got][1:] == [code, SEQ_TRIPLE_MID, SEQ_PAIR_2ND] * 3, got
    assert [got[i][1] for i in (1, 4, 7)] == [0, 0, 0] and [got[i][2] for i in (2, 5, 8)] == [0, 0, 0]
    assert SEQ_TRIPLE_MID not in [c for c, _, _ in read_back]
    assert [c for c, _, _ in read_back].count(SEQ_PAIR_2ND) == 3
    with _knobs(seq_fuse3=0):
        assert SEQ_TRIPLE_MID not in [c for c, _, _ in _plan_seq(B, S, layers, want_outputs=keep)]


def test_seq_plan_triples_leave_short_rows_and_shared_conv2_outputs_alone():
    """tests/test_gpu_seq.py test_conv_seq_triples_leave_short_rows_and_shared_conv2_outputs_alone, and the same across a launch
    boundary: the 15 x 15 template rows keep the pairs; a conv2 output that another record reads -- in the same launch or in
    the next one -- reaches memory"""
    _needs_measure_build()
    from helpers import seq_chain, seq_weight
    rng = np.random.default_rng(4)
    with _knobs(seq_fuse3=1):
        got = _plan_seq(8, 15, seq_chain(rng, 1024, 256, 2, 2), want_outputs=False)
        assert [c for c, _, _ in got].count(SEQ_PAIR_2ND) == 2 and SEQ_TRIPLE_MID not in [c for c, _, _ in got]
        layers = seq_chain(rng, 1024, 256, 1, 2)
        layers.append(dict(w=seq_weight(rng, 256, 256, 1), relu=True, src=1))
        assert SEQ_TRIPLE_MID not in [c for c, _, _ in _plan_seq(8, 31, layers, want_outputs=False)]
        layers = seq_chain(rng, 1024, 256, 12, 2)
        alone = _plan_seq(8, 31, layers, want_outputs=False)
        assert [c for c, _, _ in alone][1:4] == [SEQ_TRIPLE_L3, SEQ_TRIPLE_MID, SEQ_PAIR_2ND]
        late = _plan_seq(8, 31, layers + [dict(w=seq_weight(rng, 256, 256, 1), relu=True, src=1)], want_outputs=False)
        assert late[1][0] != SEQ_TRIPLE_L3 and late[2][0] == SEQ_PAIR_L3
