"""VOS datasets through the B slots, the host half: the scheduler siammask_amd.dataset.plan_vos (pure numpy), every
SMK_E_ARG of smk_vos_rle_v / smk_vos_rle_dev_v (no device: the pointers are host memory never read), and every ValueError of
dataset.run_vos, none of which reaches the tracker's reserve / enqueue / start."""
import ctypes
from unittest import mock

import numpy as np
import pytest
import torch

from siammask_amd import _lib, dataset, preproc


# ---- 1. plan_vos ----------------------------------------------------------------------------------------------------------------------
def _check_plan(p, lengths, n_obj, B):
    V = len(lengths)
    held = np.full((p.G, B), -1)
    for v in range(V):
        s, g = p.slots[v], int(p.first_step[v])
        assert len(s) == n_obj[v] == len(set(s)) and list(s) == sorted(s) and 0 <= s[0] and s[-1] < B, v
        assert 0 <= g and g + lengths[v] <= p.G
        for b in s:
            assert (held[g:g + lengths[v], b] == -1).all(), "slot %d is held twice" % b          # no slot, two videos, one step
            held[g:g + lengths[v], b] = v
    for v in range(V):                                                  # exactly `length` consecutive steps on n_obj slots
        steps = np.nonzero((held == v).any(axis=1))[0]
        assert steps.tolist() == list(range(int(p.first_step[v]), int(p.first_step[v]) + lengths[v]))
        assert ((held == v).sum(axis=1)[steps] == n_obj[v]).all()
    assert p.G <= sum(lengths) and (held[-1] >= 0).any() and (held >= 0).any(axis=1).all()
    assert p.efficiency == sum(n * t for n, t in zip(n_obj, lengths)) / (p.G * B) == (held >= 0).mean()
    for g in range(p.G):                                                # the groups of a step are the videos that hold slots on it
        assert sorted(v for v, _ in p.steps[g]) == sorted(set(held[g][held[g] >= 0].tolist()))
        assert all(list(s) == list(p.slots[v]) for v, s in p.steps[g])
    return held


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("order", dataset.ORDERS)
def test_plan_vos_properties(seed, order):
    rng = np.random.default_rng(seed)
    B, V = int(rng.integers(1, 9)), int(rng.integers(1, 12))
    lengths = rng.integers(1, 9, V).tolist()
    n_obj = rng.integers(1, B + 1, V).tolist()
    p = dataset.plan_vos(lengths, n_obj, B, order)
    held = _check_plan(p, lengths, n_obj, B)
    assert set(held[held >= 0].tolist()) == set(range(V))               # every video is placed
    # first fit on the lowest free slots: a video that starts on step g > 0 did not fit on step g - 1 beside what ran there
    for v in range(V):
        g = int(p.first_step[v])
        if g:
            before = [u for u in range(V) if p.first_step[u] < g and p.first_step[u] + lengths[u] > g - 1]
            assert sum(n_obj[u] for u in before) + n_obj[v] > B, v
        free = [b for b in range(B) if g == 0 or held[g - 1, b] == -1 or held[g, b] != held[g - 1, b]]
        assert p.slots[v][0] >= min(free)


def test_plan_vos_hand_cases():
    p = dataset.plan_vos((6, 4, 5, 2), (2, 1, 3, 1), 4)                 # video 3 overtakes video 2, which needs three slots
    _check_plan(p, (6, 4, 5, 2), (2, 1, 3, 1), 4)
    assert p.slots == [[0, 1], [2], [0, 1, 2], [3]] and p.first_step.tolist() == [0, 0, 6, 0] and p.G == 11
    assert p.efficiency == 33 / 44
    assert p.steps[0] == [(0, [0, 1]), (1, [2]), (3, [3])] and p.steps[2] == [(0, [0, 1]), (1, [2])] and p.steps[6] == [(2, [0, 1, 2])]
    q = dataset.plan_vos((6, 4, 5, 2), (2, 1, 3, 1), 4, "longest")      # 6, 5, 4, 2: the three-object video still has to wait
    assert q.slots == p.slots and q.first_step.tolist() == p.first_step.tolist()
    r = dataset.plan_vos((2, 5, 3), (1, 1, 1), 2, "longest")            # the longest first, ties and the rest in the given order
    assert r.slots == [[1], [0], [1]] and r.first_step.tolist() == [3, 0, 0] and r.G == 5
    full = dataset.plan_vos((3, 2, 4), (4, 1, 4), 4)                    # n_obj = B: the video runs alone
    assert full.slots == [[0, 1, 2, 3], [0], [0, 1, 2, 3]] and full.first_step.tolist() == [0, 3, 5] and full.G == 9
    one = dataset.plan_vos([7], [3], 8)
    assert one.G == 7 and one.slots == [[0, 1, 2]] and one.efficiency == 21 / 56 and len(one.steps) == 7


def test_plan_vos_refusals():
    for bad in (lambda: dataset.plan_vos([], [], 4), lambda: dataset.plan_vos([3, 2], [1], 4), lambda: dataset.plan_vos([3, 0], [1, 1], 4),
                lambda: dataset.plan_vos([3], [0], 4), lambda: dataset.plan_vos([3], [5], 4), lambda: dataset.plan_vos([3], [1], 0),
                lambda: dataset.plan_vos([3], [1], 2.5), lambda: dataset.plan_vos([3], [1], 4, "shortest")):
        with pytest.raises(ValueError, match="plan_vos"):
            bad()


# ---- 2. the C entries: every SMK_E_ARG, with no device ----------------------------------------------------------------------------------
def test_symbols_and_argument_checks_of_the_entries():
    L = _lib.lib()
    for s in ("smk_vos_rle_v", "smk_vos_rle_dev_v"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert L.smk_version() == (1 << 16) | 10                            # additive: the symbols are the probe
    E = -1
    buf = np.zeros(4096, np.float64)
    f, odd4, odd2 = buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(buf.ctypes.data + 4), ctypes.c_void_p(buf.ctypes.data + 2)
    Bn, cw, ch = 8, 70, 45
    need = L.smk_rle_workspace(Bn, cw, ch)
    masks = lambda *m: np.array(m, dtype=np.uint32)
    wh = lambda *s: np.array(s, dtype=np.int32).reshape(-1, 2)
    ptrs = lambda *p: (ctypes.c_void_p * len(p))(*p)
    gm, gs = masks(0b100101, 0b10, 0b10001000), wh(70, 45, 33, 41, 64, 1)
    keep = [gm, gs]

    def call(fn, order, k):
        a = dict(order, **k)
        for n in ("masks", "wh"):
            if isinstance(a[n], np.ndarray):
                keep.append(a[n])
                a[n] = a[n].ctypes.data_as(ctypes.c_void_p)
        return fn(*[a[n] for n, _ in order])
    tail = (("G", 3), ("masks", gm), ("wh", gs), ("init", None), ("live", 7), ("border", -1.0), ("ids", f), ("alive", 0b10101111),
            ("seg", 0.35), ("given", 0), ("cap", 100), ("ws", f), ("ws_bytes", need), ("counts", f), ("meta", f), ("stream", None))
    host = (("logits", f), ("ms", 127), ("inv", f), ("B", Bn), ("W", cw), ("H", ch)) + tail
    dev = (("logits", f), ("head", None), ("S", 25), ("ms", 127), ("state", f), ("slot", 0), ("B", Bn), ("W", cw), ("H", ch)) + tail
    shared = (
        dict(logits=None), dict(ids=None), dict(masks=None), dict(wh=None), dict(ws=None), dict(counts=None), dict(meta=None),    # null
        dict(B=0), dict(B=-1), dict(B=33), dict(G=0), dict(G=-2), dict(G=9),                                 # B or G out of range
        dict(masks=masks(0b100101, 0, 0b10001000)),                                                           # an empty group
        dict(masks=masks(0b100101, 0b100, 0b10001000)), dict(masks=masks(0b1, 0b10, 0b11)),                   # overlapping groups
        dict(masks=masks(0b100101, 0b10, 0b110001000)), dict(masks=masks(0b1, 0b10, 1 << 31)),                # bits at or above B
        dict(wh=wh(71, 45, 33, 41, 64, 1)), dict(wh=wh(70, 45, 33, 46, 64, 1)), dict(wh=wh(70, 45, 0, 41, 64, 1)),
        dict(wh=wh(70, 45, 33, 41, 64, -1)),                                                                  # a size outside the canvas
        dict(given=0b10), dict(given=0b10, init=ptrs(f, None, f)), dict(given=0b1000, init=ptrs(f, f, None)),   # given, no init labels
        dict(given=0b10000, init=ptrs(f, f, f)), dict(given=1 << 31, init=ptrs(f, f, f)),                     # given outside every group
        dict(alive=0b1010000), dict(alive=0b10101111 | (1 << 20)),                                            # alive outside every group
        dict(cap=0), dict(cap=-1), dict(cap=cw * ch + 2),                                                     # a bad cap
        dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=odd4), dict(counts=odd2), dict(meta=odd2),         # short / misaligned
        dict(W=0), dict(H=0), dict(W=4097), dict(H=4097), dict(W=69), dict(ms=0))
    for bad in shared + (dict(inv=None),):
        assert call(L.smk_vos_rle_v, host, bad) == E, bad
        assert b"smk_vos_rle_v" in L.smk_last_error(), bad
    for bad in shared + (dict(state=None), dict(slot=2), dict(slot=-1), dict(head=f, S=0), dict(head=f, S=1025),
                         dict(logits=None, head=None)):
        assert call(L.smk_vos_rle_dev_v, dev, bad) == E, bad
        assert b"smk_vos_rle_dev_v" in L.smk_last_error(), bad
    for bad, word in ((dict(masks=masks(0b100101, 0, 0b10001000)), b"empty"), (dict(masks=masks(0b1, 0b10, 0b11)), b"overlaps"),
                      (dict(given=0b10), b"init labels"), (dict(alive=0b1010000), b"outside every group"),
                      (dict(cap=cw * ch + 2), b"3151"), (dict(wh=wh(71, 45, 33, 41, 64, 1)), b"canvas")):
        assert call(L.smk_vos_rle_v, host, bad) == E and word in L.smk_last_error(), bad


def test_the_python_wrappers_check_the_groups_before_the_library():
    ok = dict(B=8, canvas_wh=(70, 45), groups=[[0, 2, 5], [1], [3, 7]], sizes=[(70, 45), (33, 41), (64, 1)], object_ids=list(range(8)))
    v = preproc.VosGroups(**ok)
    assert v.masks.tolist() == [0b100101, 0b10, 0b10001000] and v.alive == 0b10101111 and v.given == 0 and v.live == 7
    assert preproc.VosGroups(**dict(ok, live=[True, False, True], alive=[True] + [False] * 7)).live == 5
    for bad in (dict(B=0), dict(B=33), dict(groups=[]), dict(groups=[[0], []], sizes=[(1, 1)] * 2), dict(groups=[[0, 1], [1]], sizes=[(1, 1)] * 2),
                dict(groups=[[8]], sizes=[(1, 1)]), dict(groups=[[0, 0]], sizes=[(1, 1)]), dict(sizes=[(70, 45), (33, 41)]),
                dict(sizes=[(71, 45), (33, 41), (64, 1)]), dict(sizes=[(70, 45), (33, 0), (64, 1)]), dict(object_ids=[1, 2]),
                dict(object_ids=[256] * 8), dict(alive=[True] * 8), dict(given=[False] * 4 + [True] + [False] * 3),
                dict(given=[True] + [False] * 7), dict(live=[True]), dict(canvas_wh=(4097, 45)), dict(init=[None])):
        with pytest.raises(ValueError, match="vos_rle_v"):
            preproc.VosGroups(**dict(ok, **bad))


# ---- 3. run_vos: every refusal, and none of them launches anything ---------------------------------------------------------------------
DEV = torch.device("cuda", 0)


def _tensor(*shape):
    """what the checks take for a contiguous uint8 CUDA tensor of a shape (no device here)"""
    t = mock.MagicMock(spec=torch.Tensor)
    t.is_cuda, t.dtype, t.shape, t.device = True, torch.uint8, torch.Size(shape), DEV
    t.dim.return_value = len(shape)
    t.is_contiguous.return_value = True
    return t


def _video(T=5, h=40, w=60, ids=(3, 7), **kw):
    d = {"frames": _tensor(T, h, w, 3), "object_ids": list(ids), "start": {i: 0 for i in ids}, "end": {str(i): T - 1 for i in ids},
         "init": _tensor(h, w)}
    d.update(kw)
    return d


def _tracker(variant="sharp", hp=None, max_batch=4):
    tr = mock.MagicMock()
    tr.model.variant, tr.model._max_batch = variant, max_batch
    tr.get_hp.return_value = hp
    return tr


def test_run_vos_refuses_before_any_launch():
    good = [_video(), _video(T=3, h=30, w=50, ids=(9,))]
    cases = [
        (dict(tr=_tracker("rpn")), "mask branch"), (dict(tr=_tracker(hp={"lr": [0.5] * 4})), "hp table"),
        (dict(videos=[_video(ids=(1, 2, 3, 4, 5))]), "objects"), (dict(videos=[_video(ids=())]), "objects"),
        (dict(videos=[_video(ids=(1, 2, 3))], B=2), "objects"),
        (dict(videos=[_video(start={3: 0})]), "missing"), (dict(videos=[_video(end={3: 4})]), "missing"),
        (dict(videos=[_video(start={3: 0, 7: 5})]), "starts on frame"), (dict(videos=[_video(start={3: -1, 7: 0})]), "starts on frame"),
        (dict(videos=[_video(init=_tensor(41, 60))]), "init"), (dict(videos=[_video(init=_tensor(4, 40, 60))]), "init"),
        (dict(videos=[_video(init=None)]), "init"), (dict(videos=[_video(ids=(3, 3))]), "distinct"), (dict(videos=[_video(ids=(3, 256))]), "0..255"),
        (dict(cap=0), "cap"), (dict(cap=40 * 60 + 2), "cap"), (dict(cap=2.5), "cap"), (dict(cap=True), "cap"),
        (dict(chunk=0), "chunk"), (dict(chunk=1.5), "chunk"), (dict(videos=[]), "at least one"), (dict(order="shortest"), "order"),
        (dict(B=0), "B in"), (dict(B=33), "B in"), (dict(videos=[{"frames": _tensor(5, 40, 60, 3)}]), "video 0"),
        (dict(videos=[_video(frames=_tensor(5, 40, 60))]), "frames"), (dict(videos=[_video(T=5, h=5000, w=8)]), "4096"),
    ]
    for kw, word in cases:
        tr = kw.pop("tr", None) or _tracker()
        args = dict(dict(videos=good, B=None, order="longest", cap=None, chunk=256), **kw)
        with pytest.raises(ValueError, match=word):
            dataset.run_vos(tr, args["videos"], B=args["B"], order=args["order"], cap=args["cap"], chunk=args["chunk"])
        called = [c[0] for c in tr.method_calls if c[0] != "get_hp"]
        assert not called and not tr.model.method_calls, (kw, called)
    cpu = _video()
    cpu["frames"].is_cuda = False
    with pytest.raises(RuntimeError, match="MI355X"):
        dataset.run_vos(_tracker(), [cpu])
