"""The scheduler of siammask_amd.dataset on the host: plan() against its stated rule and a reference simulation
written here, a hand-checked case, its refusals, and the gather step of run_videos on fabricated chunks."""
import numpy as np
import pytest

from siammask_amd import dataset


def _lengths(V, seed):
    return [int(n) for n in np.random.default_rng(seed).integers(2, 30, V)]


def _simulate(lengths, B, order):
    """the rule, step by step: a clock, B slots with the frames they still owe, a queue of videos; a slot that has nothing left takes
    the head of the queue (lowest slot first) before the step is made -> (G, slot_of, first_step)"""
    V = len(lengths)
    queue = sorted(range(V), key=lambda v: -lengths[v]) if order == "longest" else list(range(V))
    owed, slot_of, first = [0] * B, [None] * V, [None] * V
    g = 0
    while True:
        for b in range(B):
            if owed[b] == 0 and queue:
                v = queue.pop(0)
                owed[b], slot_of[v], first[v] = lengths[v] - 1, b, g
        if not any(owed):
            return g, slot_of, first
        owed = [max(n - 1, 0) for n in owed]
        g += 1


CASES = [(V, B, order) for V in (1, 2, 7, 40) for B in (1, 2, 8) for order in ("given", "longest")]


@pytest.mark.parametrize("V,B,order", CASES)
def test_plan_properties(V, B, order):
    lengths = _lengths(V, 100 * V + B)
    p = dataset.plan(lengths, B, order)
    G, table = p.G, p.table
    assert table.shape == (G, B, 2) and table.dtype == np.int32 and len(p.starts) == G
    # every (v, t), 1 <= t < T_v, exactly once; nothing else
    seen = [tuple(x) for x in table.reshape(-1, 2).tolist() if x[0] >= 0]
    assert sorted(seen) == [(v, t) for v in range(V) for t in range(1, lengths[v])]
    assert all(x[1] == -1 for x in table.reshape(-1, 2).tolist() if x[0] < 0)
    # a video's frames: one slot, consecutive steps, in order
    for v in range(V):
        g, b = np.nonzero(table[:, :, 0] == v)
        assert set(b.tolist()) == {int(p.slot_of[v])} and g.tolist() == list(range(int(p.first_step[v]), int(p.first_step[v]) + lengths[v] - 1))
        assert table[g, b, 1].tolist() == list(range(1, lengths[v]))
    # started once, behind the step before its frame 1, in the slot the table shows
    where = {v: ("initial", s) for s, v in p.initial}
    assert len(where) == len(p.initial) == min(B, V)
    for g, pairs in enumerate(p.starts):
        for s, v in pairs:
            assert v not in where
            where[v] = (g, s)
    assert sorted(where) == list(range(V))
    for v, (g, s) in where.items():
        assert s == p.slot_of[v] and (p.first_step[v] == 0 if g == "initial" else g == p.first_step[v] - 1)
    assert sorted(s for s, _ in p.initial) == list(range(min(B, V)))
    # a slot is never idle between two of its videos: its busy steps are 0 .. k - 1
    for b in range(B):
        busy = table[:, b, 0] >= 0
        assert not busy.any() or busy[:int(busy.sum())].all()
    # the reference simulation: G and the assignment, ties included
    Gs, slot_s, first_s = _simulate(lengths, B, order)
    assert (G, p.slot_of.tolist(), p.first_step.tolist()) == (Gs, slot_s, first_s)
    assert p.efficiency == (sum(lengths) - V) / (G * B) and 0 < p.efficiency <= 1
    # "longest" against the padded lock-step grouping of the same videos in the same order
    padded = sum(max(lengths[i:i + B]) - 1 for i in range(0, V, B))
    assert dataset.plan(lengths, B, "longest").G <= padded


def test_ties_go_to_the_lowest_slot():
    p = dataset.plan([4, 4, 4, 2, 2, 2], 3, "given")                   # all three slots fall free at step 3
    assert p.slot_of.tolist() == [0, 1, 2, 0, 1, 2] and p.first_step.tolist() == [0, 0, 0, 3, 3, 3] and p.G == 4
    assert p.starts[2] == [(0, 3), (1, 4), (2, 5)]


def test_hand_checked_case():
    p = dataset.plan((5, 3, 4, 2, 3), 2, "given")
    # slot 0: video 0 on steps 0..3, video 3 on step 4, video 4 on steps 5..6; slot 1: video 1 on 0..1, video 2 on 2..4
    want = [[(0, 1), (1, 1)], [(0, 2), (1, 2)], [(0, 3), (2, 1)], [(0, 4), (2, 2)], [(3, 1), (2, 3)], [(4, 1), (-1, -1)], [(4, 2), (-1, -1)]]
    assert p.G == 7 and p.table.tolist() == [[list(c) for c in row] for row in want]
    assert p.initial == [(0, 0), (1, 1)]
    assert p.starts == [[], [(1, 2)], [], [(0, 3)], [(0, 4)], [], []]
    assert p.slot_of.tolist() == [0, 1, 1, 0, 0] and p.first_step.tolist() == [0, 0, 2, 4, 5]
    assert p.efficiency == 12 / 14
    # taken as 5 (v0), 4 (v2), 3 (v1), 3 (v4), 2 (v3): slot 0 tracks 4 + 2 frames (v0, v4), slot 1 3 + 2 + 1 (v2, v1, v3)
    q = dataset.plan((5, 3, 4, 2, 3), 2, "longest")
    assert q.G == 6 and q.slot_of.tolist() == [0, 1, 1, 1, 0] and q.first_step.tolist() == [0, 3, 0, 5, 4]
    assert q.efficiency == 1.0


def test_refusals():
    for args in (([5, 1, 3], 2, "given"), ([5, 3], 0, "given"), ([5, 3], -1, "given"), ([5, 3], 2, "shortest"), ([], 2, "given"),
                 ([0], 1, "given")):
        with pytest.raises(ValueError):
            dataset.plan(*args)


def _fabricated(p, cap=6):
    """collect()-shaped rows of the whole plan: every value names its (step, slot), so a row in the wrong place shows"""
    G, B = p.G, p.B
    g, b = np.mgrid[0:G, 0:B]
    code = (g * 100 + b).astype(np.float64)
    live = p.table[:, :, 0] >= 0
    n = np.where(live, 1 + (g + b) % (cap + 2), 0).astype(np.int32)     # 0: not live; cap + 1: an overflow
    counts = np.zeros((G, B, cap), dtype=np.int32)
    for i in range(cap):
        counts[:, :, i] = g * 1000 + b * 10 + i
    sizes = np.stack([10 + p.table[:, :, 0], 20 + p.table[:, :, 0]], axis=2).astype(np.int32)
    return {"target_pos": np.stack([code, code + 0.5], axis=2), "target_sz": np.stack([code + 0.25, code + 0.75], axis=2),
            "score": code / 7, "best_id": (g * 100 + b).astype(np.int64),
            "rle": {"counts": counts, "n": n, "area": n * 3, "cap": cap, "sizes": sizes}}


def _cut(res, a, b):
    out = {k: v[a:b] for k, v in res.items() if k != "rle"}
    out["rle"] = {k: (v if k == "cap" else v[a:b]) for k, v in res["rle"].items()}
    return out


@pytest.mark.parametrize("bounds", [(), (1,), (3, 4), (2, 5, 6), tuple(range(1, 7))])
def test_gather_returns_the_rows_per_video_whatever_the_chunks(bounds):
    lengths = (5, 3, 4, 2, 3)
    p = dataset.plan(lengths, 2, "given")
    res = _fabricated(p)
    edges = (0,) + bounds + (p.G,)
    vids = dataset.gather(p, [_cut(res, a, b) for a, b in zip(edges[:-1], edges[1:])])
    assert len(vids) == 5
    overflow = 0
    for v, d in enumerate(vids):
        s, g0, n = int(p.slot_of[v]), int(p.first_step[v]), lengths[v] - 1
        assert (d["slot"], d["first_step"]) == (s, g0)
        steps = np.arange(g0, g0 + n)
        assert d["best_id"].tolist() == (steps * 100 + s).tolist() and d["score"].tolist() == ((steps * 100 + s) / 7).tolist()
        assert d["target_pos"].shape == (n, 2) and d["target_pos"][:, 1].tolist() == (steps * 100 + s + 0.5).tolist()
        assert d["target_sz"][:, 0].tolist() == (steps * 100 + s + 0.25).tolist()
        assert d["n"].tolist() == res["rle"]["n"][steps, s].tolist() and d["area"].tolist() == (res["rle"]["n"][steps, s] * 3).tolist()
        assert d["sizes"].tolist() == [[10 + v, 20 + v]] * n and len(d["rle"]) == n
        for t, g in enumerate(steps):
            if d["n"][t] > 6:
                overflow += 1
                assert d["rle"][t] is None
            else:
                assert d["rle"][t].dtype == np.int64 and d["rle"][t].tolist() == [g * 1000 + s * 10 + i for i in range(d["n"][t])]
    assert overflow >= 1
    with pytest.raises(ValueError):
        dataset.gather(p, [_cut(res, 0, p.G - 1)])
    with pytest.raises(ValueError):
        dataset.gather(p, [res, _cut(res, 0, 1)])


def test_ope_video_is_what_pack_ope_and_ope_lines_take():
    from siammask_amd import evaluate, tune
    d = {"target_pos": np.array([[50.0, 40.0], [52.0, 41.0]]), "target_sz": np.array([[20.0, 10.0], [22.0, 12.0]])}
    gt = np.array([[38.0, 34.0, 20.0, 10.0], [40.0, 35.0, 20.0, 10.0], [41.0, 35.0, 22.0, 12.0]])
    vid = dataset.ope_video(d, gt, "a")
    assert vid["rect"].shape == (1, 3, 4) and vid["rect"][0].tolist() == [gt[0].tolist(), [40.0, 35.0, 20.0, 10.0], [41.0, 35.0, 22.0, 12.0]]
    packed = evaluate.pack_ope([vid], device=None)
    assert packed["offsets"].tolist() == [0, 3] and packed["rect"].shape == (1, 3, 4)
    assert tune.ope_lines(vid["rect"][0])[1] == "40.0000,35.0000,20.0000,10.0000"
