"""The host half of DeviceTracker.collect() (tracker.collect_host) on hand-made float64 rows: which column every key of the
result comes from, the polygon fallback and its error, the VOS counts, and what the start events do to tr.state.  Pure numpy."""
import numpy as np
import pytest
import torch

from siammask_amd import preproc, tracker
from siammask_amd.tracker import RESULT_ROW, START_ROW, collect_host

T, B = 3, 2


def _rows(extra=0):
    """[T,B,16 + extra] with a distinct value in every cell: 1000 t + 100 b + column (+ .25 where a float is kept as it is)"""
    t, b, c = np.meshgrid(np.arange(T), np.arange(B), np.arange(RESULT_ROW + extra), indexing="ij")
    rows = (1000.0 * t + 100.0 * b + c).astype(np.float64)
    rows[:, :, [0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13]] += 0.25
    return rows


def _state():
    return {"im_h": 240, "im_w": 320, "avg_chans": [np.full(3, 10.0 + b) for b in range(B)], "target_pos": np.zeros((B, 2)),
            "target_sz": np.ones((B, 2)), "score": np.zeros(B), "mask": "the mask before", "polygon": "stale", "polygon_found": "stale"}


def _corners(pos, sz):
    x, y, w, h = pos[0] - sz[0] / 2, pos[1] - sz[1] / 2, sz[0], sz[1]
    return np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]])


def test_every_key_comes_from_its_column():
    rows, state = _rows(), _state()
    before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    res, st = collect_host(rows, T, B, [False] * T, None, [], None, state)
    assert set(res) == {"target_pos", "target_sz", "score", "best_id", "delta_yx", "crop_box", "mask"} and res["mask"] is None
    assert np.array_equal(res["target_pos"], rows[:, :, 0:2]) and np.array_equal(res["target_sz"], rows[:, :, 2:4])
    assert np.array_equal(res["score"], rows[:, :, 4]) and res["score"].dtype == np.float64
    assert res["best_id"].dtype == np.int64 and np.array_equal(res["best_id"], rows[:, :, 5].astype(np.int64))
    assert res["delta_yx"].dtype == np.int64 and np.array_equal(res["delta_yx"], rows[:, :, 6:8].astype(np.int64))
    assert res["delta_yx"][2, 1].tolist() == [2106, 2107] and res["best_id"][1, 0] == 1005
    assert np.array_equal(res["crop_box"], rows[:, :, [12, 13, 14, 14]]) and res["crop_box"].shape == (T, B, 4)
    # the state: the last frame's rows; the polygon of an earlier step goes; nothing that was given is modified
    for k in ("target_pos", "target_sz", "score", "best_id", "delta_yx"):
        assert np.array_equal(st[k], res[k][-1]) and not np.shares_memory(st[k], res[k])
    assert st["crop_box"] == [[2012.25, 2013.25, 2014, 2014], [2112.25, 2113.25, 2114, 2114]]
    assert all(type(v[2]) is int and type(v[0]) is float for v in st["crop_box"])
    assert "polygon" not in st and "polygon_found" not in st and st["x_crop"] is None
    assert (st["im_h"], st["im_w"], st["mask"]) == (240, 320, "the mask before") and st["avg_chans"] is state["avg_chans"]
    assert set(state) == set(before) and all(np.array_equal(state[k], before[k]) for k in ("target_pos", "target_sz", "score"))


def test_polygon_rows_of_a_mixed_chunk(monkeypatch):
    asked = [True, False, True]
    rows = _rows(12)
    q = rows[:, :, RESULT_ROW:]
    q[:, :, 9] = 1.0                                                    # found
    q[0, 1, 9] = 0.0                                                    # an empty mask on an asked frame
    q[1, :, 9] = -1.0                                                   # a frame that did not ask: its rows mean nothing
    res, st = collect_host(rows, T, B, asked, None, [], None, _state())
    assert res["polygon"].shape == (T, B, 4, 2) and res["polygon"].dtype == np.float64
    assert res["polygon_found"].tolist() == [[True, False], [False, False], [True, True]]
    assert np.array_equal(res["polygon"][0, 0], q[0, 0, :8].reshape(4, 2)) and np.array_equal(res["polygon"][2], q[2, :, :8].reshape(B, 4, 2))
    want = _corners(rows[0, 1, 8:10], rows[0, 1, 10:12])                # the state BEFORE the clip: columns 8:12
    assert np.array_equal(res["polygon"][0, 1], want) and not np.array_equal(want, _corners(rows[0, 1, 0:2], rows[0, 1, 2:4]))
    # exactly the corners rotated_boxes() builds for an empty mask (its device rows replaced by rows that found nothing)
    monkeypatch.setattr(preproc, "mask_rboxes", lambda masks, min_area=100.0: torch.zeros((B, 12), dtype=torch.float64))
    poly, found = tracker.rotated_boxes(None, rows[0, :, 8:10], rows[0, :, 10:12])
    assert not found.any() and np.array_equal(poly[1], res["polygon"][0, 1])
    assert np.array_equal(st["polygon"], res["polygon"][2]) and st["polygon_found"].tolist() == [True, True]
    # the last frame did not ask: the state has no polygon
    _, st = collect_host(rows, T, B, [True, False, False], None, [], None, _state())
    assert "polygon" not in st and "polygon_found" not in st
    # a loop bound exceeded on an asked frame is an error
    q[2, 0, 9] = -1.0
    with pytest.raises(RuntimeError):
        collect_host(rows, T, B, asked, None, [], None, _state())
    collect_host(rows, T, B, [True, False, False], None, [], None, _state())


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("poly", [False, True])
def test_vos_counts_come_from_the_tail(K, poly):
    rows = _rows((12 if poly else 0) + 2 * K)
    if poly:
        rows[:, :, RESULT_ROW + 9] = 1.0
    counts = np.arange(T * B * K * 2).reshape(T, B, K * 2) * 7 + 3
    rows[:, :, -2 * K:] = counts                                        # int32 counts as float64
    res, _ = collect_host(rows, T, B, [poly] * T, K, [], None, _state())
    assert res["vos_counts"].dtype == np.int64 and res["vos_counts"].shape == (T, B, K, 2)
    assert np.array_equal(res["vos_counts"], counts.reshape(T, B, K, 2))
    assert ("polygon" in res) == poly and np.array_equal(res["crop_box"][:, :, 3], rows[:, :, 14])
    if poly:
        assert np.array_equal(res["polygon"], rows[:, :, RESULT_ROW:RESULT_ROW + 8].reshape(T, B, 4, 2))


def _ev_rows(n):
    ev = np.zeros((n, B, START_ROW))
    for e in range(n):
        for b in range(B):
            ev[e, b] = [1.0] + [50.5 + 10 * e + b + c for c in range(7)]       # started, mean colour (3), target_pos, target_sz
    return ev


def test_start_events_and_the_state():
    rows = _rows()
    # a start behind the last frame: the state takes its position and size; nothing follows it in the chunk
    ev = _ev_rows(1)
    res, st = collect_host(rows, T, B, [False] * T, None, [(T, [1])], ev, _state())
    e = res["events"][0]
    assert (e["t"], e["streams"], e["started"].tolist()) == (T, [1], [True])
    assert np.array_equal(e["avg_chans"], ev[0, 1:2, 1:4]) and np.array_equal(e["target_pos"], ev[0, 1:2, 4:6])
    assert np.array_equal(e["target_sz"], ev[0, 1:2, 6:8])
    assert np.array_equal(st["target_pos"][1], ev[0, 1, 4:6]) and np.array_equal(st["target_sz"][1], ev[0, 1, 6:8])
    assert np.array_equal(st["target_pos"][0], rows[-1, 0, 0:2]) and np.array_equal(st["target_sz"][0], rows[-1, 0, 2:4])
    assert np.array_equal(st["avg_chans"][1], ev[0, 1, 1:4]) and np.array_equal(st["avg_chans"][0], np.full(3, 10.0))
    assert np.array_equal(res["target_pos"][-1], rows[-1, :, 0:2])      # the result rows are the frames', not the event's
    # a start with frames behind it: the frames' rows are the state; the mean colour is still taken
    state = _state()
    res, st = collect_host(rows, T, B, [False] * T, None, [(1, [0, 1])], ev, state)
    assert np.array_equal(st["target_pos"], rows[-1, :, 0:2]) and np.array_equal(st["target_sz"], rows[-1, :, 2:4])
    assert np.array_equal(np.stack(st["avg_chans"]), ev[0, :, 1:4]) and res["events"][0]["started"].tolist() == [True, True]
    assert np.array_equal(np.stack(state["avg_chans"]), [[10.0] * 3, [11.0] * 3])       # (the list given is not modified)
    # started == 0 (the object was absent from the labels): nothing changes, the event says so
    ev0 = _ev_rows(1)
    ev0[0, 1, 0] = 0.0
    res, st = collect_host(rows, T, B, [False] * T, None, [(T, [0, 1])], ev0, _state())
    assert res["events"][0]["started"].tolist() == [True, False]
    assert np.array_equal(st["target_pos"][1], rows[-1, 1, 0:2]) and np.array_equal(st["avg_chans"][1], np.full(3, 11.0))
    assert np.array_equal(st["target_pos"][0], ev0[0, 0, 4:6]) and np.array_equal(st["avg_chans"][0], ev0[0, 0, 1:4])


def test_events_only():
    ev, state = _ev_rows(2), _state()
    ev[1, 0, 0] = 0.0
    res, st = collect_host(np.zeros((0, B, RESULT_ROW)), 0, B, [], None, [(0, [1]), (0, [0])], ev, state)
    assert list(res) == ["events"] and [e["t"] for e in res["events"]] == [0, 0]
    assert [e["started"].tolist() for e in res["events"]] == [[True], [False]]
    assert np.array_equal(st["target_pos"], [[0.0, 0.0], ev[0, 1, 4:6]]) and np.array_equal(st["target_sz"], [[1.0, 1.0], ev[0, 1, 6:8]])
    assert np.array_equal(st["avg_chans"][1], ev[0, 1, 1:4]) and np.array_equal(st["avg_chans"][0], np.full(3, 10.0))
    assert not state["target_pos"].any() and st["polygon"] == "stale" and st["mask"] == "the mask before"
    assert set(st) == set(state)                                        # no frame: no key comes or goes
