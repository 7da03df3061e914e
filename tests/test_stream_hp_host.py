"""Per-stream tracker hyper-parameters, the parts that need no device: the sweep's grid, directory names and pass plan
(siammask_amd/tune.py against tools/tune_vot.py:64-68,225-228, written out by hand), smk_host_trk_advance_hp against
smk_host_trk_advance called once per stream with that stream's lr in its cfg (byte for byte), and the null-context check of
smk_set_stream_hp."""
import ctypes

import numpy as np

import tracker_state_ref as R
from siammask_amd import _lib, tune
from siammask_amd.tracker import TrackerConfig
from test_tracker_state_host import _cfg, _ptr, _random_case


def test_grid_is_in_the_tools_nesting_order():
    got = tune.grid(penalty_k=[0.05, 0.1], window_influence=[0.3, 0.4], lr=[0.2, 0.6])
    want = [(0.05, 0.3, 0.2), (0.05, 0.3, 0.6), (0.05, 0.4, 0.2), (0.05, 0.4, 0.6),
            (0.1, 0.3, 0.2), (0.1, 0.3, 0.6), (0.1, 0.4, 0.2), (0.1, 0.4, 0.6)]
    assert got == [{"penalty_k": k, "window_influence": w, "lr": r} for k, w, r in want]


def test_result_dir_is_the_tools_directory_name():
    hp = {"penalty_k": 0.05, "window_influence": 0.1, "lr": 0.35}
    assert tune.result_dir("Custom_x", hp) == "Custom_x_r255_penalty_k_0_050_window_influence_0_100_lr_0_350"
    # '{:.3f}' rounds to three decimals; a '.' in the network's name is replaced as well (the replace covers the whole string)
    hp = {"penalty_k": 0.1234, "window_influence": 0.8, "lr": 1.0}
    assert tune.result_dir("Custom_v1.2", hp, instance_size=263) == "Custom_v1_2_r263_penalty_k_0_123_window_influence_0_800_lr_1_000"
    hp = {"penalty_k": 0.0, "window_influence": 0.45, "lr": 0.3}
    assert tune.result_dir("SiamMask_sharp", hp) == "SiamMask_sharp_r255_penalty_k_0_000_window_influence_0_450_lr_0_300"


def test_pass_plan_pads_the_last_pass_and_drops_the_padding():
    plan = tune.pass_plan(5, 4)
    assert plan == [([0, 1, 2, 3], 4), ([4, 4, 4, 4], 1)]
    assert len(plan) == 2 and sum(4 - keep for _, keep in plan) == 3          # 2 passes, 3 padded streams
    kept = [i for idx, keep in plan for i in idx[:keep]]
    assert kept == [0, 1, 2, 3, 4]                                             # every point once, no padded stream kept
    assert tune.pass_plan(8, 8) == [(list(range(8)), 8)] and tune.pass_plan(1, 3) == [([0, 0, 0], 1)]


def test_host_advance_hp_equals_the_advance_at_each_streams_lr():
    L = _lib.lib()
    B, im_w, im_h = 3, 320, 240
    lrs = [0.0, 0.38, 1.0]
    rng = np.random.default_rng(77)
    pos, sz, box = _random_case(rng, B, im_w, im_h)
    p = TrackerConfig({"lr": 0.77})                                            # cfg.lr is ignored by the _hp entry
    cfg = _cfg(p, 127)
    hp = np.zeros((B, 4))
    hp[:, 0], hp[:, 1], hp[:, 2] = 0.04, 0.4, lrs
    for slot, plan_next in ((0, 0), (1, 1)):
        blk = R.make_block(pos, sz, im_w, im_h)
        assert L.smk_host_trk_plan(_ptr(blk), B, ctypes.byref(cfg)) == 0
        start = blk.copy()
        rows = np.full((B, 16), np.nan)
        assert L.smk_host_trk_advance_hp(_ptr(blk), B, ctypes.byref(cfg), _ptr(hp), _ptr(box), slot, _ptr(rows), plan_next) == 0
        rec, twh = R.split_block(blk, B)
        seen = set()
        for b in range(B):
            one = start.copy()
            cfg_b = _cfg(TrackerConfig({"lr": lrs[b]}), 127)
            rows_b = np.full((B, 16), np.nan)
            assert L.smk_host_trk_advance(_ptr(one), B, ctypes.byref(cfg_b), _ptr(box), slot, _ptr(rows_b), plan_next) == 0
            rec_b, twh_b = R.split_block(one, B)
            assert rec[b].tobytes() == rec_b[b].tobytes() and len(rec[b].tobytes()) == 224, b
            assert rows[b].tobytes() == rows_b[b].tobytes(), b
            assert twh[b].tobytes() == twh_b[b].tobytes(), b
            seen.add(rec_b["target_sz"].tobytes())
        assert len(seen) == B                                                  # the three lr really give three states
    E = -1
    assert L.smk_host_trk_advance_hp(_ptr(blk), B, ctypes.byref(cfg), None, _ptr(box), 0, None, 0) == E
    assert L.smk_host_trk_advance_hp(_ptr(blk), B, ctypes.byref(cfg), _ptr(hp), _ptr(box), 2, None, 0) == E
    assert L.smk_trk_advance_hp(_ptr(blk), B, ctypes.byref(cfg), None, _ptr(box), 0, None, 0, None) == E      # before any device use
    assert L.smk_trk_advance_hp(None, B, ctypes.byref(cfg), _ptr(hp), _ptr(box), 0, None, 0, None) == E


def test_set_stream_hp_refuses_a_null_context():
    L = _lib.lib()
    hp = np.zeros((2, 4))
    assert L.smk_set_stream_hp(None, _ptr(hp)) == -1 and L.smk_set_stream_hp(None, None) == -1
    assert L.smk_last_error()
    assert _lib.HP_STRIDE == 4 and "smk_set_stream_hp" in _lib.SYMBOLS and "smk_trk_advance_hp" in _lib.SYMBOLS
