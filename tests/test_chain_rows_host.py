"""Row bands of the split Refine chain (csrc/chain_rows.h through smk_host_chain_rows: the function the kernel compiles).

A stream's chain runs on S workgroups; band s computes post2's rows [y0, y1) and, of post1 / h0.0 / h0.2, the rows the next
layer's range reads.  The demand is propagated here by brute force, row by row: post2 reads its input through the row table of
the nearest upsampling, (iy * 61) / 127 (refine_chain_body.inc build_up_tables), at the three taps iy = oy - 1 .. oy + 1 clipped to
the image; h0.2 and h0.0 read rows oy - 1 .. oy + 1 of a 61-row image."""
import ctypes

import numpy as np
import pytest

from siammask_amd import _lib

H_FINE, H_MID = 127, 61
LAYERS = ("post1", "h0.0", "h0.2", "post2")


def rows(S, s):
    out = (ctypes.c_int * 8)()
    _lib.check(_lib.lib().smk_host_chain_rows(S, s, out))
    return {name: (out[2 * i], out[2 * i + 1]) for i, name in enumerate(LAYERS)}


def demand(rng, H, SRC=0):
    """input rows (bool mask) a 3x3 pad-1 layer reads to produce the output rows rng of an H-row image; SRC > 0: the input has SRC
    rows and is read through the nearest upsampling to H"""
    hi = SRC or H
    need = np.zeros(hi, bool)
    for oy in range(*rng):
        for tap in (-1, 0, 1):
            iy = oy + tap
            if 0 <= iy < H:                               # outside: the zero border
                need[(iy * SRC) // H if SRC else iy] = True
    return need


def covers(rng, need):
    have = np.zeros(need.size, bool)
    have[rng[0]:rng[1]] = True
    return bool((have | ~need).all())


@pytest.mark.parametrize("S", [2, 4])
def test_post2_bands_tile_the_rows_once(S):
    count = np.zeros(H_FINE, int)
    for s in range(S):
        y0, y1 = rows(S, s)["post2"]
        assert 0 <= y0 < y1 <= H_FINE
        count[y0:y1] += 1
    assert (count == 1).all()


@pytest.mark.parametrize("S,s", [(S, s) for S in (2, 4) for s in range(S)])
def test_each_layer_computes_what_the_next_reads(S, s):
    r = rows(S, s)
    for name in LAYERS[:3]:
        assert 0 <= r[name][0] < r[name][1] <= H_MID, (name, r[name])
    assert covers(r["h0.2"], demand(r["post2"], H_FINE, H_MID)), r
    assert covers(r["h0.0"], demand(r["h0.2"], H_MID)), r
    assert covers(r["post1"], demand(r["h0.0"], H_MID)), r


def test_the_split_pays():
    """no band computes more than the issue's estimate of the fine layers' share (36 / 32 / 29 / 25 % at S = 4, + one row)"""
    for s in range(4):
        r = rows(4, s)
        assert r["post2"][1] - r["post2"][0] <= 32
        assert r["h0.2"][1] - r["h0.2"][0] <= 18 and r["h0.0"][1] - r["h0.0"][0] <= 20 and r["post1"][1] - r["post1"][0] <= 22


def test_one_band_is_the_whole_image():
    assert rows(1, 0) == {"post1": (0, H_MID), "h0.0": (0, H_MID), "h0.2": (0, H_MID), "post2": (0, H_FINE)}


@pytest.mark.parametrize("S,s", [(3, 0), (0, 0), (4, 4), (2, -1), (8, 0)])
def test_bad_band_is_refused(S, s):
    out = (ctypes.c_int * 8)()
    assert _lib.lib().smk_host_chain_rows(S, s, out) != 0


def test_tail_knobs_read_back():
    """smk_tune chain_split / mask_nsplit (no GPU): the rule is the default, a knob reads back what was set, other values are errors"""
    for key, good, bad in (("chain_split", (1, 2, 4), (3, 8, -1)), ("mask_nsplit", (1, 5, 15), (16, -1))):
        old = _lib.tune_get(key)
        try:
            for v in good:
                _lib.tune(**{key: v})
                assert _lib.tune_get(key) == v
            for v in bad:
                with pytest.raises(RuntimeError):
                    _lib.tune(**{key: v})
            assert _lib.tune_get(key) == good[-1]
        finally:
            _lib.tune(**{key: old})
    import subprocess
    import sys
    import os
    code = "from siammask_amd import _lib; print(_lib.tune_get('chain_split'), _lib.tune_get('mask_nsplit'))"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and r.stdout.split()[-2:] == ["0", "0"], r.stderr[-1000:]
