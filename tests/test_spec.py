"""State-dict contract: the drop-in Custom exposes exactly the
reference's parameter/buffer names and shapes, and a checkpoint saved for the reference loads
through the reference's UNCHANGED utils/load_helper.load_pretrain."""
import json
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

from siammask_amd import spec, synth
from siammask_amd.custom import build

EXPECTED = {"sharp": (356, 21482052), "base": (324, 18816735), "rpn": (304, 16549982)}


@pytest.mark.parametrize("variant", spec.VARIANTS)
def test_entry_and_parameter_counts(variant):
    sd = build(variant).state_dict()
    n_entries, n_params = EXPECTED[variant]
    assert len(sd) == n_entries
    learnable = sum(v.numel() for k, v in sd.items()
                    if not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked")))
    assert learnable == n_params
    assert list(sd.keys()) == list(spec.state_dict_spec(variant).keys())


def test_synth_checkpoint_covers_spec_and_is_deterministic():
    a = synth.state_dict("sharp", "synthetic_damped")
    b = synth.state_dict("sharp", "synthetic_damped")
    assert list(a.keys()) == list(spec.state_dict_spec("sharp").keys())
    for k in a:
        assert a[k].shape == tuple(spec.state_dict_spec("sharp")[k][0])
        assert np.array_equal(a[k], b[k])
    # variants share tensors: base/rpn checkpoints are subsets of the sharp one
    base = synth.state_dict("base", "synthetic_damped")
    assert all(np.array_equal(base[k], a[k]) for k in base)


def _reference_custom(variant):
    from oracle.make_golden import import_reference_custom
    return import_reference_custom(variant)


@pytest.mark.parametrize("variant", spec.VARIANTS)
def test_names_and_shapes_equal_reference(variant):
    """against the reference's own Custom as recorded in tests/golden/reference_state_dict.json (oracle/make_spec_golden.py)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_state_dict.json")) as f:
        gold = json.load(f)
    ref = gold["variants"][variant]
    ours = build(variant)
    osd = ours.state_dict()
    assert [k for k, _, _ in ref["state_dict"]] == list(osd.keys())
    for k, shape, dtype in ref["state_dict"]:
        assert list(osd[k].shape) == shape, k
        assert str(osd[k].dtype) == "torch." + dtype, k
    assert ours.anchors == ref["anchors"] == gold["anchors_cfg"] and ours.anchor_num == ref["anchor_num"]


@pytest.mark.reference
def test_loads_through_unchanged_reference_load_pretrain():
    _reference_custom("sharp")
    from utils.load_helper import load_pretrain   # the reference's own loader
    sd = synth.torch_state_dict("sharp", "synthetic_damped")
    with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
        path = f.name
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}}, path)
    try:
        m = load_pretrain(build("sharp"), path)
    finally:
        os.unlink(path)
    got = m.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k].cpu(), v), k


def test_cpu_tensor_is_rejected_loudly():
    m = build("sharp")
    with pytest.raises(RuntimeError):
        m.template(torch.zeros(1, 3, 127, 127))
    with pytest.raises(RuntimeError):
        m.track_refine((1, 1))
