"""CPU-only checks of the fused-producer MSDA backward's host side: the opt-in switch, and the argument refusals of the two C
entry points, which happen before any HIP call."""
import ctypes

import pytest
import torch

from relation_detr_amd import _lib, ops, options


def test_msda_train_fused_switch():
    assert options.Options().msda_train_fused is False
    assert options.Options.from_env({}).msda_train_fused is False
    assert options.Options.from_env({"RDETR_MSDA_TRAIN_FUSED": "1"}).msda_train_fused is True
    assert options.Options.from_env({"RDETR_MSDA_TRAIN_FUSED": "0"}).msda_train_fused is False
    with pytest.raises(ValueError):
        options.Options.from_env({"RDETR_MSDA_TRAIN_FUSED": "on"})


@pytest.mark.parametrize("name", ["rdetr_msda_backward_fused_f32", "rdetr_msda_backward_fused_bf16"])
def test_fused_backward_argument_refusals(name):
    fn = getattr(_lib.load(), name)
    one = ctypes.c_void_p(16)                       # an aligned non-null dummy: never dereferenced on these paths
    ins = [one] * 6                                 # value, spatial_shapes, level_start_index, offsets, logits, reference_points
    outs = [one, one, one, None]                    # grad_value, grad_offsets, grad_logits, grad_ref_partial
    shape = [1, 10, 8, 32, 4, 5, 4]                 # B, S, H, D, L, Nq, P
    assert fn(*([None] * 6), 2, None, *shape, None, 0, None, None, None, None, None) == -1              # null pointers
    assert fn(*ins, 2, one, *shape, None, 0, one, None, one, None, None) == -1                          # null grad_offsets
    assert fn(*([None] * 6), 2, None, 0, 10, 8, 32, 4, 5, 4, None, 0, None, None, None, None, None) == 0   # empty batch
    assert fn(*([None] * 6), 2, None, 1, 10, 8, 32, 4, 0, 4, None, 0, None, None, None, None, None) == 0   # no queries
    assert fn(*ins, 2, one, 1, 10, 8, 32, 4, -1, 4, None, 0, *outs, None) == -1                         # negative size
    assert fn(*ins, 3, one, *shape, None, 0, *outs, None) == -1                                         # ref_dim
    assert fn(*ins, 2, one, 1, 10, 8, 64, 4, 5, 4, None, 0, *outs, None) == -2                          # head dim
    assert fn(*ins, 2, one, 1, 10, 8, 32, 9, 5, 4, None, 0, *outs, None) == -2                          # nine levels
    assert fn(*ins, 4, one, 1, 10, 8, 32, 4, 5, 2, None, 0, *outs, None) == -2                          # two points
    assert fn(*ins, 2, one, *shape, one, 16, *outs, None) == -1                                         # workspace too small
    assert fn(*ins, 2, one, *shape, one, -1, *outs, None) == -1                                         # negative workspace size


def test_fused_backward_op_refuses_cpu_tensors_and_other_shapes():
    v = torch.zeros(1, 10, 8, 32)
    off = torch.zeros(1, 5, 8, 1, 4, 2)
    lg = torch.zeros(1, 5, 8, 4)
    ref = torch.zeros(1, 5, 1, 2)
    shapes = torch.tensor([[2, 5]])
    start = torch.tensor([0])
    with pytest.raises(_lib.RdetrError):
        ops.ms_deform_attn_backward_fused(v, shapes, start, off, lg, ref, torch.zeros(1, 5, 256))
    assert hasattr(ops, "MultiScaleDeformableAttnFusedFunction")
