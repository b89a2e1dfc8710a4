"""CPU-only checks of the head-major MSDA training route's host side: the two C entry points are declared, bound and exported, the
ABI version is unchanged, their argument refusals happen before any HIP call, the opt-in switch, and the differentiable split of
the merged query projection (pure torch)."""
import ctypes
import os
import re

import pytest
import torch

from relation_detr_amd import _lib, msda_train_hm, options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rdetr_msda_backward_fused_hm_bf16", "rdetr_grad_value_from_head_major_bf16")


@pytest.mark.parametrize("name", NEW)
def test_symbol_is_declared_bound_and_exported(name):
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert re.search(r"\bint " + name + r"\s*\(", header)
    assert name in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert callable(getattr(_lib.load(), name))


def test_abi_version_is_unchanged():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert "#define RDETR_ABI_VERSION 3" in header
    assert _lib.load().rdetr_abi_version() == 3


def _bwd(*, ins=None, ld=(0, 0), ref_dim=2, go="one", shape=(1, 10, 8, 32, 4, 5, 4), ws=(None, 0), gv="one", goff="one", glg="one",
         gld=(0, 0)):
    one = ctypes.c_void_p(16)                       # an aligned non-null dummy: never dereferenced on these paths
    pick = lambda x: one if x == "one" else x
    ins = [one] * 6 if ins is None else ins         # value, spatial_shapes, level_start_index, offsets, logits, reference_points
    fn = _lib.load().rdetr_msda_backward_fused_hm_bf16
    return fn(ins[0], ins[1], ins[2], ins[3], ld[0], ins[4], ld[1], ins[5], ref_dim, pick(go), *shape, ws[0], ws[1], pick(gv),
              pick(goff), gld[0], pick(glg), gld[1], None, None)


def test_backward_argument_refusals():
    one = ctypes.c_void_p(16)
    assert _bwd(ins=[None] * 6, go=None, gv=None, goff=None, glg=None) == -1                       # null pointers
    assert _bwd(goff=None) == -1                                                                   # null grad_offsets
    assert _bwd(ins=[None] * 6, go=None, gv=None, goff=None, glg=None, shape=(0, 10, 8, 32, 4, 5, 4)) == 0      # B = 0
    assert _bwd(ins=[None] * 6, go=None, gv=None, goff=None, glg=None, shape=(1, 10, 8, 32, 4, 0, 4)) == 0      # Nq = 0
    assert _bwd(shape=(1, 10, 8, 32, 4, -1, 4)) == -1                                              # negative size
    assert _bwd(ref_dim=3) == -1
    assert _bwd(shape=(1, 10, 8, 64, 4, 5, 4)) == -2                                               # D = 64
    assert _bwd(shape=(1, 10, 8, 32, 9, 5, 4)) == -2                                               # nine levels
    assert _bwd(shape=(1, 10, 8, 32, 4, 5, 2)) == -2                                               # two points
    assert _bwd(ld=(385, 0)) in (-1, -2)                                                           # odd ld_offsets
    assert _bwd(gld=(385, 0)) in (-1, -2)                                                          # odd ld_grad_offsets
    assert _bwd(ld=(254, 0)) == -1 and _bwd(ld=(0, 126)) == -1                                     # strides below the row length
    assert _bwd(gld=(254, 0)) == -1 and _bwd(gld=(0, 126)) == -1 and _bwd(ld=(-2, 0)) == -1
    assert _bwd(ws=(one, 16)) == -1 and _bwd(ws=(one, -1)) == -1                                   # short / negative workspace
    assert _bwd(ins=[ctypes.c_void_p(8)] + [one] * 5) == -2                                        # value misses its alignment


def test_relayout_argument_refusals():
    fn = _lib.load().rdetr_grad_value_from_head_major_bf16
    one = ctypes.c_void_p(16)
    assert fn(None, None, 1, 10, 8, 32, None, 256, None) == -1                                     # null pointers
    assert fn(None, None, 0, 10, 8, 32, None, 256, None) == 0 and fn(None, None, 1, 0, 8, 32, None, 256, None) == 0
    assert fn(one, None, 1, 10, 8, 64, one, 512, None) == -1                                       # other head sizes
    assert fn(one, None, 1, 10, 8, 32, one, 255, None) == -1 and fn(one, None, 1, 10, 8, 32, one, 260, None) == -1
    assert fn(one, None, 1, 10, 8, 32, ctypes.c_void_p(8), 256, None) == -1                        # dst misses 16 bytes
    assert fn(one, None, -1, 10, 8, 32, one, 256, None) == -1


def test_msda_train_head_major_switch():
    assert options.Options().msda_train_head_major is False
    assert options.Options.from_env({}).msda_train_head_major is False
    assert options.Options.from_env({"RDETR_MSDA_TRAIN_HEAD_MAJOR": "1"}).msda_train_head_major is True
    assert options.Options.from_env({"RDETR_MSDA_TRAIN_HEAD_MAJOR": "0"}).msda_train_head_major is False
    with pytest.raises(ValueError):
        options.Options.from_env({"RDETR_MSDA_TRAIN_HEAD_MAJOR": "yes"})


def test_shadow_tables_still_complete():
    import test_shadow_complete as t
    t.test_every_ops_function_is_classified()
    t.test_every_rdetr_symbol_is_under_the_tripwire_or_excluded()
    t.test_every_options_field_is_switched_in_the_ab_test_or_covered_elsewhere()


def test_no_cpu_path():
    with pytest.raises(_lib.RdetrError):
        msda_train_hm.grad_value_from_head_major(torch.zeros(1, 8, 10, 32))
    off, lg = torch.zeros(1, 10, 8, 1, 4, 2, dtype=torch.bfloat16), torch.zeros(1, 10, 8, 4, dtype=torch.bfloat16)
    with pytest.raises(_lib.RdetrError):
        msda_train_hm.ms_deform_attn_backward_fused_hm(torch.zeros(1, 8, 10, 32, dtype=torch.bfloat16), torch.tensor([[2, 5]]),
                                                       torch.tensor([0]), off, lg, torch.zeros(1, 10, 1, 2),
                                                       torch.zeros(1, 10, 256, dtype=torch.bfloat16))
    assert hasattr(msda_train_hm, "MultiScaleDeformableAttnHeadMajorFunction")


class _WritesMergedGrad(torch.autograd.Function):
    """Stands in for the MSDA core: its backward writes the two gradients into the column slices of one buffer."""
    buffers = []

    @staticmethod
    def forward(ctx, o, l):
        ctx.dims = (o.shape, l.shape)
        return o.flatten(2).sum(2) * 2 + l.flatten(2).sum(2) * 3

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (so, sl), (B, N) = ctx.dims, g.shape
        n_off, n_lg = so[2:].numel(), sl[2:].numel()
        buf = torch.empty(B, N, n_off + n_lg)
        go, gl = buf[..., :n_off].view(so), buf[..., n_off:].view(sl)
        go.copy_(g.view(B, N, *[1] * (len(so) - 2)).expand(so) * 2)
        gl.copy_(g.view(B, N, *[1] * (len(sl) - 2)).expand(sl) * 3)
        _WritesMergedGrad.buffers.append(buf)
        return go, gl


def test_split_merged_projection_hands_the_merged_gradient_on():
    B, N, n_off, W = 2, 5, 8, 12
    g = torch.randn(B, N)
    want = torch.cat([g[..., None].expand(B, N, n_off) * 2, g[..., None].expand(B, N, W - n_off) * 3], -1)
    seen = []
    both = torch.randn(B, N, W, requires_grad=True)
    stage = both * 1.0
    stage.register_hook(lambda t: seen.append(t))
    o, l = msda_train_hm.split_merged_projection(stage, n_off)
    assert torch.equal(o, stage[..., :n_off]) and torch.equal(l, stage[..., n_off:])
    _WritesMergedGrad.apply(o.view(B, N, 2, 2, 2), l.view(B, N, 2, 2)).backward(g)
    assert torch.equal(both.grad, want)
    assert seen[0].data_ptr() == _WritesMergedGrad.buffers[-1].data_ptr()       # the buffer itself, not a re-assembled copy
    # ordinary consumers, and one slice unused: concatenated / zero-filled
    both = torch.randn(B, N, W, requires_grad=True)
    o, l = msda_train_hm.split_merged_projection(both, n_off)
    (o.sum() * 2 + l.sum() * 3).backward()
    assert torch.equal(both.grad, torch.cat([torch.full((B, N, n_off), 2.0), torch.full((B, N, W - n_off), 3.0)], -1))
    both = torch.randn(B, N, W, requires_grad=True)
    o, l = msda_train_hm.split_merged_projection(both, n_off)
    (o.sum() * 2).backward()
    assert torch.equal(both.grad, torch.cat([torch.full((B, N, n_off), 2.0), torch.zeros(B, N, W - n_off)], -1))


def test_package_exports_the_route():
    import relation_detr_amd
    for name in ("MultiScaleDeformableAttnHeadMajorFunction", "ms_deform_attn_backward_fused_hm", "grad_value_from_head_major"):
        assert getattr(relation_detr_amd, name) is getattr(msda_train_hm, name) and name in relation_detr_amd.__all__
