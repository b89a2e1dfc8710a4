"""Host side of the optimizer step (relation_detr_amd/optim.py): the torch route against torch.optim.AdamW + clip_grad_norm_ bit for
bit, the state-dict round trip, the chunk-map builder, the parameter groups, the refusals, the ABI and train_step on the CPU.
Needs no GPU."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import relation_detr_amd
from relation_detr_amd import _lib, optim, options
from relation_detr_amd.optim import CHUNK, FusedAdamW, build_chunk_map, relation_param_groups, train_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rdetr_grad_sqnorm_f32", "rdetr_grad_clip_coef", "rdetr_adamw_step_f32")
SIZES = (1, 3, 4, 5, 91, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)


def make_params(seed=0):
    """Seven parameters for three groups; [5] is frozen, [2] has no gradient on odd steps."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(7, 5), (91,), (4, 3), (13,), (2, 3, 4), (6,), (33,)]
    params = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]
    params[5].requires_grad_(False)
    return params


def groups_of(params):
    return [{"params": params[:3]}, {"params": params[3:5], "weight_decay": 0.0}, {"params": params[5:], "lr": 3e-4}]


def set_grads(params, step, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + step)
    for i, p in enumerate(params):
        if not p.requires_grad or (i == 2 and step % 2 == 1):
            p.grad = None
        else:
            p.grad = torch.randn(p.shape, generator=g) * (10.0 if step % 2 == 0 else 1e-3)      # clipped on even steps only


def run(opt, params, steps, first=0, scheduler=None, max_norm=0.1):
    norms = []
    for s in range(first, first + steps):
        set_grads(params, s)
        if isinstance(opt, FusedAdamW):
            norms.append(opt.clip_grad_norm_(max_norm))
        else:
            norms.append(torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], max_norm))
        opt.step()
        if scheduler is not None:
            scheduler.step()
    return norms


def assert_same_run(a, b, pa, pb, na, nb):
    for x, y in zip(na, nb):
        assert torch.equal(x, y)
    for i, (p, q) in enumerate(zip(pa, pb)):
        assert torch.equal(p, q), i
        sa, sb = a.state.get(p, {}), b.state.get(q, {})
        assert set(sa) == set(sb), i
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (i, k)
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), i                              # the torch route scales the gradient in place


def test_torch_route_is_torch_adamw_with_clip_bit_for_bit():
    pa, pb = make_params(), make_params()
    a = FusedAdamW(groups_of(pa), lr=1e-3, weight_decay=1e-2, fused=False)
    b = torch.optim.AdamW(groups_of(pb), lr=1e-3, weight_decay=1e-2)
    sa = torch.optim.lr_scheduler.LinearLR(a, start_factor=0.1, total_iters=4)
    sb = torch.optim.lr_scheduler.LinearLR(b, start_factor=0.1, total_iters=4)
    frozen, idle = pa[5].detach().clone(), pa[2].detach().clone()
    na, nb = run(a, pa, 5, scheduler=sa), run(b, pb, 5, scheduler=sb)
    assert_same_run(a, b, pa, pb, na, nb)
    assert [g["lr"] for g in a.param_groups] == [g["lr"] for g in b.param_groups]
    assert any(n > 0.1 for n in na) and any(n < 0.1 for n in na)                # both a clipped and an unclipped step
    assert torch.equal(pa[5], frozen) and pa[5] not in a.state and not torch.equal(pa[2], idle)
    assert a.state[pa[2]]["step"].item() == 3 and a.state[pa[0]]["step"].item() == 5      # step counts only gradients seen
    for ga, gb in zip(a.param_groups, b.param_groups):
        assert set(ga) == set(gb) and all(ga[k] == gb[k] for k in ga if k != "params")
    # the default route on CPU parameters is the torch route as well, as in RelationCriterion
    pc = make_params()
    c = FusedAdamW(groups_of(pc), lr=1e-3, weight_decay=1e-2)
    nc = run(c, pc, 5, scheduler=torch.optim.lr_scheduler.LinearLR(c, start_factor=0.1, total_iters=4))
    assert_same_run(c, b, pc, pb, nc, nb)


def test_state_dict_round_trip_in_the_middle_of_a_run():
    pr, p1, p2, p3 = make_params(), make_params(), make_params(), make_params()
    make = lambda cls, params, **kw: cls(groups_of(params), lr=1e-3, weight_decay=1e-2, **kw)
    ref = make(torch.optim.AdamW, pr)
    nr = run(ref, pr, 2) + run(ref, pr, 2, first=2) + run(ref, pr, 2, first=4)

    first = make(torch.optim.AdamW, p1)
    n = run(first, p1, 2)
    second = make(FusedAdamW, p2, fused=False)                                  # torch -> FusedAdamW
    with torch.no_grad():
        for q, p in zip(p2, p1):
            q.copy_(p)
    second.load_state_dict(first.state_dict())
    n += run(second, p2, 2, first=2)
    third = make(torch.optim.AdamW, p3)                                         # FusedAdamW -> torch
    with torch.no_grad():
        for q, p in zip(p3, p2):
            q.copy_(p)
    third.load_state_dict(second.state_dict())
    n += run(third, p3, 2, first=4)
    assert_same_run(third, ref, p3, pr, n, nr)
    a, b = second.state_dict(), make(torch.optim.AdamW, make_params()).state_dict()
    assert [set(g) for g in a["param_groups"]] == [set(g) for g in b["param_groups"]]


def test_multistep_lr_drives_it():
    params = make_params()
    opt = FusedAdamW(groups_of(params), lr=1e-3, fused=False)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.1)
    run(opt, params, 3, scheduler=sched)
    assert [g["lr"] for g in opt.param_groups] == pytest.approx([1e-4, 1e-4, 3e-5])


@pytest.mark.parametrize("chunk", [CHUNK, 4, 8])
def test_chunk_map_covers_every_element_once(chunk):
    numels = [0] + list(SIZES) + [0, 7, 0]
    cmap = build_chunk_map(numels, chunk)
    assert cmap.dtype == optim.CHUNK_DT and cmap.dtype.itemsize == 16
    covered = [np.zeros(n, dtype=np.int32) for n in numels]
    for first, tensor, _ in cmap.tolist():
        n = numels[tensor]
        assert 0 <= first < n and first % chunk == 0                            # starts inside its tensor, on a chunk boundary
        covered[tensor][first:min(first + chunk, n)] += 1                       # and ends inside it: the kernel clamps to numel
    for n, c in zip(numels, covered):
        assert (c == 1).all(), n
    assert len(cmap) == sum(-(-n // chunk) for n in numels)
    assert 0 not in {numels[t] for t in cmap["tensor"]}                          # zero-numel tensors have no chunk
    assert (np.diff(cmap["tensor"]) >= 0).all()                                  # tensors in order
    assert len(build_chunk_map([], chunk)) == 0 and len(build_chunk_map([0, 0], chunk)) == 0
    with pytest.raises(ValueError):
        build_chunk_map([4], 6)
    with pytest.raises(ValueError):
        build_chunk_map([-1], chunk)


def test_table_layouts_match_the_header():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    for dt, struct in ((optim.TENSOR_DT, "rdetr_optim_tensor"), (optim.STEP_DT, "rdetr_optim_step"), (optim.CHUNK_DT, "rdetr_optim_chunk")):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, re.S).group(1)
        assert re.findall(r"([a-z_0-9]+)\s*[,;]", body) == list(dt.names), struct
    assert (optim.TENSOR_DT.itemsize, optim.STEP_DT.itemsize) == (40, 40)
    want = optim.step_scalars(1e-4, 0.9, 0.999, 1e-8, 1e-4, 3.0)
    assert want == (1 - 1e-4 * 1e-4, 1 - 0.9, 0.999, 1 - 0.999, 1e-4 / (1 - 0.9 ** 3.0), (1 - 0.999 ** 3.0) ** 0.5, 1e-8)


class Named(torch.nn.Module):
    def __init__(self, names):
        super().__init__()
        self.names = list(names)
        self.values = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(2)) for _ in self.names])

    def named_parameters(self, *args, **kwargs):
        return iter(zip(self.names, self.values))


def test_param_groups_on_hand_written_names():
    lr, wd = 1e-4, 1e-2
    cases = [("transformer.encoder.layers.0.self_attn.sampling_offsets.weight", 0.1, wd),
             ("transformer.encoder.layers.0.self_attn.sampling_offsets.bias", 0.1, 0),
             ("transformer.decoder.layers.1.norm1.weight", 1, 0),
             ("transformer.decoder.layers.1.linear1.bias", 1, 0),
             ("transformer.decoder.layers.1.linear1.weight", 1, wd),
             ("backbone.body.layer2.0.conv1.weight", 0.1, wd),
             ("backbone.body.layer2.0.bn.bias", 0.1, 0),
             ("transformer.decoder.reference_points.weight", 0.1, wd),
             ("transformer.tgt_embed.weight", 1, wd)]
    model = Named(n for n, _, _ in cases)
    model.values[8].requires_grad_(False)                                       # frozen: in no group
    groups = relation_param_groups(model, lr)
    opt = FusedAdamW(groups, lr=lr, weight_decay=wd, fused=False)
    found = {}
    for g in opt.param_groups:
        for p in g["params"]:
            assert id(p) not in found
            found[id(p)] = (g["lr"], g["weight_decay"])
    for (name, factor, decay), p in zip(cases[:8], model.values):
        assert found[id(p)] == (pytest.approx(lr * factor), decay), name
    assert id(model.values[8]) not in found
    # the reference's order: rest, backbone, backbone norm/bias, projections, their biases, other norm/bias; empty groups dropped
    first = [[n for n, p in zip(model.names, model.values) if p is g["params"][0]][0] for g in groups]
    assert first == [cases[4][0], cases[5][0], cases[6][0], cases[0][0], cases[1][0], cases[2][0]]
    assert len(relation_param_groups(Named(["a.weight", "a.bias"]), lr)) == 2


def test_param_groups_on_the_real_head():
    from test_denoising_host import tiny_head
    head = tiny_head("cpu", False)
    groups = relation_param_groups(head, 1e-4)
    ids = [id(p) for g in groups for p in g["params"]]
    trainable = [id(p) for p in head.parameters() if p.requires_grad]
    assert len(ids) == len(set(ids)) and set(ids) == set(trainable)
    assert all(g["params"] for g in groups) and 3 <= len(groups) <= 6
    by_name = dict(head.named_parameters())
    offsets = by_name["transformer.encoder.layers.0.self_attn.sampling_offsets.weight"]
    (g,) = [g for g in groups if any(p is offsets for p in g["params"])]
    assert g == {"params": g["params"], "lr": pytest.approx(1e-5)}


def test_refusals():
    p = lambda *a, **k: torch.nn.Parameter(torch.zeros(*a, **k))
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=flag):
            FusedAdamW([p(3)], **{flag: True})
        with pytest.raises(ValueError, match=flag):
            FusedAdamW([p(3)], fused=False, **{flag: True})
    with pytest.raises(ValueError, match="tensor lr"):
        FusedAdamW([p(3)], lr=torch.tensor(1e-3))
    opt = FusedAdamW([p(3)], fused=False)
    opt.param_groups[0]["lr"] = torch.tensor(1e-3)                              # or set later, by a scheduler or by hand
    opt.param_groups[0]["params"][0].grad = torch.ones(3)
    with pytest.raises(ValueError, match="tensor lr"):
        opt.step()
    opt.param_groups[0]["lr"] = 1e-3
    opt.param_groups[0]["amsgrad"] = True                                       # as a loaded state dict could
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()

    for fused in (True, False):
        emb = p(4, 3)
        emb.grad = torch.sparse_coo_tensor(torch.tensor([[1], [2]]), torch.tensor([1.0]), (4, 3))
        opt = FusedAdamW([emb], fused=fused)
        with pytest.raises(ValueError, match="sparse"):
            opt.clip_grad_norm_(0.1)
        with pytest.raises(ValueError, match="sparse"):
            opt.step()

    # the fused route: any parameter off the CPU selects it, and then every parameter has to be fp32, dense, contiguous, on one GPU
    meta = lambda *a, **k: torch.nn.Parameter(torch.empty(*a, device="meta", **k))
    with pytest.raises(ValueError, match="not on a GPU"):
        FusedAdamW([meta(4)])
    with pytest.raises(ValueError, match="not on a GPU"):
        FusedAdamW([meta(4), p(4)])                                             # a CPU parameter among them
    with pytest.raises(ValueError, match="fp32"):
        FusedAdamW([meta(4, dtype=torch.bfloat16)])
    with pytest.raises(ValueError, match="fp32"):
        FusedAdamW([meta(4, dtype=torch.float64)])
    with pytest.raises(ValueError, match="not contiguous"):
        FusedAdamW([torch.nn.Parameter(torch.empty(4, 6, device="meta").t())])
    opt = FusedAdamW([p(4)])
    assert not opt._on_fused_route()
    with pytest.raises(ValueError, match="not on a GPU"):
        opt.add_param_group({"params": [meta(4)]})
    assert "dense" in optim.fused_refusal(torch.zeros(3, 3).to_sparse())
    assert optim.fused_refusal(torch.zeros(3)) == "on cpu, not on a GPU" and "fp32" in optim.fused_refusal(torch.zeros(3, dtype=torch.half))
    FusedAdamW([meta(4)], fused=False)                                          # the torch route takes any device and dtype
    FusedAdamW([p(4, dtype=torch.bfloat16)])                                    # and CPU parameters always take it


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_once_bound_and_exported(name):
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert len(re.findall(r"^int " + name + r"\s*\(", header, re.M)) == 1
    assert name in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert callable(getattr(_lib.load(), name))


def test_abi_exports_and_options_are_unchanged():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert set(re.findall(r"\b(rdetr_[a-z0-9_]+)\s*\(", header)) == set(_lib.SIGNATURES)
    assert len(re.findall(r"^long long rdetr_optim_workspace_bytes\s*\(", header, re.M)) == 1
    assert "#define RDETR_ABI_VERSION 3" in header and _lib.load().rdetr_abi_version() == 3
    assert len(dataclasses.fields(options.Options)) == 25                       # `fused` is a constructor argument, not a routing switch
    for name in ("FusedAdamW", "relation_param_groups", "train_step"):
        assert name in relation_detr_amd.__all__ and getattr(relation_detr_amd, name) is getattr(optim, name)
    assert CHUNK > 0 and CHUNK % 4 == 0
    import test_shadow_complete as t
    t.test_every_ops_function_is_classified()
    t.test_every_rdetr_symbol_is_under_the_tripwire_or_excluded()
    t.test_every_training_module_function_is_classified()


def test_argument_refusals_without_gpu():
    lib = _lib.load()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(4)
    assert lib.rdetr_optim_workspace_bytes(0) == 0 and lib.rdetr_optim_workspace_bytes(-3) == 0
    assert lib.rdetr_optim_workspace_bytes(5) == 28

    def table(fn, tensors=one, steps=one, cmap=one, n_tensors=2, n_chunks=3, chunk=CHUNK, cap=0):
        if fn is lib.rdetr_grad_sqnorm_f32:
            return fn(tensors, steps, cmap, n_tensors, n_chunks, chunk, cap, one, 20, None)
        return fn(tensors, steps, cmap, n_tensors, n_chunks, chunk, cap, None, None)
    for fn in (lib.rdetr_grad_sqnorm_f32, lib.rdetr_adamw_step_f32):
        assert table(fn, n_chunks=0, tensors=None, steps=None, cmap=None, n_tensors=0) == 0        # zero work: no launch
        assert table(fn, tensors=None) == -1 and table(fn, steps=None) == -1 and table(fn, cmap=None) == -1
        assert table(fn, n_tensors=-1) == -1 and table(fn, n_tensors=0) == -1 and table(fn, n_chunks=-1) == -1 and table(fn, chunk=0) == -1
        assert table(fn, chunk=6) == -2 and table(fn, tensors=odd) == -2 and table(fn, steps=odd) == -2 and table(fn, cmap=odd) == -2
    sq = lib.rdetr_grad_sqnorm_f32
    assert sq(one, one, one, 2, 3, CHUNK, 0, None, 20, None) == -1 and sq(one, one, one, 2, 3, CHUNK, 0, one, 19, None) == -1
    assert sq(one, one, one, 2, 3, CHUNK, 0, ctypes.c_void_p(6), 20, None) == -2
    assert lib.rdetr_adamw_step_f32(one, one, one, 2, 3, CHUNK, 0, ctypes.c_void_p(6), None) == -2
    coef = lib.rdetr_grad_clip_coef
    assert coef(None, 20, 3, 0.1, None) == -1 and coef(one, 19, 3, 0.1, None) == -1 and coef(one, 20, -1, 0.1, None) == -1
    assert coef(one, 4, 0, 0.1, None) == -1 and coef(ctypes.c_void_p(6), 20, 3, 0.1, None) == -2


def test_train_step_on_cpu_is_the_hand_written_loop():
    from oracle.cpu_modules import OracleMSDA, OracleRelation, OracleSelfAttention
    from relation_detr_amd import denoising as dn
    from test_denoising_host import EXPECTED_KEYS, C, head_inputs, tiny_head
    kw = dict(msda_cls=OracleMSDA, self_attn_cls=OracleSelfAttention, relation_cls=OracleRelation)
    a, b = tiny_head("cpu", False, **kw).train(), tiny_head("cpu", False, **kw).train()
    (feats, masks, pos), targets = head_inputs("cpu")
    oa = FusedAdamW(relation_param_groups(a, 1e-4), lr=1e-4, weight_decay=1e-4, fused=False)
    ob = torch.optim.AdamW(relation_param_groups(b, 1e-4), lr=1e-4, weight_decay=1e-4)
    groups = dn.denoising_groups(6, 3)
    before = [p.detach().clone() for p in a.parameters()]
    for step in range(2):
        noise = dn.cdn_noise(11 + step, 2 * groups * 5, C, "cpu")
        losses, norm = train_step(a, oa, feats, masks, pos, targets, max_norm=0.1, noise=noise)
        ob.zero_grad()
        want = b(feats, masks, pos, targets, noise=noise)
        sum(want.values()).backward()
        want_norm = torch.nn.utils.clip_grad_norm_([p for g in ob.param_groups for p in g["params"]], 0.1)     # in group order
        ob.step()
        assert set(losses) == EXPECTED_KEYS and norm.ndim == 0 and torch.equal(norm, want_norm) and norm > 0.1
        for k in want:
            assert torch.equal(losses[k], want[k]), (step, k)
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q), (step, n)
    moved = sum(not torch.equal(p, q) for p, q in zip(a.parameters(), before))
    assert moved > 0.5 * len(before)
    _, norm = train_step(a, oa, feats, masks, pos, targets, max_norm=0, noise=noise)
    assert norm is None
