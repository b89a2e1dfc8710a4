"""Every kernel launch of the benchmarked stack, checked on the exact inputs the network hands it (tests/shadow.py): bench.py's
networks and pyramids at full size, every element of every call against a float64 reference, the set of kernel entries each
run calls pinned.  Then the harness's own fault detection (eval and training step), every Options switch that acts in
eval mode flipped alone against the defaults -- with the assert that the flip changes what is launched -- and the band-interleaved
gather decode at the largest value the fast path accepts.

Runs (each its own test):
  * R50, bf16, B = 4 as bench.py launches it (two image groups of B = 2, eager), 900 and 300 queries, select_detections; plus
    one single-group forward at B = 4, where `auto` takes the resident gather at BASELINE.json configs[1].
  * FocalNet-L, bf16, 900 queries, B = 2: the L = 5 query-run gather with band-interleaved block order on all 204,098 rows.
  * R50, fp32, B = 1.
  * One bf16 training step (forward + backward) of the R50-size network in training mode, B = 2, with 2 x 50 denoising queries:
    with the defaults and with msda_train_fused + attn_train_fused on.  300 matching queries instead of 900 (the hybrid branch
    keeps its 1500) to bound the float64 autograd references of the backward entries; the R50 pyramid is kept.
  * One bf16 training step at the mid-size ragged pyramid (MID_SHAPES, B = 2, 20,274 encoder rows) with ALL SIX training
    switches on, atomic and deterministic: the smallest shapes at which every opt-in training route applies (the FFN route needs
    >= 16,384 rows, the head-major MSDA route S >= 4096; the decoder runs 400 rows, the hybrid branch 1,500 per image), the
    full 6 + 6 layers.  Every launch checked, the op set and the launch counts pinned; then the same step with the switches on,
    with the defaults and in fp32, gradient by gradient (what per-launch checks cannot see: a gradient dropped or sent to the
    wrong operand).
Every image batch has right / bottom padding on one image.
"""
import dataclasses

import pytest
import torch

import shadow

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ------------------------------------------------------------------------------------------- the switch A/B parameter list
# switches that act only where a gradient is needed: an eval-mode A/B of them compares the default route with itself.  All of them
# are on in test_shadow_all_training_routes_step / test_training_routes_match_defaults_against_fp32 below (TRAIN_SWITCHES), and
# their own test files compare both routes against float64 / the reference
_HERE = "tests/test_gpu_shadow_stack.py"
COVERED_ELSEWHERE = {
    "msda_train_fused": (_HERE, "tests/test_gpu_msda_train_fused.py"),
    "attn_train_fused": (_HERE, "tests/test_gpu_attn_train.py"),
    "rel_train_fused": (_HERE, "tests/test_gpu_attn_rel_train.py"),
    "ffn_train_fused": (_HERE, "tests/test_gpu_ffn_train.py"),
    "msda_train_head_major": (_HERE, "tests/test_gpu_msda_train_hm.py"),
    "ln_train_fused": (_HERE, "tests/test_gpu_ln_train.py"),
}
# what the training-step tests switch on (tests/test_shadow_complete.py holds this against COVERED_ELSEWHERE)
TRAIN_SWITCHES = ("msda_train_fused", "attn_train_fused", "rel_train_fused", "ffn_train_fused", "msda_train_head_major", "ln_train_fused")


def _ab_cases():
    """Every bool field flipped, mask_in_kernel forced both ways.  A field of any other kind gets no case until it is handled
    here, so tests/test_shadow_complete.py reports it as untested."""
    from relation_detr_amd.options import Options
    cases = []
    for f in dataclasses.fields(Options):
        if f.name in COVERED_ELSEWHERE:
            continue
        if f.name == "mask_in_kernel":
            cases += [(f.name, "always"), (f.name, "never")]
        elif isinstance(f.default, bool):
            cases.append((f.name, not f.default))
    return cases


AB_CASES = _ab_cases()

# --------------------------------------------------------------------------------------------------------- inputs
EVAL_BF16_OPS = {"tokens_from_levels", "pyramid_points", "encoder_proj", "ms_deform_attn_forward_fused", "linear_ln_k256", "ffn_k256",
                 "add_layer_norm", "row_max", "topk", "box_head_k256", "decoder_reference", "query_pos_k256", "relation_attention",
                 "relation_attention_boxes", "detections_from_topk"}
EVAL_FP32_OPS = {"tokens_from_levels", "pyramid_points", "zero_masked_rows_", "ms_deform_attn_forward_fused", "add_layer_norm", "row_max",
                 "topk", "decoder_reference", "scaled_pos", "relation_bias", "bias_softmax_", "box_refine", "detections_from_topk"}
TRAIN_OPS = {"ms_deform_attn_forward", "ms_deform_attn_backward", "relation_bias", "relation_bias_backward", "bias_softmax_"}
TRAIN_FUSED_OPS = {"ms_deform_attn_forward_fused", "ms_deform_attn_backward_fused", "relation_bias", "relation_bias_backward",
                   "_relation_attention_train", "_relation_attention_backward"}
# all six training switches on, MID_SHAPES, B = 2, 2 x 50 denoising + 300 matching queries, 1500 hybrid queries
TRAIN_ALL_OPS = {
    "value_to_head_major",                                 # encoder MSDA: _trains_head_major (bf16, Nq == S = 10,137 >= 4096), the eval
    "ms_deform_attn_forward_fused",                        # path's relayout and gather; the decoder's cross-attention gather too
    "msda_train_hm.ms_deform_attn_backward_fused_hm",      # ... and its backward on the head-major value
    "msda_train_hm.grad_value_from_head_major",            # ... whose grad_value goes back to [B,S,256] bf16, padded rows zero
    "ms_deform_attn_backward_fused",                       # decoder cross-attention (400 / 1500 queries != S): msda_train_fused
    "ffn_train.ffn_k256_train",                            # encoder FFN: _fused_ffn_train_applies, 20,274 rows >= 16,384
    "ffn_train.ffn_k256_backward",                         # (the decoder's 800 / 3000 rows stay with the library GEMMs)
    "ln_train.add_layer_norm_train",                       # every add_norm and the encoder's _output(post_norm=...): ln_train_fused
    "ln_train.add_layer_norm_backward",
    "attn_rel_train._relation_attention_boxes_train",      # decoder layers 1.. of the main pass: a deferred relation bias, rel_train_fused
    "attn_rel_train._relation_attention_boxes_backward",
    "_relation_attention_train",                           # main pass layer 0 (bool denoising mask, no bias yet) and every layer of the
    "_relation_attention_backward",                        # hybrid pass (skip_relation: no bias, no mask): attn_train_fused
}


@pytest.fixture(scope="module")
def bench():
    import bench as b
    return b


def _padded_pyramid(bench, B, shapes, dtype, seed=11):
    feats, masks, pos = bench.build_pyramid(B, DEV, seed, dtype=dtype, shapes=shapes)
    for m in masks:                                   # last image: right and bottom padding on every level
        h, w = m.shape[1:]
        m[-1, :, max(1, w * 7 // 8):] = True
        m[-1, max(1, h * 9 // 10):, :] = True
    return feats, masks, pos


def _eval_run(net, feats, masks, pos, groups):
    from relation_detr_amd.graph import ImageGroups
    from relation_detr_amd.transformer import select_detections
    L = len(feats)
    B = feats[0].shape[0]
    sizes = torch.tensor([[800, 1333]] * B, device=DEV)

    @torch.no_grad()
    def fwd(*t):
        classes, coords = net(list(t[:L]), list(t[L:2 * L]), list(t[2 * L:3 * L]))[:2]
        return select_detections(classes[-1].float(), coords[-1].float(), t[3 * L])
    run = ImageGroups(fwd, groups, device=DEV) if groups > 1 else fwd
    out = run(*feats, *masks, *pos, sizes)
    torch.cuda.synchronize()
    return out


def _report(sh, title):
    text = sh.report(title)
    launches = ", ".join(f"{k} x{v}" for k, v in sorted(sh.launches.items()))
    print(f"C launches: {launches}")
    return text


# ----------------------------------------------------------------------------------------------------- full-size runs
@pytest.mark.parametrize("queries", [900, 300])
def test_shadow_r50_bf16_bench_launch(bench, monkeypatch, queries):
    """bench.py's default launch: bf16, B = 4 in two image groups of B = 2, eager; then one group of B = 4 (the resident gather)."""
    net = bench.build_network(queries, 0).to(DEV).to(torch.bfloat16)
    feats, masks, pos = _padded_pyramid(bench, 4, bench.CONFIGS["r50"]["shapes"], torch.bfloat16)
    sh = shadow.Shadow(monkeypatch)
    det = _eval_run(net, feats, masks, pos, groups=2)
    _report(sh, f"R50 bf16, {queries} queries, B = 4 as two image groups")
    assert det.shape == (4, 300, 6) and torch.isfinite(det).all()
    sh.assert_ok(EVAL_BF16_OPS)
    assert sh.launches["rdetr_msda_forward_fused_resident_bf16"] == 2 * 6          # every encoder layer of both groups
    monkeypatch.undo()
    sh = shadow.Shadow(monkeypatch)
    _eval_run(net, feats, masks, pos, groups=1)
    _report(sh, f"R50 bf16, {queries} queries, B = 4 as one group")
    sh.assert_ok(EVAL_BF16_OPS)
    assert sh.launches["rdetr_msda_forward_fused_resident_bf16"] == 6


def test_shadow_focalnet_bf16(bench, monkeypatch):
    """FocalNet-L, bf16, B = 2, 900 queries: the 5-level query-run gather in band-interleaved order, every one of 204,098 rows."""
    cfg = bench.CONFIGS["focalnet"]
    net = bench.build_network(900, 0, num_levels=5).to(DEV).to(torch.bfloat16)
    feats, masks, pos = _padded_pyramid(bench, cfg["batch"], cfg["shapes"], torch.bfloat16)
    sh = shadow.Shadow(monkeypatch)
    det = _eval_run(net, feats, masks, pos, groups=1)
    _report(sh, "FocalNet-L bf16, 900 queries, B = 2")
    assert torch.isfinite(det).all()
    sh.assert_ok(EVAL_BF16_OPS)
    assert sh.launches["rdetr_msda_forward_fused_opt_bf16"] >= 6 and not sh.launches["rdetr_msda_forward_fused_resident_bf16"]


def test_shadow_r50_fp32(bench, monkeypatch):
    """R50, fp32, B = 1 (one image group): the fp32 kernels at their 1e-4-class bounds."""
    net = bench.build_network(900, 0).to(DEV)
    feats, masks, pos = _padded_pyramid(bench, 1, bench.CONFIGS["r50"]["shapes"], torch.float32)
    sh = shadow.Shadow(monkeypatch)
    _eval_run(net, feats, masks, pos, groups=1)
    _report(sh, "R50 fp32, 900 queries, B = 1")
    sh.assert_ok(EVAL_FP32_OPS)


def _dn_inputs(B, ndn_groups, per_group, N, gen):
    """Denoising queries (labels [B,Ndn,256], logit-space boxes [B,Ndn,4]) and their visibility mask [Ndn+N, Ndn+N]."""
    Ndn = ndn_groups * per_group
    label = torch.randn(B, Ndn, 256, generator=gen)
    box = torch.randn(B, Ndn, 4, generator=gen)
    mask = torch.zeros(Ndn + N, Ndn + N, dtype=torch.bool)
    mask[Ndn:, :Ndn] = True                                   # matching queries do not see the denoising queries
    for g in range(ndn_groups):                               # denoising groups do not see each other
        lo, hi = g * per_group, (g + 1) * per_group
        mask[lo:hi, :lo] = True
        mask[lo:hi, hi:Ndn] = True
    return label, box, mask


@pytest.mark.parametrize("fused", [False, True], ids=["defaults", "train_fused"])
def test_shadow_r50_bf16_training_step(bench, monkeypatch, fused):
    """Forward + backward of the R50-size network in training mode, bf16, B = 2, 2 x 50 denoising queries, 300 matching queries
    (the hybrid branch keeps its 1500).  Backward entries are checked by float64 autograd on the recorded inputs."""
    from relation_detr_amd import options
    net = bench.build_network(300, 0).to(DEV).to(torch.bfloat16).train()
    if fused:
        options.apply(net, msda_train_fused=True, attn_train_fused=True)
    feats, masks, pos = _padded_pyramid(bench, 2, bench.CONFIGS["r50"]["shapes"], torch.bfloat16)
    label, box, mask = _dn_inputs(2, 2, 50, 300, torch.Generator().manual_seed(5))
    sh = shadow.Shadow(monkeypatch)
    with torch.enable_grad():
        outs = net(feats, masks, pos, label.to(DEV, torch.bfloat16), box.to(DEV), mask.to(DEV))
        loss = sum((o.float() * torch.cos(torch.arange(o.numel(), device=DEV, dtype=torch.float32) * 0.37 + i).view(o.shape)).sum()
                   for i, o in enumerate(outs) if o is not None)
        loss.backward()
    torch.cuda.synchronize()
    _report(sh, f"R50 bf16 training step ({'msda_train_fused + attn_train_fused' if fused else 'defaults'})")
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.encoder.parameters())
    sh.assert_ok(TRAIN_FUSED_OPS if fused else TRAIN_OPS)


# ------------------------------------------------------------------------------- every training route in one step
MID_SHAPES = [(75, 101), (38, 51), (19, 26), (10, 13)]       # ragged levels; S = 10,137, B = 2: 20,274 encoder rows (fused FFN)


def _loss(outs):
    return sum((o.float() * torch.cos(torch.arange(o.numel(), device=DEV, dtype=torch.float32) * 0.37 + i).view(o.shape)).sum()
               for i, o in enumerate(outs) if o is not None)


def _mid_training_step(bench, switches, dtype=torch.bfloat16, feature_grad=False, selection=None):
    """One forward + backward of the full 6 + 6-layer network in training mode at MID_SHAPES, B = 2, with 2 x 50 denoising
    queries: the same bf16-valued inputs and initial weights whatever `dtype` -> (net, feats).
    `selection`: a list.  Empty: the indices of every torch.topk of the step (the two-stage proposal selections of the main and
    the hybrid branch) are appended to it; filled: they are taken from it instead of from this run's own scores."""
    from relation_detr_amd import options
    real_topk, replay = torch.topk, list(selection or ())

    def topk(x, k, dim=-1, **kw):
        if replay:
            idx = replay.pop(0)
            return x.gather(dim, idx), idx
        values, idx = real_topk(x, k, dim=dim, **kw)
        if selection is not None:
            selection.append(idx.clone())
        return values, idx
    net = bench.build_network(300, 0).to(DEV).to(torch.bfloat16).to(dtype).train()
    options.apply(net, **dict.fromkeys(switches, True))
    feats, masks, pos = _padded_pyramid(bench, 2, MID_SHAPES, torch.bfloat16)
    feats, pos = [f.to(dtype) for f in feats], [p.to(dtype) for p in pos]
    if feature_grad:
        feats[0].requires_grad_(True)
    label, box, mask = _dn_inputs(2, 2, 50, 300, torch.Generator().manual_seed(5))
    mp = pytest.MonkeyPatch()
    try:
        if selection is not None:
            mp.setattr(torch, "topk", topk)
        with torch.enable_grad():
            _loss(net(feats, masks, pos, label.to(DEV, torch.bfloat16).to(dtype), box.to(DEV), mask.to(DEV))).backward()
        torch.cuda.synchronize()
    finally:
        mp.undo()
    assert not replay, "a recorded proposal selection was not used"
    return net, feats


def _ratio_table(sh):
    worst = {}
    for r in sh.records:
        worst[r.op] = max(worst.get(r.op, 0.0), r.ratio)
    return worst


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "deterministic"])
def test_shadow_all_training_routes_step(bench, monkeypatch, deterministic):
    """All six training switches on (TRAIN_SWITCHES): every launch of the step inside a checked entry and within its bound, the
    op set pinned, the launch counts as the layer counts give them.  `deterministic`: the sorted grad_value sums of the two MSDA
    backwards instead of float atomics, at the same bounds."""
    sh = shadow.Shadow(monkeypatch)
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(deterministic)
        net, _ = _mid_training_step(bench, TRAIN_SWITCHES)
    finally:
        torch.use_deterministic_algorithms(was)
    _report(sh, f"mid-size bf16 training step, all six training switches ({'deterministic' if deterministic else 'atomic'})")
    assert_all_training_routes(sh, net)


def assert_all_training_routes(sh, net):
    """What a bf16 training step with all six switches on has to show, whatever its shapes (tall enough for every route): no error,
    every ratio below 1, the op set, the launch counts as the layer counts give them, a finite gradient for every parameter of the
    encoder and the decoder."""
    assert not sh.errors, sorted(set(sh.errors))
    sh.assert_ok(TRAIN_ALL_OPS)
    assert max(_ratio_table(sh).values()) < 1.0
    E, D, passes = len(net.encoder.layers), len(net.decoder.layers), 2               # passes: the main and the hybrid decoder pass
    norms = 2 * E + 1 + 1 + passes * D * 4       # norm1 + norm2 per encoder layer, memory_fusion's norm, enc_output_norm; norm2, norm1,
    want = {                                     # norm3 of a decoder layer and the decoder's own norm after it, in both passes
        "rdetr_value_to_head_major_bf16": E,
        "rdetr_msda_backward_fused_hm_bf16": E,
        "rdetr_grad_value_from_head_major_bf16": E,
        "rdetr_msda_backward_fused_bf16": passes * D,
        "rdetr_ffn_k256_train_bf16": E,
        "rdetr_ffn_k256_backward_bf16": E,
        "rdetr_ffn_k256_pack_bf16": 2 * E,                                           # one re-layout of the weights per direction
        "rdetr_add_layernorm_train_bf16": norms,
        "rdetr_add_layernorm_backward_bf16": norms,
        "rdetr_relation_attention_boxes_train_bf16": D - 1,
        "rdetr_relation_attention_boxes_backward_bf16": D - 1,
        "rdetr_relation_attention_train_bf16": 1 + D,
        "rdetr_relation_attention_backward_bf16": 1 + D,
    }
    got = {k: sh.launches[k] for k in want}
    assert got == want, (got, want)
    assert sh.calls["ln_train.add_layer_norm_train"] == norms and sh.calls["ffn_train.ffn_k256_backward"] == E
    for name, p in list(net.encoder.named_parameters()) + list(net.decoder.named_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name


def _nrel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_training_routes_match_defaults_against_fp32(bench):
    """The same step three times -- all six switches on (bf16), the defaults (bf16), the defaults in fp32 -- on the same inputs
    and initial weights.  For every parameter and the level-0 feature: the normwise gradient error against the fp32 run with
    the switches on is at most 1.25 x the defaults' + 2e-2, and so is the mean over the parameters (the criterion and constants
    of tests/test_gpu_attn_rel_train.py::test_transformer_g8_bf16_training_switch_on_matches_off).
    The two bf16 runs take the fp32 run's two-stage proposal selection (the indices of its two torch.topk calls).  Left to their
    own scores they pick and ORDER the proposals differently -- the encoder scores of a random-init network are near ties, bf16
    noise is ~20 rank spacings (bench.build_network) -- and the loss weights every query slot differently: measured without it,
    both bf16 runs are 1.0-1.5 normwise from the fp32 gradients on every parameter (mean 1.17 switches on, 1.11 defaults), i.e.
    uncorrelated with them, and the criterion compares noise with noise."""
    runs, selection = {}, []
    for key, switches, dtype in (("fp32", (), torch.float32), ("on", TRAIN_SWITCHES, torch.bfloat16), ("off", (), torch.bfloat16)):
        net, feats = _mid_training_step(bench, switches, dtype, feature_grad=True, selection=selection)
        assert len(selection) == 2 and selection[0].shape == (2, 300) and selection[1].shape == (2, 1500)
        grads = {n: p.grad for n, p in net.named_parameters()}
        grads["<level-0 feature>"] = feats[0].grad
        runs[key] = grads
        del net
    assert set(runs["on"]) == set(runs["off"]) == set(runs["fp32"])
    rows, bad = [], []
    for n, ref in runs["fp32"].items():
        g_on, g_off = runs["on"][n], runs["off"][n]
        assert (g_on is None) == (ref is None) == (g_off is None), n
        if ref is None:
            continue
        assert bool(torch.isfinite(g_on).all()), n
        if not ref.any():
            assert not g_on.any() and not g_off.any(), n
            continue
        e_on, e_off = _nrel(g_on, ref), _nrel(g_off, ref)
        rows.append((n, e_on, e_off))
        if not e_on <= 1.25 * e_off + 2e-2:
            bad.append((n, e_on, e_off))
    print("gradient error against the fp32 step (normwise): parameter, six switches on, defaults")
    for n, e_on, e_off in rows:
        print(f"{n:64s} {e_on:10.3e} {e_off:10.3e}{'   <-- over 1.25 x + 2e-2' if (n, e_on, e_off) in bad else ''}")
    m_on, m_off = sum(r[1] for r in rows) / len(rows), sum(r[2] for r in rows) / len(rows)
    print(f"{'mean over ' + str(len(rows)) + ' tensors':64s} {m_on:10.3e} {m_off:10.3e}")
    assert not bad, bad
    assert m_on <= 1.25 * m_off + 2e-2, (m_on, m_off)


# ------------------------------------------------------------------------------------------------ the harness can fail
def _swap_tiles(name, call, args, result, fn):
    out = result.clone()
    out[0, 64:128], out[0, 128:192] = result[0, 128:192], result[0, 64:128]
    result.copy_(out)
    return result


def _bump_channel(name, call, args, result, fn):
    col = int(result.float().abs().amax(dim=tuple(range(result.dim() - 1))).argmax())      # the channel of the largest scale
    scale = result[..., col].float().abs().max()
    result[..., col] += (2.0 ** -5 * scale).to(result.dtype)
    return result


def _drop_key_tile(name, call, args, result, fn):
    a = dict(args)
    M = a["k"].shape[1]
    m = (M - 1) // 64 * 64
    for key in ("k", "v", "tgt_boxes"):
        a[key] = a[key][:, :m]
    if a["mask"] is not None:
        a["mask"] = a["mask"][:, :m]
    return fn(**a)


FAULTS = {"gather_tiles_swapped": ("ms_deform_attn_forward_fused", 1, _swap_tiles),
          "ffn_channel_bumped": ("ffn_k256", 2, _bump_channel),
          "attention_last_key_tile_dropped": ("relation_attention_boxes", 1, _drop_key_tile)}


def _swap_dx_tiles(name, call, args, result, fn):
    _swap_tiles(name, call, args, result[0], fn)                       # (dx, dH): rows 64-127 and 128-191 of dx exchanged
    return result


def _bump_dgamma(name, call, args, result, fn):
    dgamma = result[1]
    col = int(dgamma.float().abs().argmax())
    dgamma[col] = (dgamma[col].float() * (1 + 2.0 ** -5)).to(dgamma.dtype)
    return result


def _forget_mask(name, call, args, result, fn):
    return fn(args["grad_hm"], None)


TRAIN_FAULTS = {"ffn_dx_tiles_swapped": ("ffn_train.ffn_k256_backward", 2, _swap_dx_tiles),
                "ln_dgamma_channel_bumped": ("ln_train.add_layer_norm_backward", 3, _bump_dgamma),
                "grad_value_mask_forgotten": ("msda_train_hm.grad_value_from_head_major", 1, _forget_mask)}


def _injector(op, call, fault):
    def inject(name, c, args, result, fn):
        return fault(name, c, args, result, fn) if (name, c) == (op, call) else result
    return inject


def test_shadow_reports_injected_faults(bench, monkeypatch):
    """A small bf16 stack (ragged pyramid, B = 2, 300 queries): clean, then one fault at a time injected through the wrapper.
    Each is reported as exactly that op and call index, nothing else.  Then the same for the training step with all six
    training switches on (its clean run is test_shadow_all_training_routes_step)."""
    net = bench.build_network(300, 0).to(DEV).to(torch.bfloat16)
    feats, masks, pos = _padded_pyramid(bench, 2, MID_SHAPES, torch.bfloat16)
    sh = shadow.Shadow(monkeypatch)
    _eval_run(net, feats, masks, pos, groups=1)
    _report(sh, "mid-size stack, clean")
    sh.assert_ok(EVAL_BF16_OPS)
    for label, (op, call, fault) in FAULTS.items():
        monkeypatch.undo()
        sh = shadow.Shadow(monkeypatch, fault=_injector(op, call, fault))
        _eval_run(net, feats, masks, pos, groups=1)
        bad = [(r.op, r.call) for r in sh.failures()]
        print(label, "->", [(r.op, r.call, round(r.ratio, 2), r.failing, r.where) for r in sh.failures()])
        assert bad == [(op, call)], (label, bad)
    del net
    for label, (op, call, fault) in TRAIN_FAULTS.items():
        monkeypatch.undo()
        sh = shadow.Shadow(monkeypatch, fault=_injector(op, call, fault))
        _mid_training_step(bench, TRAIN_SWITCHES)
        bad = [(r.op, r.call) for r in sh.failures()]
        print(label, "->", [(r.op, r.call, round(r.ratio, 2), r.failing, r.where) for r in sh.failures()])
        assert not sh.errors, sorted(set(sh.errors))
        assert bad == [(op, call)], (label, bad)


# ----------------------------------------------------------------------------------------- every switch against defaults
SMALL_SHAPES = [(38, 51), (19, 26), (10, 13), (5, 7)]         # S = 2,597 < 4096: the encoder's gather is not head-major
# cases whose flip launches exactly what the defaults launch at the common inputs get a setting at which it does not:
#   linear_k256 serves linear1 of a tall FFN only where the fused FFN block (ffn_fused, default on) has not taken it, so both
#     sides of its case run with ffn_fused off;
#   mask_in_kernel = "always" is what None already picks for the decoder (4 Nq <= S), and the encoder's head-major gather has
#     the padding fill in its relayout either way: below S = 4096 the encoder fills by default and masks in the kernel when forced
AB_SCENARIOS = {("linear_k256", True): dict(shapes=MID_SHAPES, base={"ffn_fused": False}),
                ("mask_in_kernel", "always"): dict(shapes=SMALL_SHAPES, base={})}
AB_COMMON = dict(shapes=MID_SHAPES, base={})


@pytest.fixture(scope="module")
def ab_baseline(bench):
    """(field, value) -> the baseline of that case's scenario, built once per scenario."""
    built = {}

    def get(field, value):
        sc = AB_SCENARIOS.get((field, value), AB_COMMON)
        key = (tuple(sc["shapes"]), tuple(sorted(sc["base"].items())))
        if key not in built:
            built[key] = _ab_build(bench, sc["shapes"], sc["base"])
        return built[key]
    return get


def _ab_build(bench, shapes, base):
    from relation_detr_amd import options
    net = bench.build_network(300, 0, exchangeable_queries=False)
    # the reference's init leaves every LayerNorm at weight 1 / bias 0 and several projection biases at 0, so norm1, norm2,
    # norm3 and enc_output_norm would be interchangeable: distinct seeded values make a fused epilogue that reads the wrong
    # norm's parameters, or drops a bias, visible
    g = torch.Generator().manual_seed(33)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
        for name, p in net.named_parameters():
            if name.endswith("bias") and not p.any():
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
    net = net.to(DEV).to(torch.bfloat16)
    defaults = {f.name: f.default for f in dataclasses.fields(options.Options)}
    defaults.update(base)
    options.apply(net, **defaults)
    feats, masks, pos = _padded_pyramid(bench, 2, shapes, torch.bfloat16, seed=21)
    seen = {}
    net.encoder.register_forward_hook(lambda m, i, o: seen.__setitem__("memory", o.detach().float().clone()))
    net.encoder_class_head.register_forward_hook(lambda m, i, o: seen.__setitem__("enc_logits", o.detach().float().clone()))
    with torch.no_grad():
        got = net(feats, masks, pos)
        mem, ref = seen["memory"], got[3].float().clone()
        geo, vr = net.level_misc(masks)
        kw = dict(key_padding_mask=net.flatten_levels(masks), reference_points=ref, spatial_shapes=geo["shapes"],
                  level_start_index=geo["start"], valid_ratios=vr)
        cls, box = net.decoder(query=net.tgt_embed.weight.expand(2, -1, -1), value=mem.to(torch.bfloat16), **kw)
    b = dict(net=net, defaults=defaults, inputs=(feats, masks, pos), seen=seen, memory=mem, kw=kw, enc_logits=seen["enc_logits"],
             cls=cls.float().clone(), box=box.float().clone(), proposals=ref)
    b["launches"] = _ab_sequence(b)[1]                # what the defaults launch over the sequence every case runs
    return b


def _ab_sequence(b):
    """The three calls a case compares -- the network, the decoder on the baseline's memory and proposals, the detections from the
    baseline's decoder outputs -- with the network's current options, under the counting tripwires alone (no references)
    -> ((network outputs, memory, encoder logits, decoder classes, decoder boxes, detections), launches per rdetr_* symbol)."""
    from relation_detr_amd.transformer import select_detections
    net, seen = b["net"], b["seen"]
    feats, masks, pos = b["inputs"]
    mp = pytest.MonkeyPatch()
    try:
        sh = shadow.Shadow(mp, check=False)
        with torch.no_grad():
            got = net(feats, masks, pos)
            mem, enc_logits = seen["memory"], seen["enc_logits"]
            cls, box = net.decoder(query=net.tgt_embed.weight.expand(2, -1, -1), value=b["memory"].to(torch.bfloat16), **b["kw"])
            det = select_detections(b["cls"][-1], b["box"][-1], AB_SIZES.to(DEV), opts=net.options)
        torch.cuda.synchronize()
    finally:
        mp.undo()
    return (got, mem, enc_logits, cls, box, det), +sh.launches


AB_SIZES = torch.tensor([[600, 800], [600, 800]])


def _matched(a, b, tol):
    """Share of the rows of a [B, K, 4] that have a row of b (same image) within `tol` in the max norm."""
    return (torch.cdist(a.double(), b.double(), p=float("inf")).amin(-1) <= tol).float().mean().item()


@pytest.mark.parametrize("field,value", AB_CASES, ids=[f"{f}={v}" for f, v in AB_CASES])
def test_switch_alone_matches_defaults(bench, ab_baseline, field, value):
    """One Options switch flipped on the built bf16 network (distinct LayerNorm parameters and biases, see _ab_build): encoder
    memory within bf16 noise of the all-default run; the encoder class logits over every token elementwise and the two-stage
    proposal boxes as a set (a near tie at the cut may swap a few); the decoder (per layer, logits and boxes) on IDENTICAL
    memory and proposals within the bound of the bf16-vs-fp32 decoder test; the detections drawn from identical decoder outputs
    the same.  And the multiset of rdetr_* launches differs from the defaults': no case compares a route with itself."""
    from relation_detr_amd import options
    from relation_detr_amd.transformer import select_detections
    b = ab_baseline(field, value)
    assert b["defaults"][field] != value
    net = b["net"]
    try:
        options.apply(net, **{field: value})
        (got, mem, enc_logits, cls, box, det), launches = _ab_sequence(b)
    finally:
        options.apply(net, **b["defaults"])
    det0 = select_detections(b["cls"][-1], b["box"][-1], AB_SIZES.to(DEV), opts=options.Options(**b["defaults"]))
    changed = {k: (b["launches"][k], launches[k]) for k in set(launches) | set(b["launches"]) if launches[k] != b["launches"][k]}
    print(f"{field}={value}: launches that differ from the defaults' (symbol: defaults, flipped) {changed}")
    # the flip must change what is launched: a case whose launches equal the defaults' compares a route with itself
    assert changed, f"{field}={value} launches exactly what the defaults launch at these inputs"
    m0 = b["memory"]
    rel = ((mem - m0).norm() / m0.norm()).item()
    dmem = (mem - m0).abs().max().item()
    spread = (b["cls"] - b["cls"].mean()).abs().max().item()
    dcls = (cls.float() - b["cls"]).abs().amax((1, 2, 3))
    dbox = (box.float() - b["box"]).abs().amax((1, 2, 3))
    e0 = b["enc_logits"]
    enc_spread = (e0 - e0.mean()).abs().max().item()
    denc = (enc_logits - e0).abs().max().item()
    prop_match = _matched(b["proposals"], got[3].float(), 2.0 ** -6)
    print(f"{field}={value}: memory rel L2 {rel:.2e} max {dmem:.3e}; encoder logits max {denc:.4f} (spread {enc_spread:.2f}), "
          f"proposals matched {prop_match:.4f}; decoder per layer logit max {[round(v, 4) for v in dcls.tolist()]} "
          f"(spread {spread:.2f}) box max {[round(v, 5) for v in dbox.tolist()]}")
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    assert rel <= 2.0 ** -6 and dmem <= 0.25, (rel, dmem)
    assert denc <= 2.0 ** -5 * enc_spread, (denc, enc_spread)
    assert prop_match >= 0.98, prop_match
    assert dcls.max().item() <= 2.0 ** -5 * spread and dbox.max().item() <= 5e-3, (dcls.tolist(), dbox.tolist())
    assert bench.detection_drift(det, det0, iou_thr=0.9)["matched_frac"] >= 0.99


# ---------------------------------------------------------------------------------- largest accepted encoder gather
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_band_interleaved_gather_at_the_largest_accepted_value(dtype):
    """The query-run gather with band-interleaved block order (Nq == S, plane > 4 MiB) at nearly the largest S the fast path
    accepts, S * H * D * sizeof(T) < 2^31: bf16 S < 2^22, fp32 S < 2^21.  Five power-of-two levels 2^21 + ... + 2^17 (bf16) /
    2^20 + ... + 2^16 (fp32): S = 31/32 of the limit (96.9 %; the L = 4 and 5 kernels interleave, other level counts do not).
    Every query samples its own pixel centre (x = (i + 0.5) / w exact in fp32, and so is x * w - 0.5) with weight 1 on one
    point, 0 on the rest; channel c < 3 of head h holds byte c of the pixel index, channel 3 holds h, channels >= 4 hold c --
    integers <= 255, exact in bf16.  So every output row has a known exact value; a tile skipped or run twice shows as rows
    that do not decode to their own index.  The output buffer is taken from a freed block filled with NaN, which no row can
    produce.
    ADVICE's overflow (msda_fwd.hip, `bnd * (A[l+1] - A[l])` in 32 bits) is out of reach: a tile holds 64 (bf16) / 32 (fp32)
    queries, so level 0 has T0 < 2^22 / 64 = 2^21 / 32 = 2^16 tiles, k = floor(log2 T0) - 4 <= 11, bnd < 2^k and every level
    has at most T0 tiles: the product stays below 2^11 * 2^16 = 2^27."""
    from relation_detr_amd import ops
    if dtype == torch.bfloat16:
        shapes = [(2048, 1024), (1024, 1024), (1024, 512), (512, 512), (512, 256)]
    else:
        shapes = [(1024, 1024), (1024, 512), (512, 512), (512, 256), (256, 256)]
    S = sum(h * w for h, w in shapes)
    limit = (1 << 31) // (256 * torch.tensor([], dtype=dtype).element_size())
    assert S < limit and S * 32 >= limit * 31
    L, H, P = len(shapes), 8, 4
    shp = torch.tensor(shapes, dtype=torch.int64, device=DEV)
    start = torch.cat([shp.new_zeros(1), (shp[:, 0] * shp[:, 1]).cumsum(0)[:-1]])
    q = torch.arange(S, device=DEV)
    code = torch.zeros(S, H, 32, dtype=torch.float32, device=DEV)
    for c in range(3):
        code[:, :, c] = ((q >> (8 * c)) & 255).float()[:, None]
    code[:, :, 3] = torch.arange(H, device=DEV, dtype=torch.float32)[None]
    code[:, :, 4:] = torch.arange(4, 32, device=DEV, dtype=torch.float32)
    value = code.to(dtype).unsqueeze(0)                                                   # [1, S, H, 32]
    loc = torch.full((1, S, H, L, P, 2), 0.5, dtype=torch.float32, device=DEV)
    attn = torch.zeros(1, S, H, L, P, dtype=torch.float32, device=DEV)
    for l, (h, w) in enumerate(shapes):
        s0 = int(start[l])
        i = torch.arange(h * w, device=DEV)
        xy = torch.stack([((i % w).float() + 0.5) / w, ((i // w).float() + 0.5) / h], -1)
        loc[0, s0:s0 + h * w, :, l, 0, :] = xy[:, None, :]
        attn[0, s0:s0 + h * w, :, l, 0] = 1.0
    want = code.view(S, H * 32).to(dtype)
    def poisoned_block():
        poison = torch.full((1, S, H * 32), float("nan"), dtype=dtype, device=DEV)
        return poison.data_ptr()                               # freed on return: the next allocation of this size gets the block

    ptr = poisoned_block()
    got = ops.ms_deform_attn_forward(value, shp, start, loc, attn, algo="direct" if dtype == torch.bfloat16 else "auto")[0]
    torch.cuda.synchronize()
    assert got.data_ptr() == ptr, "the output did not land in the NaN-filled block"
    bad = (got != want).any(-1)
    rows = bad.nonzero().flatten()
    assert not bool(bad.any()), f"{rows.numel()} of {S} rows wrong, first {rows[:8].tolist()}"
    if dtype == torch.bfloat16:                                                           # the head-major layout of the same map
        vh = value.permute(0, 2, 1, 3).contiguous()
        del got, bad, rows
        ptr = poisoned_block()
        got_hm = ops.ms_deform_attn_forward(vh, shp, start, loc, attn, value_layout="bhsd", algo="direct")[0]
        torch.cuda.synchronize()
        assert got_hm.data_ptr() == ptr, "the output did not land in the NaN-filled block"
        assert torch.equal(got_hm, want)
