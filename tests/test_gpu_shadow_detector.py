"""A whole detector training step under the shadow harness (tests/shadow.py): neck, position encoding, denoising generator,
transformer, criterion, global-norm clip and AdamW, every launch inside a checked entry and within the bound of its unit test.

``train_step(RelationDETR, FusedAdamW, features, mask, None, targets, max_norm=0.1, noise=<keyed draws>)`` with synthetic weights:

  (a) mixed precision: fp32 parameters under ``torch.autocast(bfloat16)``, all six training switches set, the device
      matcher; 2 + 2 layers, 300 queries, 1500 hybrid proposals; three backbone maps (64, 100), (32, 50), (16, 25) and one extra
      level (8, 13), B = 2: S = 8,504 >= 4096 (head-major MSDA) and B S = 17,008 >= 16,384 (fused FFN); the last image padded right
      and bottom; 17 boxes in image 0 and none in image 1, labels over all 91 classes, denoising_nums = 100: 5 groups, 170 denoising
      queries, 470 decoder queries (not a multiple of 8), 17 * 6 = 102 target copies for the device matcher.  TWO consecutive steps:
      the second runs on existing optimizer state (bias correction at step 2) and on weights the first step wrote through raw
      pointers, so every checker that reads the current weights also checks the packed-weight caches behind ``_step_fused``.
      Two of the six switches find nothing to do in this mode and the launch counts pin that: msda_train_head_major and
      rel_train_fused want bf16 WEIGHTS, which fp32 master parameters under autocast are not, so the encoder's MSDA runs
      through the fused-producer gather and its backward and the relation bias through its own fp32 kernel -- HIP routes both.
      Those two routes (and with them the S >= 4096 head-major threshold) therefore stay OUTSIDE every detector-step test; in
      composition they are held only by the transformer-level step of tests/test_gpu_shadow_stack.py, on a ``.to(bfloat16)`` network.
  (b) fp32, defaults, the scipy matcher: the tiny model and inputs of tests/test_gpu_neck.py::test_train_step_steps_the_neck, one
      step: the _f32 kernels at their fp32 bounds in composition, and the host-matcher branch, whose assign_match launches nothing
      and is not recorded.
  (c) (b) with one fault at a time injected through the wrapper: each is reported as exactly one failing record of that op.

With ``RDETR_SHADOW_REPORTS=<directory>`` the report tables of (a) and (b) are written there (profiles/r23/)."""
import os
import time

import pytest
import torch

import shadow
from conftest import load_golden
from helpers import synthetic_state_dict
from test_gpu_shadow_stack import TRAIN_SWITCHES, _ratio_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
MAPS = ((64, 100), (32, 50), (16, 25))           # the backbone's maps; the neck adds (8, 13)
IN_CHANNELS = (16, 24, 40)
CLASSES, QUERIES, HYBRID, DN_NUMS, BOXES = 91, 300, 1500, 100, 17

# ops of the transformer on the routes (a) takes, then the rest of the step
STEP_OPS = {"neck.group_norm_levels_forward", "neck.group_norm_levels_backward", "neck._masks_and_counts", "neck._sine_pos_packed",
            "denoising.cdn_noise", "denoising.denoising_mask", "denoising.cdn_queries_forward", "denoising.cdn_embed_backward",
            "criterion.match_cost", "criterion.set_loss_forward", "optim.FusedAdamW._clip_fused", "optim.FusedAdamW._step_fused"}
AMP_OPS = {"amp_train.add_layer_norm_mixed_train", "amp_train.add_layer_norm_mixed_backward", "amp_train.ffn_mixed_train",
           "amp_train.ffn_mixed_backward"}


def _write_report(name, text, sh):
    out = os.environ.get("RDETR_SHADOW_REPORTS")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name), "w") as f:
            f.write(text + "\nC launches: " + ", ".join(f"{k} x{v}" for k, v in sorted(sh.launches.items())) + "\n")


def _report(sh, title, name):
    text = sh.report(title)
    print("C launches: " + ", ".join(f"{k} x{v}" for k, v in sorted(sh.launches.items())))
    print("ops called: " + ", ".join(sorted(sh.called())))
    _write_report(name, text, sh)


# ------------------------------------------------------------------------------------------------------------------ (a)
def mixed_model():
    from relation_detr_amd import GenerateCDNQueries, RelationCriterion, RelationDETR, options
    from relation_detr_amd.neck import ChannelMapper, PositionEmbeddingSine
    from relation_detr_amd.transformer import build_relation_transformer
    net = build_relation_transformer(num_classes=CLASSES, enc_layers=2, dec_layers=2, num_queries=QUERIES, hybrid_num_proposals=HYBRID)
    net.load_state_dict(synthetic_state_dict(net.state_dict()))
    # enc_output.bias keeps the model's own initial value, zero.  A synthetic bias gives the zeroed memory rows of the padded and
    # out-of-range proposals one common class score (0.64) above every valid token's (at most 0.25); the two-stage selection then
    # takes 300 of those rows, whose boxes are sigmoid(+inf) = 1 with derivative 0, and the encoder's box head gets a zero
    # gradient, which the first step's AdamW turns into no change at all.
    with torch.no_grad():
        net.enc_output.bias.zero_()
    generator = GenerateCDNQueries(num_queries=QUERIES, num_classes=CLASSES, label_embed_dim=256, denoising_nums=DN_NUMS, fused=True)
    generator.load_state_dict(synthetic_state_dict(generator.state_dict()))
    mapper = ChannelMapper(list(IN_CHANNELS), 256, 4, fused=True)
    mapper.load_state_dict(synthetic_state_dict(mapper.state_dict()))
    pe = PositionEmbeddingSine(128, 10000, True, offset=-0.5, fused=True)
    model = RelationDETR(mapper, pe, net, RelationCriterion(CLASSES, fused=True, matcher="device"), generator).to(DEV).train()
    return options.apply(model, **dict.fromkeys(TRAIN_SWITCHES, True))


def mixed_inputs(batch=2, maps=MAPS, counts=(BOXES, 0), hard=()):
    """Backbone maps [batch, c, h, w], the image mask and the targets (`counts` boxes per image).  The last image is padded right and
    bottom; the images in `hard` so far that the coarsest level (the neck's extra one) keeps two valid rows and one valid column."""
    g = torch.Generator().manual_seed(23)
    feats = [torch.randn(batch, c, h, w, generator=g).to(DEV) for c, (h, w) in zip(IN_CHANNELS, maps)]
    H, W = 8 * maps[0][0], 8 * maps[0][1]
    mask = torch.zeros(batch, H, W, dtype=torch.bool)
    mask[batch - 1, :, W * 7 // 8:] = True                                      # the last image: padded right and bottom
    mask[batch - 1, H * 450 // 512:, :] = True
    hc, wc = (maps[-1][0] + 1) // 2, (maps[-1][1] + 1) // 2                      # the extra level: a stride-2 3 x 3 convolution
    for b in hard:                                                              # level pixel (y, x) reads mask[y H // hc, x W // wc]
        mask[b, 2 * H // hc:, :] = True
        mask[b, :, W // wc:] = True
    targets = []
    for n in counts:
        labels = (torch.arange(n) * (CLASSES - 1)) // max(n - 1, 1)             # 0 .. 90
        boxes = torch.cat((0.1 + 0.8 * torch.rand(n, 2, generator=g), 0.03 + 0.3 * torch.rand(n, 2, generator=g)), -1) if n else torch.zeros(0, 4)
        targets.append({"labels": labels.to(DEV), "boxes": boxes.to(DEV)})
    return feats, mask.to(DEV), targets


def test_shadow_mixed_precision_detector_two_steps(monkeypatch):
    mixed_two_steps(monkeypatch, mixed_inputs(), MAPS, "mixed-precision detector, all six training switches, device matcher, two steps",
                    "shadow_detector_mixed.txt")


def mixed_two_steps(monkeypatch, inputs, maps, title, report_name):
    """(a) on `inputs` = mixed_inputs(...) over the backbone maps `maps`: the two steps, then every assertion of the test."""
    from relation_detr_amd import denoising as dn
    from relation_detr_amd.criterion import MAX_ASSIGN
    from relation_detr_amd.optim import FusedAdamW, relation_param_groups, train_step
    model = mixed_model()
    feats, mask, targets = inputs
    counts = [int(t["labels"].numel()) for t in targets]
    assert max(counts) == BOXES
    groups = dn.denoising_groups(DN_NUMS, BOXES)
    n_dn = 2 * groups * BOXES
    assert (groups, n_dn) == (5, 170) and (n_dn + QUERIES) % 8 and BOXES * 6 <= MAX_ASSIGN
    S = sum(h * w for h, w in tuple(maps) + (((maps[-1][0] + 1) // 2, (maps[-1][1] + 1) // 2),))
    assert S >= 4096 and len(counts) * S >= 16384
    opt = FusedAdamW(relation_param_groups(model, 1e-4), lr=1e-4, weight_decay=1e-4, fused=True)
    assert sum(len(g_["params"]) for g_ in opt.param_groups) == len(list(model.parameters()))
    sh = shadow.Shadow(monkeypatch)
    steps, started, unchanged = 2, time.perf_counter(), []
    for step in range(steps):
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        noise = dn.cdn_noise(1234 + step, 2 * groups * sum(counts), CLASSES, DEV)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            losses, norm = train_step(model, opt, feats, mask, None, targets, max_norm=0.1, noise=noise)
        torch.cuda.synchronize()
        assert len(losses) == 3 * (3 * 2 + 2) and all(bool(torch.isfinite(v)) for v in losses.values()) and bool(torch.isfinite(norm))
        unchanged += [(step + 1, k) for k, p in model.named_parameters() if torch.equal(p.detach(), before[k])]
        assert all(float(opt.state[p]["step"]) == step + 1 for p in model.parameters())
    print(f"two mixed-precision detector steps under the harness: {time.perf_counter() - started:.1f} s")
    _report(sh, title, report_name)
    assert not sh.errors, sorted(set(sh.errors))
    assert not unchanged, f"(step, parameter) the step left unchanged: {unchanged}"
    called = sh.called()
    assert AMP_OPS <= called, sorted(AMP_OPS - called)
    sh.assert_ok(MIXED_OPS)
    assert max(_ratio_table(sh).values()) < 1.0
    E, D, passes, stacks = len(model.transformer.encoder.layers), len(model.transformer.decoder.layers), 2, 4
    want = {
        # the neck: one group_norm_levels call over the three mapped levels and the first extra one, each way (the C entry makes
        # its two launches itself); masks + counts and the position encodings one launch each
        "rdetr_group_norm_levels_bf16": steps, "rdetr_group_norm_levels_backward_bf16": steps,
        "rdetr_pyramid_masks": steps, "rdetr_pyramid_sine_pos_bf16": steps,
        "rdetr_cdn_noise": steps, "rdetr_cdn_queries_f32": steps, "rdetr_cdn_mask": steps, "rdetr_cdn_embed_backward_f32": steps,
        # _forward_fused: the four stacks (decoder layers, encoder proposals, hybrid layers, hybrid proposals) get one cost launch
        # and one loss launch each.  The merge rule joins neighbours of one (N, skip, repeat): the hybrid layers and the hybrid
        # proposals (1500, 0, 6) are one launch; the decoder layers (470 queries, 170 skipped) and the encoder proposals (300, 0)
        # are not
        "rdetr_match_cost_bf16": steps * stacks, "rdetr_set_loss_bf16": steps * stacks, "rdetr_assign_match": steps * 3,
        "rdetr_grad_sqnorm_f32": steps, "rdetr_grad_clip_coef": steps, "rdetr_adamw_step_f32": steps,
        # the transformer: the encoder's FFN through the mixed-precision kernels with one fp32 weight pack per direction; every
        # MSDA call, the encoder's too, through the fused-producer gather and its backward (msda_train_head_major wants bf16
        # weights, see the module docstring); the decoder's self-attention through the fused attention kernels of both passes,
        # the relation bias of the main pass's later layers from its own fp32 kernel (rel_train_fused wants bf16 weights too)
        "rdetr_ffn_k256_train_xf32_bf16": steps * E, "rdetr_ffn_k256_backward_dxf32_bf16": steps * E, "rdetr_ffn_k256_pack_f32": steps * 2 * E,
        "rdetr_msda_forward_fused_opt_bf16": steps * (E + passes * D), "rdetr_msda_backward_fused_bf16": steps * (E + passes * D),
        "rdetr_msda_backward_fused_hm_bf16": 0, "rdetr_value_to_head_major_bf16": 0,
        "rdetr_relation_attention_train_bf16": steps * passes * D, "rdetr_relation_attention_backward_bf16": steps * passes * D,
        "rdetr_relation_attention_boxes_train_bf16": 0,
        "rdetr_relation_bias_ws_f32": steps * (D - 1), "rdetr_relation_bias_backward_f32": steps * (D - 1),
    }
    got = {k: sh.launches[k] for k in want}
    assert got == want, (got, want)
    assert sh.calls["criterion.assign_match"] == steps * 3 and sh.calls["optim.FusedAdamW._step_fused"] == steps
    norms = sh.launches["rdetr_add_layernorm_train_mixed"] + sh.launches["rdetr_add_layernorm_train_f32"] + sh.launches["rdetr_add_layernorm_train_bf16"]
    assert norms == steps * (2 * E + 1 + 1 + passes * D * 4), norms             # as test_shadow_all_training_routes_step counts them
    # one norm per decoder layer and pass sees fp32 operands alone (the decoder's own norm of the layer's fp32 output, no residual):
    # ln_train's same-dtype case; every other one has a bf16 operand and is the mixed-precision kernel's
    same_dtype = steps * passes * D
    assert sh.launches["rdetr_add_layernorm_train_f32"] == sh.launches["rdetr_add_layernorm_backward_f32"] == same_dtype
    assert sh.launches["rdetr_add_layernorm_train_mixed"] == sh.launches["rdetr_add_layernorm_backward_mixed"] == norms - same_dtype
    assert sh.calls["amp_train.ffn_mixed_train"] == sh.calls["amp_train.ffn_mixed_backward"] == steps * E


# the whole pinned set of (a): the step's own entries, the four mixed-precision ones, and the transformer's
MIXED_OPS = STEP_OPS | AMP_OPS | {"criterion.assign_match", "ln_train.add_layer_norm_train", "ln_train.add_layer_norm_backward",
                                  "ms_deform_attn_forward_fused", "ms_deform_attn_backward_fused", "_relation_attention_train",
                                  "_relation_attention_backward", "relation_bias", "relation_bias_backward"}


# ------------------------------------------------------------------------------------------------------------------ (b), (c)
def tiny_inputs():
    """tests/test_gpu_neck.py's inputs: the g12 maps and image mask, the g10 targets -> (maps, mask, targets)."""
    g12, z = load_golden("g12_neck.npz"), load_golden("g10_criterion.npz")
    targets = [{"labels": T(z[f"tgt.labels.{b}"]).to(DEV), "boxes": T(z[f"tgt.boxes.{b}"]).to(DEV)} for b in range(2)]
    return [T(g12[f"x{i}"]).to(DEV) for i in range(3)], T(g12["img_mask"]).to(DEV), targets


def tiny_step(monkeypatch, fault=None, inputs=None):
    """One fp32 step of tests/test_gpu_neck.py's tiny model (`inputs`: tiny_inputs() unless given) under the harness
    -> (harness, model, the parameters before the step)."""
    from relation_detr_amd import denoising as dn
    from relation_detr_amd.optim import FusedAdamW, relation_param_groups, train_step
    from test_denoising_host import C
    from test_gpu_neck import tiny_model
    feats, mask, targets = inputs or tiny_inputs()
    counts = [int(t["labels"].numel()) for t in targets]
    model = tiny_model(True).train()
    opt = FusedAdamW(relation_param_groups(model, 1e-3), lr=1e-3, weight_decay=1e-4, fused=True)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    sh = shadow.Shadow(monkeypatch, fault=fault)
    noise = dn.cdn_noise(11, 2 * dn.denoising_groups(6, max(counts)) * sum(counts), C, DEV)
    losses, norm = train_step(model, opt, feats, mask, None, targets, max_norm=0.1, noise=noise)
    torch.cuda.synchronize()
    assert len(losses) == 3 * (3 * 2 + 2) and bool(torch.isfinite(norm))   # 2 decoder layers: 8 sets x 3 losses
    return sh, model, before


def test_shadow_fp32_detector_step(monkeypatch):
    fp32_step(monkeypatch, None, "fp32 detector step, defaults, scipy matcher", "shadow_detector_fp32.txt")


def fp32_step(monkeypatch, inputs, title, report_name):
    """(b) on `inputs` (tiny_inputs() unless given): the step, then every assertion of the test."""
    sh, model, before = tiny_step(monkeypatch, inputs=inputs)
    _report(sh, title, report_name)
    assert not sh.errors, sorted(set(sh.errors))
    sh.assert_ok(FP32_OPS)
    assert max(_ratio_table(sh).values()) < 1.0
    assert "criterion.assign_match" not in sh.calls and not sh.launches["rdetr_assign_match"]          # scipy: nothing launched, nothing recorded
    want = {"rdetr_group_norm_levels_f32": 1, "rdetr_group_norm_levels_backward_f32": 1, "rdetr_pyramid_masks": 1, "rdetr_pyramid_sine_pos_f32": 1,
            "rdetr_cdn_noise": 1, "rdetr_cdn_queries_f32": 1, "rdetr_cdn_mask": 1, "rdetr_cdn_embed_backward_f32": 1,
            "rdetr_match_cost_f32": 4, "rdetr_set_loss_f32": 4, "rdetr_grad_sqnorm_f32": 1, "rdetr_grad_clip_coef": 1, "rdetr_adamw_step_f32": 1}
    got = {k: sh.launches[k] for k in want}
    assert got == want, (got, want)
    same = [k for k, p in model.named_parameters() if torch.equal(p.detach(), before[k])]
    assert not same, same


FP32_OPS = STEP_OPS | {"ms_deform_attn_forward", "ms_deform_attn_backward", "relation_bias", "relation_bias_backward", "bias_softmax_"}


def _bump_dlogits(name, call, args, result, fn):
    result[1][0, 0, 0] += 1e-3
    return result


def _bump_gn_dgamma(name, call, args, result, fn):
    dgamma = result[1]
    col = int(dgamma[0].abs().argmax())
    dgamma[0, col] *= 1 + 2.0 ** -10
    return result


def _bump_parameter(name, call, args, result, fn):
    p = args["self"].param_groups[0]["params"][0]
    with torch.no_grad():
        p.view(-1)[1] += 2.0 ** -12
    return result


DETECTOR_FAULTS = {"set_loss_dlogits_element": ("criterion.set_loss_forward", 2, _bump_dlogits),
                   "group_norm_dgamma_element": ("neck.group_norm_levels_backward", 0, _bump_gn_dgamma),
                   "parameter_element_after_the_step": ("optim.FusedAdamW._step_fused", 0, _bump_parameter)}


@pytest.mark.parametrize("label", list(DETECTOR_FAULTS))
def test_shadow_detector_reports_injected_faults(monkeypatch, label):
    from test_gpu_shadow_stack import _injector
    op, call, fault = DETECTOR_FAULTS[label]
    sh, _, _ = tiny_step(monkeypatch, fault=_injector(op, call, fault))
    bad = [(r.op, r.call, r.failing) for r in sh.failures()]
    print(label, "->", [(r.op, r.call, round(r.ratio, 2), r.failing, r.where) for r in sh.failures()])
    assert not sh.errors, sorted(set(sh.errors))
    assert bad == [(op, call, 1)], (label, bad)
