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

Steps that start at the IMAGES: ``relation_detr_r50`` reduced as tests/test_gpu_backbone.py reduces it (2 + 2 layers, 30 queries, 30 hybrid
proposals, 11 classes, 6 denoising pairs, d_ffn 64), the backbone's weights from its ``randomise``, the others synthetic, the library's
convolutions deterministic.  B = 3; the padded batch is 160 x 224, so the stem's convolution gives 80 x 112, the pool 40 x 56, layer2 to
layer4 20 x 28, 10 x 14 and 5 x 7 (35-element planes, off the 16-byte grid in both dtypes) and the neck's extra level 3 x 4; one image
fills less than half of its slot.  The front end and every epilogue kernel of the ResNet-50 run inside the harness: the in-place
``frozen_bn_act`` on each convolution result as the library hands it over, its backward on the saved output and the library's dy.

  (d) fp32, scipy matcher, one step from three float images (160, 200), (131, 224), (50, 70): the _f32 epilogues at bit equality
  (e) (d) under ``torch.autocast(bfloat16)`` with the six training switches and the device matcher, two steps: the bf16 epilogues on the
      library's bf16 convolution results with fp32 constants; the second step on weights the fused optimizer wrote
  (f) eval from three uint8 images (211, 300), (100, 400), (333, 410) resized by min_size 150 / max_size 224 to (150, 213), (56, 224),
      (150, 184): fp32 and ``.to(bfloat16)``, each with an NCHW and a channels-last batch: ``rdetr_image_batch``'s resize path and
      ``rdetr_stem_pool_*`` (tests/test_shadow_train_host.py holds on the CPU that this batch is inside the near-tie cap)
  (c) also injects one fault per new entry into (d).
The transformer's size-dependent routes (head-major MSDA, the fused FFN) are held by (a); these shapes are below both thresholds.
The launch counts of the epilogues come from the module: one forward per FrozenBatchNorm2d but the stem's (52), one stem pool, one
backward per norm whose convolution has a trainable weight (42 with freeze_indices = (0,)).

With ``RDETR_SHADOW_REPORTS=<directory>`` the report tables of (a), (b), (d), (e) and (f) are written there (profiles/r23/, profiles/r28/)."""
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


# ------------------------------------------------------------------------------------------------------------ (d), (e), (f)
R50_CLASSES, R50_QUERIES, R50_DN = 11, 30, 6
IMAGE_OPS = {"frontend.images.batch_images", "backbones.epilogue.stem_bn_relu_maxpool", "backbones.epilogue.frozen_bn_act_forward"}
BACKBONE_TRAIN_OPS = IMAGE_OPS | {"backbones.epilogue.frozen_bn_act_backward"}


def r50_model(matcher="scipy", switches=False):
    """The reduced ``relation_detr_r50`` of tests/test_gpu_backbone.py::test_detector_with_the_r50_backbone_end_to_end, its front end
    set to resize to the 160 x 224-class batch."""
    import relation_detr_amd
    from helpers import DETECTOR_RESIZE
    from relation_detr_amd import options
    from test_gpu_backbone import randomise
    model = relation_detr_amd.relation_detr_r50(num_classes=R50_CLASSES, num_queries=R50_QUERIES, hybrid_num_proposals=30, enc_layers=2,
                                                dec_layers=2, d_ffn=64, denoising_nums=R50_DN, min_size=DETECTOR_RESIZE[0],
                                                max_size=DETECTOR_RESIZE[1], num_select=10)
    rest = {k: v for k, v in model.state_dict().items() if not k.startswith("backbone.")}
    missing, unexpected = model.load_state_dict(synthetic_state_dict(rest), strict=False)
    assert not unexpected and all(k.startswith("backbone.") for k in missing)
    with torch.no_grad():
        model.transformer.enc_output.bias.zero_()                              # mixed_model has why
    randomise(model.backbone, 46)
    model.criterion.matcher = matcher
    model = model.to(DEV)
    return options.apply(model, **dict.fromkeys(TRAIN_SWITCHES, True)) if switches else model


def epilogue_counts(backbone):
    """(forwards, backwards) of frozen_bn_act per pass, from the module: every FrozenBatchNorm2d but the stem's follows a
    convolution through the kernel; its backward runs where that convolution's weight is trained."""
    from relation_detr_amd.backbones import FrozenBatchNorm2d
    pairs = []
    for module in backbone.modules():
        for i in (1, 2, 3):
            if module is not backbone and isinstance(getattr(module, f"bn{i}", None), FrozenBatchNorm2d):
                pairs.append((getattr(module, f"conv{i}"), getattr(module, f"bn{i}")))
        down = getattr(module, "downsample", None)
        if down is not None:
            pairs.append((down[0], down[1]))
    norms = [m for m in backbone.modules() if isinstance(m, FrozenBatchNorm2d)]
    assert len(pairs) == len(norms) - 1 and {id(n) for _, n in pairs} == {id(n) for n in norms} - {id(backbone.bn1)}
    return len(pairs), sum(conv.weight.requires_grad for conv, _ in pairs)


def image_targets():
    """Boxes in xyxy pixels inside each of the three float images: 3, none and 2."""
    boxes = ([[4.0, 6.0, 120.0, 150.0], [30.0, 2.0, 190.0, 60.0], [100.0, 80.0, 170.0, 158.0]], [], [[5.0, 5.0, 30.0, 40.0], [20.0, 10.0, 66.0, 48.0]])
    labels = ([1, 7, 3], [], [0, 10])
    return [{"labels": torch.tensor(l, dtype=torch.int64, device=DEV), "boxes": torch.tensor(b, dtype=torch.float32, device=DEV).reshape(-1, 4)}
            for l, b in zip(labels, boxes)]


def assert_backbone_launches(sh, model, steps, forwards, suffix, trained):
    fwd, bwd = epilogue_counts(model.backbone)
    other = "_bf16" if suffix == "_f32" else "_f32"
    want = {"rdetr_image_batch": forwards, "rdetr_stem_pool" + suffix: forwards, "rdetr_frozen_bn_act" + suffix: forwards * fwd,
            "rdetr_frozen_bn_act_backward" + suffix: steps * bwd if trained else 0,
            "rdetr_stem_pool" + other: 0, "rdetr_frozen_bn_act" + other: 0, "rdetr_frozen_bn_act_backward" + other: 0}
    got = {k: sh.launches[k] for k in want}
    assert got == want, (got, want)
    assert (fwd, bwd) == (52, 42)                                               # ResNet-50 with the stem and layer1 frozen
    calls = {k: sh.calls[k] for k in BACKBONE_TRAIN_OPS}
    assert calls == {"frontend.images.batch_images": forwards, "backbones.epilogue.stem_bn_relu_maxpool": forwards,
                     "backbones.epilogue.frozen_bn_act_forward": forwards * fwd,
                     "backbones.epilogue.frozen_bn_act_backward": steps * bwd if trained else 0}, calls


def image_steps(monkeypatch, steps, autocast, fault=None):
    """`steps` training steps of the reduced R50 detector from the three float images under the harness -> (harness, model)."""
    from helpers import DETECTOR_BATCH, detector_float_images
    from relation_detr_amd import denoising as dn
    from relation_detr_amd.optim import FusedAdamW, relation_param_groups, train_step
    from test_gpu_backbone import deterministic_convolutions
    model = r50_model("device" if autocast else "scipy", switches=autocast).train()
    images, targets = [im.to(DEV) for im in detector_float_images()], image_targets()
    counts = [int(t["labels"].numel()) for t in targets]
    opt = FusedAdamW(relation_param_groups(model, 1e-4), lr=1e-4, weight_decay=1e-4, fused=True)
    trained = {k for k, p in model.named_parameters() if p.requires_grad}
    assert sum(len(g["params"]) for g in opt.param_groups) == len(trained) < len(list(model.parameters()))
    frozen = {k: t.detach().clone() for k, t in model.state_dict().items() if k not in trained}
    assert any(k.startswith("backbone.layer1.") for k in frozen) and "backbone.layer2.0.conv1.weight" in trained
    head = lambda batch, _, tgts, noise=None: model(batch, tgts, noise)         # noqa: E731  train_step's (feats, masks, targets, noise)
    sh = shadow.Shadow(monkeypatch, fault=fault)
    groups, unchanged = dn.denoising_groups(R50_DN, max(counts)), []
    for step in range(steps):
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        noise = dn.cdn_noise(77 + step, 2 * groups * sum(counts), R50_CLASSES, DEV)
        with deterministic_convolutions(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            losses, norm = train_step(head, opt, images, None, None, targets, max_norm=0.1, noise=noise)
        torch.cuda.synchronize()
        assert len(losses) == 3 * (3 * 2 + 2) and all(bool(torch.isfinite(v)) for v in losses.values()) and bool(torch.isfinite(norm))
        unchanged += [(step + 1, k) for k in trained if torch.equal(model.get_parameter(k).detach(), before[k])]
    assert not unchanged, f"(step, parameter) the step left unchanged: {unchanged}"
    moved = [k for k, t in model.state_dict().items() if k in frozen and not torch.equal(t.view(torch.uint8), frozen[k].view(torch.uint8))]
    assert not moved, f"frozen parameters and buffers that changed: {moved}"
    assert tuple(DETECTOR_BATCH) == (160, 224)
    return sh, model


def check_image_case(sh, model, title, name, ops, steps, forwards, suffix, trained=True):
    _report(sh, title, name)
    assert not sh.errors, sorted(set(sh.errors))
    sh.assert_ok(ops)
    assert max(_ratio_table(sh).values()) < 1.0
    assert_backbone_launches(sh, model, steps, forwards, suffix, trained)


def test_shadow_fp32_detector_step_from_images(monkeypatch):
    started = time.perf_counter()
    sh, model = image_steps(monkeypatch, 1, autocast=False)
    print(f"(d) under the harness: {time.perf_counter() - started:.1f} s")
    check_image_case(sh, model, "(d) fp32 detector step from three float images, R50 backbone, scipy matcher", "shadow_images_fp32.txt",
                     IMAGES_FP32_OPS, 1, 1, "_f32")
    assert "criterion.assign_match" not in sh.calls and not sh.launches["rdetr_assign_match"]
    assert not any(v for k, v in sh.launches.items() if k.endswith("_bf16"))


def test_shadow_mixed_precision_detector_two_steps_from_images(monkeypatch):
    started = time.perf_counter()
    sh, model = image_steps(monkeypatch, 2, autocast=True)
    print(f"(e) under the harness: {time.perf_counter() - started:.1f} s")
    check_image_case(sh, model, "(e) mixed-precision detector from three float images, R50 backbone, device matcher, two steps",
                     "shadow_images_mixed.txt", IMAGES_MIXED_OPS, 2, 2, "_bf16")
    assert sh.calls["criterion.assign_match"] == 2 * 3 and sh.calls["optim.FusedAdamW._step_fused"] == 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_shadow_eval_from_uint8_images(monkeypatch, dtype):
    from helpers import DETECTOR_BATCH, detector_uint8_images
    from test_gpu_backbone import deterministic_convolutions
    model = r50_model().eval().to(dtype)
    model.preprocessor.dtype = dtype
    images = [im.to(DEV) for im in detector_uint8_images()]
    assert model.preprocessor.takes_fused_route(images) and model.preprocessor.target_sizes(images) == [(150, 213), (56, 224), (150, 184)]
    frozen = {k: t.detach().clone() for k, t in model.state_dict().items()}
    sh = shadow.Shadow(monkeypatch)
    started, results = time.perf_counter(), []
    for channels_last in (False, True):
        model.preprocessor.channels_last = channels_last
        with torch.no_grad(), deterministic_convolutions():
            batch, _ = model.preprocessor(images)                                # one more forward of the front end: the layout it hands over
            assert tuple(batch.tensors.shape) == (3, 3) + tuple(DETECTOR_BATCH) and batch.tensors.dtype == dtype
            assert batch.tensors.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
            dets, tensor = model(images)
        torch.cuda.synchronize()
        assert tuple(tensor.shape) == (3, 10, 6) and bool(torch.isfinite(tensor).all()) and len(dets) == 3
        results.append(tensor)
    name = "fp32" if dtype == torch.float32 else "bf16"
    print(f"(f) {name} under the harness: {time.perf_counter() - started:.1f} s")
    _report(sh, f"(f) eval from three uint8 images, resized, R50 backbone, {name}, NCHW then channels-last", f"shadow_images_eval_{name}.txt")
    assert not sh.errors, sorted(set(sh.errors))
    sh.assert_ok(IMAGES_EVAL_OPS[name])
    assert max(_ratio_table(sh).values()) < 1.0
    fwd, _ = epilogue_counts(model.backbone)
    suffix = "_f32" if dtype == torch.float32 else "_bf16"
    assert sh.launches["rdetr_image_batch"] == 4 and sh.launches["rdetr_stem_pool" + suffix] == 2
    assert sh.launches["rdetr_frozen_bn_act" + suffix] == 2 * fwd == 104
    assert not sh.launches["rdetr_frozen_bn_act_backward_f32"] and not sh.launches["rdetr_frozen_bn_act_backward_bf16"]
    assert "backbones.epilogue.frozen_bn_act_backward" not in sh.calls
    moved = [k for k, t in model.state_dict().items() if not torch.equal(t.view(torch.uint8), frozen[k].view(torch.uint8))]
    assert not moved, moved


# the pinned op sets of these small shapes: S = 747 tokens and B S = 2,241 encoder rows, below S >= 4096 (the head-major value) and
# below 16,384 rows (the fused feed-forward kernels, whose mixed-precision training entries (a) holds: the library's GEMMs run here)
IMAGES_FP32_OPS = FP32_OPS | BACKBONE_TRAIN_OPS
IMAGES_MIXED_OPS = (MIXED_OPS - {"amp_train.ffn_mixed_train", "amp_train.ffn_mixed_backward"}) | BACKBONE_TRAIN_OPS
_EVAL_OPS = IMAGE_OPS | {"neck.group_norm_levels_forward", "neck._masks_and_counts", "neck._sine_pos_packed", "add_layer_norm",
                         "decoder_reference", "detections_from_topk", "ms_deform_attn_forward_fused", "pyramid_points", "row_max",
                         "tokens_from_levels", "topk", "zero_masked_rows_"}
IMAGES_EVAL_OPS = {"fp32": _EVAL_OPS | {"bias_softmax_", "box_refine", "relation_bias", "scaled_pos"},
                   "bf16": _EVAL_OPS | {"box_head_k256", "linear_ln_k256", "query_pos_k256", "relation_attention", "relation_attention_boxes"}}


def _bump_first(t):
    first = (0,) * t.dim()
    t[first] = torch.nextafter(t[first], t.new_tensor(1e30))                     # one ulp: the fp32 entries are exact


def _bump_output(name, call, args, result, fn):
    _bump_first(result)
    return result


def _bump_dx(name, call, args, result, fn):
    _bump_first(result[0])
    return result


def _flip_mask_pixel(name, call, args, result, fn):
    result.mask[0, 159, 223] = False                                            # a padded pixel no pyramid level samples
    return result


IMAGE_FAULTS = {"epilogue_output_element": ("backbones.epilogue.frozen_bn_act_forward", 17, _bump_output),
                "epilogue_dx_element": ("backbones.epilogue.frozen_bn_act_backward", 5, _bump_dx),
                "pooled_element": ("backbones.epilogue.stem_bn_relu_maxpool", 0, _bump_output),
                "mask_pixel": ("frontend.images.batch_images", 0, _flip_mask_pixel)}
DETECTOR_FAULTS.update(IMAGE_FAULTS)


@pytest.mark.parametrize("label", list(DETECTOR_FAULTS))
def test_shadow_detector_reports_injected_faults(monkeypatch, label):
    from test_gpu_shadow_stack import _injector
    op, call, fault = DETECTOR_FAULTS[label]
    if label in IMAGE_FAULTS:
        sh, _ = image_steps(monkeypatch, 1, autocast=False, fault=_injector(op, call, fault))
    else:
        sh, _, _ = tiny_step(monkeypatch, fault=_injector(op, call, fault))
    bad = [(r.op, r.call, r.failing) for r in sh.failures()]
    print(label, "->", [(r.op, r.call, round(r.ratio, 2), r.failing, r.where) for r in sh.failures()])
    assert not sh.errors, sorted(set(sh.errors))
    assert bad == [(op, call, 1)], (label, bad)
