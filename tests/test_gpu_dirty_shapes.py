"""The shadow harness (tests/shadow.py) at small ragged shapes, on poisoned scratch memory (tests/dirty.py).

Every case runs three times: with every uninitialised device allocation of the process filled with 0x00 (the control: a failure
here is a shape bug), with 0xFF (NaN as floats, -1 as integers) and with 0x42 (48.56 / 48.5 / 1,111,638,594: finite garbage that
fmaxf, ordered compares and counters do not swallow).  A failure on the dirty patterns alone is a result that depends on what the
memory held before: a partial that is added into and never cleared, a row of an output that is skipped and later read.  Every
launch runs inside a checked entry and every returned element is compared with the float64 reference at the bound of the kernel's
unit test (the table in tests/shadow.py).  No constant is new; two bounds that T1 exceeded on clean memory, pattern 0x00 as much as the
others, got the scale term their form lacked (shadow.boxes_lse_bound, shadow.attention_grad_rounding; profiles/r26/README.md).

Networks: ``build_relation_transformer(enc_layers=2, dec_layers=2)`` with ``synthetic_state_dict`` weights and, as
tests/test_gpu_shadow_detector.py explains, ``enc_output.bias`` left at zero; built anew for every case and pattern, so the
packed-weight caches are allocated under the pattern too.

Pyramids (S, the level starts and the query counts are multiples of no tile):
  A  (67,83) (34,42) (17,21) (9,11)          S =  7,445 = 5 mod 16, starts 0, 9, 13, 2 mod 16; levels 2 + 3 are 29,184 B a plane
  C  (75,100) (38,50) (19,25) (10,13) (5,7)  S = 10,040 = 8 mod 16, five levels: the query-run gather, never the resident one
  D  (25,43) (13,22) (7,11) (4,6)            S =  1,462 = 6 mod 16, below 4096: the [B,S,H,D] layout and every unfused fallback
  M  maps (61,99) (31,50) (16,25), the neck adds (8,13): S = 8,093 = 13 mod 16 (the detector step)
Padding: the last image right and bottom, as tests/test_gpu_shadow_stack.py::_padded_pyramid (with B = 1 that is the only image);
with B = 3 image 0 is unpadded and the middle image keeps two valid rows and one valid column of the coarsest level (and the same
share of the finer ones): valid ratios of 2/9 and 1/11, and fewer valid tokens than queries, so its two-stage selection takes
zeroed rows.

Eval forwards (no_grad, one image group, select_detections), the route each has to reach pinned by its launch counts:
  E1  A, B = 3, bf16, 300 queries   B S = 22,335: the resident gather once per encoder layer, the fused FFN, encoder_proj
  E2  A, B = 2, bf16, 301 queries   B S = 14,890 < 16,384, S >= 4096: the head-major query-run gather, the library-GEMM FFN, the
                                    short-row projection + LayerNorm kernel; the fused relation attention TAKES the 301 queries
                                    (its contract has no multiple-of-a-tile condition: one launch per decoder layer after the first,
                                    and no materialised relation bias)
  E3  C, B = 2, bf16, 300 queries   B S = 20,080, five levels: rdetr_msda_forward_fused_opt_bf16, no resident launch
  E4  D, B = 1, bf16 and fp32, 77 queries, 700 hybrid proposals (<= S): the [B,S,H,D] gather, the one-launch top-k with k = 77
  E5  A, B = 1, fp32, 300 queries   the _f32 entries in composition
Training steps:
  T1  the transformer-level step of test_shadow_all_training_routes_step on a .to(bfloat16) network with all six switches: A,
      B = 3, 2 x 13 denoising + 301 matching queries, with atomics and under torch.use_deterministic_algorithms(True); the only
      composition that reaches msda_train_head_major and rel_train_fused
  T2  the mixed-precision detector step of tests/test_gpu_shadow_detector.py, two steps: M, B = 3, 17 boxes / none / one, device matcher
  T3  its fp32 default step: the tiny model on three images of odd maps (13,21) (7,11) (4,6) + (2,3)
  T4  case (e) of tests/test_gpu_shadow_detector.py, one step: the reduced R50 detector from three float images under
      torch.autocast(bfloat16), the front end's batch and every epilogue output of the ResNet-50 (5 x 7 planes at layer4) allocated
      under the pattern; the routes pinned by the launch counts the module gives (52 epilogues, 42 backwards, one stem pool)

With ``RDETR_SHADOW_REPORTS=<directory>`` every case writes its report table there (profiles/r26/; T4: profiles/r28/).

Every case is a builder (``eval_case``, ``t1_case`` ... ``t4_case``) that takes ``install(monkeypatch, pattern)``, what prepares the
scratch memory before the harness stands, and the prefix of its report file: here ``dirty.poison``; tests/test_gpu_write_sets.py runs
the same builders on guarded allocations (tests/guard.py), where the poison must not be installed."""
import time

import pytest
import torch

import dirty
import shadow
from helpers import synthetic_state_dict
from test_gpu_shadow_detector import (IMAGES_MIXED_OPS, _write_report, check_image_case, fp32_step, image_steps, mixed_inputs,
                                      mixed_two_steps)
from test_gpu_shadow_stack import (EVAL_BF16_OPS, EVAL_FP32_OPS, TRAIN_SWITCHES, _dn_inputs, _eval_run, _loss, _ratio_table,
                                   assert_all_training_routes)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
PATTERNS = pytest.mark.parametrize("pattern", dirty.PATTERNS, ids=[f"0x{b:02X}" for b in dirty.PATTERNS])

A = [(67, 83), (34, 42), (17, 21), (9, 11)]
C = [(75, 100), (38, 50), (19, 25), (10, 13), (5, 7)]
D = [(25, 43), (13, 22), (7, 11), (4, 6)]
M = ((61, 99), (31, 50), (16, 25))
E_LAYERS = D_LAYERS = 2
HEAD_MAJOR = ("rdetr_encoder_proj_k256_bf16", "rdetr_linear_k256_hm_bf16", "rdetr_value_to_head_major_bf16")   # the producers of [B,H,S,D]
RESIDENT, QUERY_RUN = "rdetr_msda_forward_fused_resident_bf16", "rdetr_msda_forward_fused_opt_bf16"


def test_the_pyramids_are_ragged():
    from relation_detr_amd.ops import _resident_pays
    for shapes, S, mod in ((A, 7445, 5), (C, 10040, 8), (D, 1462, 6), (list(M) + [(8, 13)], 8093, 13)):
        sizes = [h * w for h, w in shapes]
        assert sum(sizes) == S and S % 16 == mod
    assert [sum(h * w for h, w in A[:l]) % 16 for l in range(4)] == [0, 9, 13, 2]
    assert sum(h * w for h, w in A[2:]) * 64 == 29184
    assert _resident_pays(3, 7445, 4, A) and not _resident_pays(2, 7445, 4, A) and not _resident_pays(2, 10040, 5, C)
    assert 2 * 7445 < 16384 <= 3 * 7445 and 7445 >= 4096 > 1462 and 2 * 10040 >= 16384 and 3 * 8093 >= 16384


def network(queries, levels=4, hybrid=1500, dtype=BF16):
    from relation_detr_amd.transformer import build_relation_transformer
    net = build_relation_transformer(num_classes=91, enc_layers=E_LAYERS, dec_layers=D_LAYERS, num_queries=queries,
                                     hybrid_num_proposals=hybrid, num_levels=levels)
    net.load_state_dict(synthetic_state_dict(net.state_dict()))
    with torch.no_grad():
        net.enc_output.bias.zero_()                               # tests/test_gpu_shadow_detector.py::mixed_model has why
    return net.to(DEV).to(dtype)


def ragged_pyramid(batch, shapes, dtype, seed=11):
    """bench.build_pyramid with the padding of the module docstring."""
    import bench
    feats, masks, pos = bench.build_pyramid(batch, DEV, seed, dtype=dtype, shapes=shapes)
    hc, wc = shapes[-1]
    for m in masks:
        h, w = m.shape[1:]
        m[-1, :, max(1, w * 7 // 8):] = True
        m[-1, max(1, h * 9 // 10):, :] = True
        for b in range(1, batch - 1):
            m[b, max(1, 2 * h // hc):, :] = True
            m[b, :, max(1, w // wc):] = True
    if batch == 3:
        assert int((~masks[-1][1]).sum()) == 2 and not masks[0][0].any()
    return feats, masks, pos


def finish(sh, poison, title, name, started, prefix="dirty"):
    """The end of every case: the report, then no error, no failing record, every ratio below 1."""
    torch.cuda.synchronize()
    wall = time.perf_counter() - started
    text = sh.report(f"{title}; scratch memory 0x{poison.byte:02X} ({poison.fills} allocations, {poison.bytes / 2 ** 20:.1f} MiB filled); "
                     f"{wall:.2f} s under the harness")
    print("C launches: " + ", ".join(f"{k} x{v}" for k, v in sorted(sh.launches.items())))
    _write_report(f"{prefix}_{name}_0x{poison.byte:02X}.txt", text, sh)
    assert poison.fills > 0, "the poison saw no allocation"
    assert not sh.errors, sorted(set(sh.errors))


def eval_case(monkeypatch, pattern, name, shapes, batch, dtype, queries, hybrid=1500, install=dirty.poison, prefix="dirty"):
    net = network(queries, len(shapes), hybrid, dtype).eval()
    feats, masks, pos = ragged_pyramid(batch, shapes, dtype)
    poison = install(monkeypatch, pattern)
    sh = shadow.Shadow(monkeypatch)
    started = time.perf_counter()
    det = _eval_run(net, feats, masks, pos, groups=1)
    dtype_name = "bf16" if dtype == BF16 else "fp32"
    finish(sh, poison, f"{name}: eval, {dtype_name}, B = {batch}, {queries} queries, levels {shapes}", f"{name}_{dtype_name}", started, prefix)
    assert det.shape == (batch, 300, 6) and bool(torch.isfinite(det).all())
    sh.assert_ok(EVAL_BF16_OPS_SMALL[name] if dtype == BF16 else EVAL_FP32_OPS)
    assert not sh.errors and max(_ratio_table(sh).values()) < 1.0
    return sh


# the op sets of the bf16 eval cases: tests/test_gpu_shadow_stack.py's EVAL_BF16_OPS where every tall route applies (E1, E3); below
# 16,384 encoder rows the feed-forward block is two library GEMMs (no ffn_k256); below S = 4096 the value is not head-major (no
# encoder_proj: the library projections, the fill pass and add_layer_norm instead of linear_ln_k256 on the encoder's rows)
EVAL_BF16_OPS_SMALL = {"E1": EVAL_BF16_OPS, "E3": EVAL_BF16_OPS, "E2": EVAL_BF16_OPS - {"ffn_k256"},
                       "E4": (EVAL_BF16_OPS - {"ffn_k256", "encoder_proj"}) | {"zero_masked_rows_"}}


def e1_case(monkeypatch, pattern, **how):
    sh = eval_case(monkeypatch, pattern, "E1", A, 3, BF16, 300, **how)
    assert sh.launches[RESIDENT] == E_LAYERS and sh.launches["rdetr_ffn_k256_bf16"] == E_LAYERS
    assert sh.launches["rdetr_encoder_proj_k256_bf16"] == E_LAYERS
    return sh


@PATTERNS
def test_e1_resident_gather_odd_batch(monkeypatch, pattern):
    e1_case(monkeypatch, pattern)


def e2_case(monkeypatch, pattern, **how):
    sh = eval_case(monkeypatch, pattern, "E2", A, 2, BF16, 301, **how)
    assert not sh.launches[RESIDENT] and sh.launches[QUERY_RUN] >= E_LAYERS
    assert sum(sh.launches[s] for s in HEAD_MAJOR) == E_LAYERS                               # S >= 4096: the head-major value
    assert not sh.launches["rdetr_ffn_k256_bf16"] and not sh.launches["rdetr_ffn_ln_k256_bf16"]   # the library GEMMs
    assert sh.launches["rdetr_linear_ln_rows_bf16"] > 0 and not sh.launches["rdetr_linear_ln_k256_bf16"]
    # the fused relation attention took 301 queries: one launch per decoder layer after the first, no materialised bias
    assert sh.launches["rdetr_relation_attention_boxes_bf16"] == D_LAYERS - 1 and sh.launches["rdetr_relation_attention_bf16"] == 1
    assert not sh.launches["rdetr_relation_bias_ws_f32"] and not sh.launches["rdetr_relation_bias_f32"]
    assert not sh.launches["rdetr_bias_softmax_f32"]
    return sh


@PATTERNS
def test_e2_below_the_row_threshold_301_queries(monkeypatch, pattern):
    e2_case(monkeypatch, pattern)


def e3_case(monkeypatch, pattern, **how):
    sh = eval_case(monkeypatch, pattern, "E3", C, 2, BF16, 300, **how)
    assert sh.launches[QUERY_RUN] >= E_LAYERS and not sh.launches[RESIDENT]
    assert sh.launches["rdetr_ffn_k256_bf16"] == E_LAYERS
    return sh


@PATTERNS
def test_e3_five_levels(monkeypatch, pattern):
    e3_case(monkeypatch, pattern)


def e4_case(monkeypatch, pattern, dtype, **how):
    sh = eval_case(monkeypatch, pattern, "E4", D, 1, dtype, 77, hybrid=700, **how)
    assert not any(sh.launches[s] for s in HEAD_MAJOR) and not sh.launches[RESIDENT]          # S < 4096: [B,S,H,D]
    assert sh.launches["rdetr_topk"] == 2                        # 77 of 1,462 proposals, 300 of 77 x 91 scores: one launch each
    gathers = [s for s in sh.launches if s.startswith("rdetr_msda_forward_fused") and s.endswith("_bf16" if dtype == BF16 else "_f32")]
    assert sum(sh.launches[s] for s in gathers) == E_LAYERS + D_LAYERS
    return sh


@PATTERNS
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_e4_short_pyramid_77_queries(monkeypatch, pattern, dtype):
    e4_case(monkeypatch, pattern, dtype)


def e5_case(monkeypatch, pattern, **how):
    sh = eval_case(monkeypatch, pattern, "E5", A, 1, F32, 300, **how)
    assert sh.launches["rdetr_msda_forward_fused_f32"] + sh.launches["rdetr_msda_forward_fused_ex_f32"] == E_LAYERS + D_LAYERS
    assert sh.launches["rdetr_bias_softmax_f32"] == D_LAYERS and sh.launches["rdetr_relation_bias_ws_f32"] == D_LAYERS - 1
    assert not any(v for k, v in sh.launches.items() if k.endswith("_bf16"))
    return sh


@PATTERNS
def test_e5_fp32_entries(monkeypatch, pattern):
    e5_case(monkeypatch, pattern)


# ------------------------------------------------------------------------------------------------------------- training steps
def t1_case(monkeypatch, pattern, deterministic, install=dirty.poison, prefix="dirty"):
    from relation_detr_amd import options
    batch, groups, per_group, queries = 3, 2, 13, 301
    net = options.apply(network(queries).train(), **dict.fromkeys(TRAIN_SWITCHES, True))
    feats, masks, pos = ragged_pyramid(batch, A, BF16)
    label, box, mask = _dn_inputs(batch, groups, per_group, queries, torch.Generator().manual_seed(5))
    assert (groups * per_group + queries) % 8 and (groups * per_group + queries) % 16
    poison = install(monkeypatch, pattern)
    sh = shadow.Shadow(monkeypatch)
    was, started = torch.are_deterministic_algorithms_enabled(), time.perf_counter()
    try:
        torch.use_deterministic_algorithms(deterministic)
        with torch.enable_grad():
            _loss(net(feats, masks, pos, label.to(DEV, BF16), box.to(DEV), mask.to(DEV))).backward()
    finally:
        torch.use_deterministic_algorithms(was)
    mode = "deterministic" if deterministic else "atomic"
    finish(sh, poison, f"T1: bf16 training step, all six switches ({mode}), A, B = 3, 26 denoising + 301 matching queries", f"T1_{mode}", started, prefix)
    assert_all_training_routes(sh, net)
    assert sh.launches["rdetr_msda_backward_fused_hm_bf16"] == E_LAYERS                      # msda_train_head_major
    assert sh.launches["rdetr_relation_attention_boxes_train_bf16"] == sh.launches["rdetr_relation_attention_boxes_backward_bf16"] == D_LAYERS - 1
    return sh


@PATTERNS
@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "deterministic"])
def test_t1_all_training_routes(monkeypatch, pattern, deterministic):
    t1_case(monkeypatch, pattern, deterministic)


def t2_case(monkeypatch, pattern, install=dirty.poison, prefix="dirty"):
    inputs = mixed_inputs(batch=3, maps=M, counts=(17, 0, 1), hard=(1,))
    rows, cols = torch.arange(8, device=DEV) * 488 // 8, torch.arange(13, device=DEV) * 792 // 13
    assert int((~inputs[1][1][rows][:, cols]).sum()) == 2            # the coarsest level's view of the middle image: 2 x 1 valid pixels
    poison = install(monkeypatch, pattern)
    mixed_two_steps(monkeypatch, inputs, M, f"T2: mixed-precision detector, two steps, M, B = 3, boxes 17 / 0 / 1; scratch memory 0x{pattern:02X}",
                    f"{prefix}_T2_0x{pattern:02X}.txt")
    assert poison.fills > 0


@PATTERNS
def test_t2_mixed_precision_detector_two_steps(monkeypatch, pattern):
    t2_case(monkeypatch, pattern)


def t3_case(monkeypatch, pattern, install=dirty.poison, prefix="dirty"):
    g = torch.Generator().manual_seed(29)
    maps = ((13, 21), (7, 11), (4, 6))
    feats = [torch.randn(3, c, h, w, generator=g).to(DEV) for c, (h, w) in zip((16, 24, 40), maps)]
    mask = torch.zeros(3, 104, 168)
    mask[2, :, 147:] = 1.0                                       # the last image: right and bottom
    mask[2, 91:, :] = 1.0
    mask[1, :, 56:] = 1.0                                        # the middle image: one valid column of the coarsest level (2, 3), whose
                                                                 # two rows are all it has
    counts = (3, 0, 4)
    targets = [{"labels": torch.randint(0, 11, (n,), generator=g).to(DEV),
                "boxes": torch.cat((0.15 + 0.7 * torch.rand(n, 2, generator=g), 0.05 + 0.25 * torch.rand(n, 2, generator=g)), -1).to(DEV)}
               for n in counts]
    poison = install(monkeypatch, pattern)
    fp32_step(monkeypatch, (feats, mask.to(DEV), targets), f"T3: fp32 detector step, three images, maps {maps}; scratch memory 0x{pattern:02X}",
              f"{prefix}_T3_0x{pattern:02X}.txt")
    assert poison.fills > 0


@PATTERNS
def test_t3_fp32_detector_step(monkeypatch, pattern):
    t3_case(monkeypatch, pattern)


def t4_case(monkeypatch, pattern, install=dirty.poison, prefix="dirty"):
    poison = install(monkeypatch, pattern)
    started = time.perf_counter()
    sh, model = image_steps(monkeypatch, 1, autocast=True)
    print(f"T4 under the harness: {time.perf_counter() - started:.1f} s")
    check_image_case(sh, model, f"T4: mixed-precision detector step from three float images, R50 backbone; scratch memory 0x{pattern:02X}",
                     f"{prefix}_T4_0x{pattern:02X}.txt", IMAGES_MIXED_OPS, 1, 1, "_bf16")
    assert poison.fills > 0


@PATTERNS
def test_t4_mixed_precision_detector_step_from_images(monkeypatch, pattern):
    t4_case(monkeypatch, pattern)
