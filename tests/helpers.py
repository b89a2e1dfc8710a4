"""Shared helpers for the parity tests (synthetic inputs, kink masks)."""
import numpy as np
import torch


def pyramid(shapes):
    shapes = torch.tensor(shapes, dtype=torch.int64)
    areas = shapes[:, 0] * shapes[:, 1]
    start = torch.cat([areas.new_zeros(1), areas.cumsum(0)[:-1]])
    return shapes, start, int(areas.sum())


def kink_mask(loc: np.ndarray, shapes: np.ndarray, tol: float = 1e-3) -> np.ndarray:
    """True where d(out)/d(loc) is well defined: bilinear interpolation is only piecewise
    differentiable, with kinks where the pixel coordinate loc*size-0.5 is an integer.  There the
    one-sided derivative an implementation returns depends on how it rounds the coordinate (the
    reference's grid_sample path computes ((2*loc-1)+1)*size/2-0.5, the CUDA op loc*size-0.5), so
    those measure-zero points are excluded from grad_loc comparisons.  Shape = loc.shape."""
    L = shapes.shape[0]
    size = np.stack([shapes[:, 1], shapes[:, 0]], -1).astype(np.float64)          # (w, h) per level
    pix = loc.astype(np.float64) * size.reshape(1, 1, 1, L, 1, 2) - 0.5
    return np.abs(pix - np.round(pix)) > tol


def make_msda_inputs(B, Nq, shapes, H=8, D=32, P=4, seed=0, spread=0.15, dtype=torch.float32):
    """Seeded value / locations / weights for a given pyramid; locations ~ U(-spread, 1+spread)."""
    g = torch.Generator().manual_seed(seed)
    shapes_t, start, S = pyramid(shapes)
    L = shapes_t.shape[0]
    value = torch.randn(B, S, H, D, generator=g, dtype=dtype)
    loc = torch.rand(B, Nq, H, L, P, 2, generator=g) * (1 + 2 * spread) - spread
    attn = torch.softmax(torch.randn(B, Nq, H, L * P, generator=g), -1).view(B, Nq, H, L, P)
    return value, shapes_t, start, loc, attn


def synthetic_state_dict(reference_state_dict):
    """Deterministic, RNG-free parameter values for a transformer state_dict (name -> tensor), so that the
    reference model (in oracle/gen_golden.py) and the harness under test can be loaded with IDENTICAL weights
    without committing tens of MB of tensors: value = f(parameter name, flat index)."""
    import zlib
    out = {}
    for name, ref in reference_state_dict.items():
        n = ref.numel()
        idx = np.arange(n, dtype=np.float64)
        phase = (zlib.crc32(name.encode()) % 1000) / 1000.0 * 6.283185307179586
        if "norm" in name and name.endswith("weight"):
            v = 1.0 + 0.1 * np.sin(idx * 0.37 + phase)
        elif name.endswith("sampling_offsets.bias"):
            v = 2.0 * np.sin(idx * 0.77 + phase)                                  # offsets of a few pixels
        elif name.endswith("bias"):
            v = 0.05 * np.sin(idx * 0.91 + phase)
        elif ref.dim() >= 2 and "embed" not in name:
            fan_in = int(np.prod(ref.shape[1:]))
            v = np.sin(idx * 0.7071 + phase) * np.sqrt(3.0 / fan_in)
        else:                                                                      # embeddings, level_embeds
            v = 0.7 * np.sin(idx * 0.613 + phase)
        out[name] = torch.from_numpy(v.astype(np.float32)).reshape(ref.shape)
    return out


def functional_weights(shape, i: int) -> torch.Tensor:
    """RNG-free weights of the linear functional g8 differentiates: loss = sum_i <out_i, functional_weights(out_i.shape, i)>
    (shared by oracle/gen_golden.py and the tests, so the fixture need not store them)."""
    n = int(np.prod(shape))
    return torch.from_numpy(np.cos(np.arange(n, dtype=np.float64) * 0.37 + i).astype(np.float32)).reshape(tuple(shape))


# parameters whose full gradients g8 stores (all others: their L2 norms)
G8_FULL_GRADS = ("level_embeds", "tgt_embed.weight", "hybrid_tgt_embed.weight",
                 "decoder.position_relation_embedding.pos_proj.0.weight", "decoder.position_relation_embedding.pos_proj.0.bias",
                 "encoder.layers.0.self_attn.sampling_offsets.bias", "encoder.layers.1.self_attn.attention_weights.bias",
                 "decoder.layers.1.self_attn.in_proj_bias", "decoder.layers.2.cross_attn.sampling_offsets.bias",
                 "decoder.bbox_head.0.layers.2.bias", "hybrid_class_head.bias", "encoder_class_head.bias")


# the optimizer checker of tests/test_gpu_optim.py and of the shadow harness (tests/shadow.py): one copy
def snapshot(opt):
    """The optimizer's tensors before a step, in group order: per parameter (p, m, v, step, grad), clones on the device."""
    rows = []
    for group in opt.param_groups:
        for p in group["params"]:
            s = opt.state.get(p) or {}
            rows.append(dict(p=p.detach().clone(), m=s["exp_avg"].clone() if s else None, v=s["exp_avg_sq"].clone() if s else None,
                             step=float(s["step"]) if s else 0.0, g=None if p.grad is None else p.grad.detach().clone(),
                             requires_grad=p.requires_grad))
    return rows


def torch_route_step(opt, rows, max_norm, dtype):
    """One clip + step of the torch route in ``dtype`` from ``rows`` under ``opt``'s current group settings ->
    (norm, per parameter (p, m, v, scaled gradient))."""
    from relation_detr_amd.optim import FusedAdamW
    groups, params, i = [], [], 0
    for group in opt.param_groups:
        mine = []
        for _ in group["params"]:
            q = torch.nn.Parameter(rows[i]["p"].to(dtype, copy=True), requires_grad=rows[i]["requires_grad"])
            q.grad = None if rows[i]["g"] is None else rows[i]["g"].to(dtype, copy=True).contiguous()
            mine.append(q)
            i += 1
        params += mine
        groups.append({"params": mine, **{k: group[k] for k in ("lr", "betas", "eps", "weight_decay")}})
    route = FusedAdamW(groups, fused=False)
    for q, row in zip(params, rows):
        if row["m"] is not None:
            route.state[q] = {"step": torch.tensor(row["step"], dtype=torch.float32), "exp_avg": row["m"].to(dtype, copy=True),
                              "exp_avg_sq": row["v"].to(dtype, copy=True)}
    norm = route.clip_grad_norm_(max_norm) if max_norm is not None else None
    route.step()
    out = []
    for q in params:
        s = route.state.get(q) or {}
        out.append((q.detach(), s.get("exp_avg"), s.get("exp_avg_sq"), q.grad))
    return norm, out


# the backbone epilogues' references and bounds (tests/test_gpu_backbone.py and the shadow harness, tests/shadow.py): one copy
def torch_bn_act(x, s, h, r, relu):
    """The reference's passes, one operator each."""
    y = x * s.reshape(1, -1, 1, 1)
    y = y + h.reshape(1, -1, 1, 1)
    if r is not None:
        y = y + r
    return torch.relu(y) if relu else y


def torch_stem(x, s, h):
    return torch.nn.functional.max_pool2d(torch.relu(x * s.reshape(1, -1, 1, 1) + h.reshape(1, -1, 1, 1)), 3, 2, 1)


def bf16_slack(x, s, h, r):
    s4, h4 = s.double().reshape(1, -1, 1, 1), h.double().reshape(1, -1, 1, 1)
    return 2.0 ** -20 * ((x.double() * s4).abs() + h4.abs() + (r.double().abs() if r is not None else 0.0))


# the images of the detector steps that start at the front end (tests/test_gpu_shadow_detector.py (d), (e), (f), tests/test_gpu_dirty_shapes.py
# T4); tests/test_shadow_train_host.py checks on the CPU that the uint8 batch is well-posed under the near-tie rule
DETECTOR_BATCH = (160, 224)                       # the padded batch: stem 80 x 112, pool 40 x 56, stages 20 x 28, 10 x 14, 5 x 7, extra level 3 x 4
DETECTOR_FLOAT_SIZES = ((160, 200), (131, 224), (50, 70))          # the last: 3,500 of 35,840 pixels, the rest padding
DETECTOR_UINT8_SIZES = ((211, 300), (100, 400), (333, 410))        # resized to (150, 213), (56, 224), (150, 184) by min_size / max_size
DETECTOR_RESIZE = (150, 224)                      # ImagePreprocessor's min_size, max_size for the uint8 images


def detector_float_images():
    """Three augmented-and-normalised training images, CPU float32."""
    g = torch.Generator().manual_seed(61)
    return [torch.randn(3, h, w, generator=g) for h, w in DETECTOR_FLOAT_SIZES]


def detector_uint8_images():
    """Three eval images of ragged sizes, CPU uint8."""
    g = torch.Generator().manual_seed(62)
    return [torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g) for h, w in DETECTOR_UINT8_SIZES]
