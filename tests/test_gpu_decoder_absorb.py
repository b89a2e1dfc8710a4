"""GPU tests of the two GEMM absorptions on the decoder's chain: the self-attention in-projection inside the query-position kernel
(rdetr_query_pos_inproj_k256_bf16, csrc/qpos.hip) and the class head inside the box-head kernel (rdetr_box_head_cls_k256_bf16,
csrc/mlp.hip).

  * the outputs the kernels had before (query_pos, query + query_pos; the boxes) are bit for bit those of the call without the new
    keyword argument;
  * the new outputs lie within 2^-8 |ref| + 2e-3 of the float64 product of the bf16 operands plus bias -- the project's bound
    for a K = 256 bf16 projection (tests/shadow.py chk_encoder_proj / chk_linear_k256) -- qk taken from the bf16 sum the kernel returns;
  * nothing is written outside the destination's rows and columns (guard-filled destinations);
  * a 2-layer decoder through the new route against the same decoder with the keyword arguments stripped (the library GEMMs),
    both measured against the fp32 CPU oracle of the same module;
  * HIP-graph replay equals the eager launch, and the decoder_tail / box_head switches still give the library route."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
QPOS_ROWS = (1, 16, 17, 33, (2, 300))                  # a single row, one exact block, a block seam, a ragged last workgroup
BOX_ROWS = (1, 31, 32, 33, (2, 300))
CLASSES = (1, 8, 91, 96, 250)
GUARD = -7.0                                           # exactly representable in bf16; no logit or projection of these inputs equals it


def make_qpos_mlps():
    from relation_detr_amd.transformer import MLP
    torch.manual_seed(7)
    head = MLP(512, 256, 256, 2).to(DEV).to(BF)
    scale = MLP(256, 256, 256, 2).to(DEV).to(BF)
    with torch.no_grad():
        for l in (*head.layers, *scale.layers):
            l.bias.copy_(torch.randn(256) * 0.1)
    return head, scale


def make_in_proj():
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(768, 256, generator=g) * 0.06).to(BF).to(DEV)           # xavier_uniform of [768, 256] has std 0.044
    b = (torch.randn(768, generator=g) * 0.1).to(BF).to(DEV)
    return w, b


def make_box_head():
    from relation_detr_amd.transformer import MLP
    torch.manual_seed(5)
    head = MLP(256, 256, 4, 3).to(DEV).to(BF)
    with torch.no_grad():
        head.layers[2].weight.copy_(torch.randn(4, 256) * 0.05)
        head.layers[2].bias.copy_(torch.randn(4) * 0.1)
        for l in head.layers[:2]:
            l.bias.copy_(torch.randn(256) * 0.1)
    return head


def make_class_head(C):
    torch.manual_seed(20 + C)
    lin = torch.nn.Linear(256, C).to(DEV).to(BF)
    with torch.no_grad():
        lin.bias.copy_(torch.randn(C) * 0.5)
    return lin


def lead(rows):
    return rows if isinstance(rows, tuple) else (rows,)


def assert_projection(name, got, x, w, b):
    """|got - (x w^T + b in float64)| <= 2^-8 |ref| + 2e-3, every element"""
    ref = x.double() @ w.double().t() + b.double()
    err = (got.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2e-3
    print(f"{name} {tuple(got.shape)}: max err {err.max().item():.3e}, worst err / bound {(err / bound).max().item():.3f}")
    assert got.dtype == BF and (err <= bound).all()


# --------------------------------------------------------------------------------------------------- query position + in-projection
@pytest.mark.parametrize("rows", QPOS_ROWS)
@pytest.mark.parametrize("scaled", [False, True])
def test_query_pos_with_in_projection(rows, scaled):
    from relation_detr_amd import ops
    head, scale = make_qpos_mlps()
    w, b = make_in_proj()
    g = torch.Generator().manual_seed(300 + sum(lead(rows)))
    emb = torch.randn(*lead(rows), 512, generator=g).to(BF).to(DEV)
    query = torch.randn(*lead(rows), 256, generator=g).to(BF).to(DEV)
    sc = scale.layers if scaled else None
    pos0, qpp0 = ops.query_pos_k256(emb, query, head.layers, sc)
    d = {"weight": w, "bias": b}
    pos, qpp = ops.query_pos_k256(emb, query, head.layers, sc, in_proj=d)
    assert torch.equal(pos, pos0) and torch.equal(qpp, qpp0)
    qk, v = d["qk"], d["v"]
    assert tuple(qk.shape) == (*lead(rows), 512) and tuple(v.shape) == (*lead(rows), 256)
    assert_projection("qk", qk, qpp, w[:512], b[:512])                       # from the bf16 sum the kernel returns
    assert_projection("v", v, query, w[512:], b[512:])


@pytest.mark.parametrize("scaled", [False, True])
def test_query_pos_with_in_projection_strided_operands_and_destinations(scaled):
    """emb / query as column slices of wider buffers, qk / v destinations whose row stride exceeds their width (guard-filled: the
    kernel writes its columns and rows only), and layer 0's stride-0 query (tgt_embed.weight.expand(B, -1, -1))."""
    from relation_detr_amd import ops
    head, scale = make_qpos_mlps()
    w, b = make_in_proj()
    sc = scale.layers if scaled else None
    g = torch.Generator().manual_seed(41)
    B, N = 2, 37
    wide_e = torch.randn(B, N, 512 + 64, generator=g).to(BF).to(DEV)
    wide_q = torch.randn(B, N, 256 + 32, generator=g).to(BF).to(DEV)
    emb, query = wide_e[..., 64:], wide_q[..., 16:272]
    buf_qk = torch.full((B, N, 512 + 24), GUARD, dtype=BF, device=DEV)
    buf_v = torch.full((B, N, 256 + 8), GUARD, dtype=BF, device=DEV)
    d = {"weight": w, "bias": b, "qk": buf_qk[..., 8:520], "v": buf_v[..., :256]}
    pos, qpp = ops.query_pos_k256(emb, query, head.layers, sc, in_proj=d)
    pos0, qpp0 = ops.query_pos_k256(emb.contiguous(), query.contiguous(), head.layers, sc)
    assert torch.equal(pos, pos0) and torch.equal(qpp, qpp0)
    assert d["qk"].data_ptr() == buf_qk[..., 8:520].data_ptr() and d["v"].data_ptr() == buf_v.data_ptr()
    assert_projection("qk", buf_qk[..., 8:520], qpp, w[:512], b[:512])
    assert_projection("v", buf_v[..., :256], query, w[512:], b[512:])
    assert (buf_qk[..., :8] == GUARD).all() and (buf_qk[..., 520:] == GUARD).all() and (buf_v[..., 256:] == GUARD).all()
    c = {"weight": w, "bias": b}
    ops.query_pos_k256(emb.contiguous(), query.contiguous(), head.layers, sc, in_proj=c)
    assert torch.equal(c["qk"], buf_qk[..., 8:520]) and torch.equal(c["v"], buf_v[..., :256])       # strides change no bit
    # layer 0: one content query for every image
    q0 = torch.randn(N, 256, generator=g).to(BF).to(DEV).expand(B, -1, -1)
    assert q0.stride(0) == 0
    e = {"weight": w, "bias": b}
    pos, qpp = ops.query_pos_k256(emb, q0, head.layers, None, in_proj=e)
    assert torch.equal(qpp, (q0.float() + pos.float()).to(BF))
    assert_projection("qk (stride-0 query)", e["qk"], qpp, w[:512], b[:512])
    assert_projection("v (stride-0 query)", e["v"], q0, w[512:], b[512:])


def test_query_pos_in_projection_refuses_bad_arguments():
    from relation_detr_amd import _lib, ops
    head, _ = make_qpos_mlps()
    w, b = make_in_proj()
    emb = torch.zeros(4, 512, dtype=BF, device=DEV)
    query = torch.zeros(4, 256, dtype=BF, device=DEV)
    for bad in ({"weight": w[:512], "bias": b}, {"weight": w.float(), "bias": b}, {"weight": w, "bias": b[:512]}, {"weight": w},
                {"weight": w, "bias": b, "qk": torch.zeros(4, 256, dtype=BF, device=DEV)},
                {"weight": w, "bias": b, "v": torch.zeros(4, 256, device=DEV)},
                {"weight": w, "bias": b, "v": torch.zeros(4, 260, dtype=BF, device=DEV)[:, 4:]}):      # rows not 16-byte aligned
        with pytest.raises(_lib.RdetrError, match="in_proj"):
            ops.query_pos_k256(emb, query, head.layers, None, in_proj=bad)


# ------------------------------------------------------------------------------------------------------------ box head + class head
@pytest.mark.parametrize("rows", BOX_ROWS)
@pytest.mark.parametrize("C", CLASSES)
def test_box_head_with_class_head(rows, C):
    from relation_detr_amd import ops
    head, lin = make_box_head(), make_class_head(C)
    g = torch.Generator().manual_seed(500 + sum(lead(rows)) + C)
    xa = torch.randn(*lead(rows), 256, generator=g).to(BF).to(DEV)
    xb = torch.randn(*lead(rows), 256, generator=g).to(BF).to(DEV)
    ref = torch.rand(*lead(rows), 4, generator=g).to(DEV)
    logit = torch.log(ref.clamp(1e-3, 1 - 1e-3) / (1 - ref.clamp(1e-3, 1 - 1e-3)))
    M = xa.numel() // 256
    # two inputs (a decoder layer), one input (the last layer), one input with the reference as a logit (the two-stage form)
    for name, second, r, kw in (("two inputs", xb, ref, {}), ("one input", None, ref, {}),
                                ("two-stage form", None, logit, {"reference_is_logit": True})):
        want = ops.box_head_k256(xa, second, head.layers, r, **kw)
        buf = torch.full((M + 3, C + 5), GUARD, dtype=BF, device=DEV)        # guard rows below, guard columns right of the logits
        out = buf[:M, :C] if len(lead(rows)) == 1 else buf[:M].view(*lead(rows), C + 5)[..., :C]
        d = {"linear": lin, "out": out}
        got = ops.box_head_k256(xa, second, head.layers, r, class_head=d, **kw)
        if second is None:
            assert torch.equal(got, want)
        else:
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert d["out"] is out
        assert_projection(f"logits ({name}, C = {C})", out, xa, lin.weight, lin.bias)
        assert (buf[:M, C:] == GUARD).all() and (buf[M:] == GUARD).all()
    d = {"linear": lin}
    ops.box_head_k256(xa, xb, head.layers, ref, class_head=d)
    assert tuple(d["out"].shape) == (*lead(rows), C) and torch.equal(d["out"], out)      # an allocated destination: the same bits


def test_box_head_class_head_refuses_bad_arguments():
    from relation_detr_amd import _lib, ops
    head = make_box_head()
    xa = torch.zeros(4, 256, dtype=BF, device=DEV)
    ref = torch.full((4, 4), 0.5, device=DEV)
    lin = make_class_head(8)
    for bad in ({"linear": torch.nn.Linear(256, 8).to(DEV)}, {"linear": torch.nn.Linear(128, 8).to(DEV).to(BF)},
                {"linear": torch.nn.Linear(256, 300).to(DEV).to(BF)}, {"linear": torch.nn.Linear(256, 8, bias=False).to(DEV).to(BF)}, {},
                {"linear": lin, "out": torch.zeros(4, 9, dtype=BF, device=DEV)}, {"linear": lin, "out": torch.zeros(4, 8, device=DEV)}):
        with pytest.raises(_lib.RdetrError, match="class_head"):
            ops.box_head_k256(xa, None, head.layers, ref, class_head=bad)


# --------------------------------------------------------------------------------------------------------------------- decoder level
SHAPES = ((16, 20), (8, 10), (4, 5), (2, 3))
FLOOR = 5e-4        # the fp32 harness against the CPU oracle (tests/test_gpu_fullsize.py, test_transformer_harness.py)


def _decoder_case():
    from oracle.cpu_modules import OracleMSDA, OracleRelation, OracleSelfAttention
    from relation_detr_amd.transformer import build_relation_transformer
    kw = dict(num_classes=91, d_ffn=256, enc_layers=1, dec_layers=2, num_queries=300, hybrid_num_proposals=8)
    torch.manual_seed(0)
    cpu = build_relation_transformer(msda_cls=OracleMSDA, self_attn_cls=OracleSelfAttention, relation_cls=OracleRelation, **kw).eval()
    with torch.no_grad():
        for h in cpu.decoder.bbox_head:                                       # the reference initialises the last layer with zeros
            h.layers[-1].weight.copy_(torch.randn(4, 256) * 0.02)
        for l in cpu.decoder.layers:
            l.self_attn.in_proj_bias.copy_(torch.randn(768) * 0.1)
        sd = {k: v.to(BF).float() for k, v in cpu.state_dict().items()}      # both sides hold the bf16 values
    cpu.load_state_dict(sd)
    gpu = build_relation_transformer(**kw).eval()
    gpu.load_state_dict(sd)
    gpu = gpu.to(DEV).to(BF)
    g = torch.Generator().manual_seed(9)
    B, N = 2, 300
    S = sum(h * w for h, w in SHAPES)
    shapes = torch.tensor(SHAPES, dtype=torch.int64)
    start = torch.cat([shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]])
    inputs = dict(query=torch.randn(B, N, 256, generator=g).to(BF).float(), value=torch.randn(B, S, 256, generator=g).to(BF).float(),
                  reference_points=torch.cat([torch.rand(B, N, 2, generator=g) * 0.8 + 0.1, torch.rand(B, N, 2, generator=g) * 0.3 + 0.05], -1),
                  spatial_shapes=shapes, level_start_index=start, valid_ratios=torch.ones(B, len(SHAPES), 2))
    return cpu, gpu, inputs


def test_decoder_through_the_absorbed_route_against_the_library_route(monkeypatch):
    """The bound is relative to the route this replaces: both routes' worst errors against the fp32 CPU oracle of the same module
    (the bf16 values of the same weights and inputs), new <= 1.25 x library + the fp32 harness's own 5e-4 against that oracle."""
    from relation_detr_amd import ops
    cpu, gpu, inputs = _decoder_case()
    with torch.no_grad():
        want_cls, want_box = cpu.decoder(**inputs)
    dev_in = {k: (v.to(DEV).to(BF) if k in ("query", "value") else v.to(DEV)) for k, v in inputs.items()}
    seen = []
    real_qpos, real_box = ops.query_pos_k256, ops.box_head_k256

    def run(strip):
        def qpos(*a, **kw):
            seen.append(("in_proj", "in_proj" in kw))
            if strip:
                kw.pop("in_proj", None)
            return real_qpos(*a, **kw)

        def box(*a, **kw):
            seen.append(("class_head", "class_head" in kw))
            if strip:
                kw.pop("class_head", None)
            return real_box(*a, **kw)
        monkeypatch.setattr(ops, "query_pos_k256", qpos)
        monkeypatch.setattr(ops, "box_head_k256", box)
        with torch.no_grad():
            c, b = gpu.decoder(**dev_in)
        return c.float().cpu(), b.float().cpu()

    new_cls, new_box = run(False)
    lib_cls, lib_box = run(True)
    assert seen == [("in_proj", True), ("class_head", True)] * 4              # two layers, two runs: the decoder asked every time
    assert new_cls.shape == want_cls.shape == (2, 2, 300, 91) and new_box.shape == want_box.shape
    for name, new, lib, want in (("classes", new_cls, lib_cls, want_cls), ("coords", new_box, lib_box, want_box)):
        e_new, e_lib = (new - want).abs().max().item(), (lib - want).abs().max().item()
        print(f"decoder {name} vs fp32 CPU oracle: absorbed route {e_new:.4e}, library route {e_lib:.4e}, "
              f"routes apart {(new - lib).abs().max().item():.4e}")
        assert e_new <= 1.25 * e_lib + FLOOR


def test_switches_fall_back_to_the_library_route(monkeypatch):
    """decoder_tail = False / box_head = False: the decoder runs without that kernel (the other stays), and agrees with the default
    route within the bf16-decoder bounds of tests/test_transformer_harness.py (boxes 5e-3, logits 2^-4 of their scale)."""
    from relation_detr_amd import _lib, options
    _, gpu, inputs = _decoder_case()
    dev_in = {k: (v.to(DEV).to(BF) if k in ("query", "value") else v.to(DEV)) for k, v in inputs.items()}
    lib = _lib.load()
    counts = {}
    for sym in ("rdetr_query_pos_inproj_k256_bf16", "rdetr_box_head_cls_k256_bf16"):
        fn = getattr(lib, sym)
        monkeypatch.setattr(lib, sym, lambda *a, fn=fn, sym=sym: (counts.__setitem__(sym, counts.get(sym, 0) + 1), fn(*a))[1])
    with torch.no_grad():
        base_cls, base_box = gpu.decoder(**dev_in)
        assert counts == {"rdetr_query_pos_inproj_k256_bf16": 2, "rdetr_box_head_cls_k256_bf16": 2}
        for switch, sym in (("decoder_tail", "rdetr_query_pos_inproj_k256_bf16"), ("box_head", "rdetr_box_head_cls_k256_bf16")):
            counts.clear()
            options.apply(gpu, **{switch: False})
            c, b = gpu.decoder(**dev_in)
            options.apply(gpu, **{switch: True})
            assert sym not in counts and len(counts) == 1
            assert torch.isfinite(c).all() and (b - base_box).abs().max().item() <= 5e-3
            assert (c.float() - base_cls.float()).abs().max().item() <= 2.0 ** -4 * base_cls.float().abs().max().item()


def test_graph_replay_equals_eager():
    from relation_detr_amd import ops
    head, scale = make_qpos_mlps()
    box, lin = make_box_head(), make_class_head(91)
    w, b = make_in_proj()
    g = torch.Generator().manual_seed(11)
    emb = torch.randn(2, 300, 512, generator=g).to(BF).to(DEV)
    query = torch.randn(2, 300, 256, generator=g).to(BF).to(DEV)
    xa = torch.randn(2, 300, 256, generator=g).to(BF).to(DEV)
    xb = torch.randn(2, 300, 256, generator=g).to(BF).to(DEV)
    ref = torch.rand(2, 300, 4, generator=g).to(DEV)

    def run():
        d0, d1, dc = {"weight": w, "bias": b}, {"weight": w, "bias": b}, {"linear": lin}
        pos0, qpp0 = ops.query_pos_k256(emb, query, head.layers, None, in_proj=d0)
        pos, qpp = ops.query_pos_k256(emb, query, head.layers, scale.layers, in_proj=d1)
        a, bb = ops.box_head_k256(xa, xb, box.layers, ref, class_head=dc)
        return pos0, qpp0, d0["qk"], d0["v"], pos, qpp, d1["qk"], d1["v"], a, bb, dc["out"]

    with torch.no_grad():
        eager = [t.clone() for t in run()]                                    # also fills the packed-weight caches outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = run()
        for t in captured:
            t.zero_()
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
    for e, c in zip(eager, captured):
        assert torch.equal(e, c)
