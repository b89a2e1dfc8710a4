"""GPU tests of the decoder chain's two fused MLP kernels, rdetr_query_pos_k256_bf16 (csrc/qpos.hip) and rdetr_box_head_k256_bf16
(csrc/mlp.hip), whose workgroups own 16 / 32 rows and split the output columns over their waves: row tails and tiny problems, rows
that are column slices of wider buffers, exact row independence (a row's result does not depend on the call it is computed in),
repeatability, HIP-graph replay, and the fp32-product reference with the bounds of tests/test_gpu_glue.py (box head: max 4e-3,
mean 2e-4; query_pos: 2^-7 of the output scale, mean a sixteenth of it; qpp exactly the bf16 sum of the kernel's own query_pos)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = (1, 15, 16, 17, 31, 33, 37, 903, 1800, 1801)


def bf(t):
    return t.to(torch.bfloat16).float()


def make_qpos_mlps():
    from relation_detr_amd.transformer import MLP
    torch.manual_seed(7)
    head = MLP(512, 256, 256, 2).to(DEV).to(torch.bfloat16)
    scale = MLP(256, 256, 256, 2).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        for l in (*head.layers, *scale.layers):
            l.bias.copy_(torch.randn(256) * 0.1)
    return head, scale


def make_box_head():
    from relation_detr_amd.transformer import MLP
    torch.manual_seed(5)
    head = MLP(256, 256, 4, 3).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        head.layers[2].weight.copy_(torch.randn(4, 256) * 0.05)           # the reference initialises the last layer with zeros
        head.layers[2].bias.copy_(torch.randn(4) * 0.1)
        for l in head.layers[:2]:
            l.bias.copy_(torch.randn(256) * 0.1)
    return head


def mlp2_want(m, x):
    """fp32 products of the bf16 operands, every intermediate rounded to bf16 where the unfused path stores it"""
    h = bf((x.float() @ m.layers[0].weight.float().t() + m.layers[0].bias.float()).relu())
    return bf(h @ m.layers[1].weight.float().t() + m.layers[1].bias.float())


def box_want(head, x, logit):
    h = x.float()
    for i, l in enumerate(head.layers):
        h = h @ l.weight.float().t() + l.bias.float()
        if i < 2:
            h = h.relu()
        h = bf(h)
    return (h + logit).sigmoid()


def check_qpos(pos, qpp, want, query):
    tol = 2.0 ** -7 * want.abs().max().item()
    err = (pos.float() - want).abs()
    print(f"query_pos rows {want.shape[0]}: max err {err.max().item():.3e} (bound {tol:.3e}) mean {err.mean().item():.3e} (bound {tol / 16:.3e})")
    assert err.max().item() <= tol and err.mean().item() <= tol / 16
    assert torch.equal(qpp, (query.float() + pos.float()).to(torch.bfloat16))          # the sum of the kernel's own query_pos


def check_box(got, want):
    err = (got - want).abs()
    print(f"box head rows {want.shape[0]}: max err {err.max().item():.3e} (bound 4e-3) mean {err.mean().item():.3e} (bound 2e-4)")
    assert err.max().item() <= 4e-3 and err.mean().item() <= 2e-4


@pytest.mark.parametrize("M", ROWS)
def test_query_pos_row_tails_against_the_fp32_product_reference(M):
    from relation_detr_amd import ops
    head, scale = make_qpos_mlps()
    g = torch.Generator().manual_seed(100 + M)
    emb = torch.randn(M, 512, generator=g).to(torch.bfloat16).to(DEV)
    query = torch.randn(M, 256, generator=g).to(torch.bfloat16).to(DEV)
    for scaled in (False, True):
        pos, qpp = ops.query_pos_k256(emb, query, head.layers, scale.layers if scaled else None)
        assert pos.dtype == torch.bfloat16 and pos.shape == query.shape and qpp.shape == query.shape
        want = mlp2_want(head, emb)
        if scaled:
            want = bf(want * mlp2_want(scale, query))
        check_qpos(pos, qpp, want, query)


@pytest.mark.parametrize("M", ROWS)
def test_box_head_row_tails_against_the_fp32_product_reference(M):
    from relation_detr_amd import ops
    from relation_detr_amd.transformer import inverse_sigmoid
    head = make_box_head()
    g = torch.Generator().manual_seed(200 + M)
    xa = torch.randn(M, 256, generator=g).to(torch.bfloat16).to(DEV)
    xb = torch.randn(M, 256, generator=g).to(torch.bfloat16).to(DEV)
    ref = torch.rand(M, 4, generator=g).to(DEV)
    ref[0] = torch.tensor([0.0, 1.0, 1e-5, 0.5])                             # the clamps of inverse_sigmoid
    got_a, got_b = ops.box_head_k256(xa, xb, head.layers, ref)                # the A / B seam falls inside a row block unless 32 | M
    assert got_a.dtype == torch.float32 and got_a.shape == ref.shape and got_b.shape == ref.shape
    check_box(got_a, box_want(head, xa, inverse_sigmoid(ref)))
    check_box(got_b, box_want(head, xb, inverse_sigmoid(ref)))
    assert torch.equal(ops.box_head_k256(xa, None, head.layers, ref), got_a)
    assert torch.equal(ops.box_head_k256(xb, None, head.layers, ref), got_b)
    # the reference given as a logit (two-stage proposals), +inf where a proposal is invalid -> box 1.0 like torch
    logit = torch.log(ref.clamp(1e-3, 1 - 1e-3) / (1 - ref.clamp(1e-3, 1 - 1e-3)))
    logit[M // 2] = float("inf")
    got_l = ops.box_head_k256(xa, None, head.layers, logit, reference_is_logit=True)
    check_box(got_l, box_want(head, xa, logit))
    assert (got_l[M // 2] == 1.0).all()


def test_rows_that_are_column_slices_of_wider_buffers_and_the_expanded_query():
    from relation_detr_amd import ops
    from relation_detr_amd.transformer import inverse_sigmoid
    head, scale = make_qpos_mlps()
    box = make_box_head()
    g = torch.Generator().manual_seed(9)
    B, N = 2, 333
    wide_e = torch.randn(B, N, 512 + 256, generator=g).to(torch.bfloat16).to(DEV)
    wide_q = torch.randn(B, N, 3 * 256, generator=g).to(torch.bfloat16).to(DEV)
    emb, query = wide_e[..., 256:], wide_q[..., 256:512]                      # lde = 768 > 512, ldq = 768 > 256
    assert not emb.is_contiguous() and not query.is_contiguous()
    for sc in (None, scale.layers):
        pos, qpp = ops.query_pos_k256(emb, query, head.layers, sc)
        pos_c, qpp_c = ops.query_pos_k256(emb.contiguous(), query.contiguous(), head.layers, sc)
        assert torch.equal(pos, pos_c) and torch.equal(qpp, qpp_c)
        want = mlp2_want(head, emb.reshape(-1, 512))
        if sc is not None:
            want = bf(want * mlp2_want(scale, query.reshape(-1, 256)))
        check_qpos(pos.reshape(-1, 256), qpp.reshape(-1, 256), want, query.reshape(-1, 256))
    # layer 0's query is an expanded embedding (batch stride 0)
    q0 = torch.randn(N, 256, generator=g).to(torch.bfloat16).to(DEV).expand(B, -1, -1)
    assert q0.stride(0) == 0
    pos, qpp = ops.query_pos_k256(emb, q0, head.layers, None)
    check_qpos(pos.reshape(-1, 256), qpp.reshape(-1, 256), mlp2_want(head, emb.reshape(-1, 512)), q0.reshape(-1, 256))
    # box head: lda != ldb, both wider than a row
    xa, xb = wide_q[..., 512:], wide_e[..., :256]
    ref = torch.rand(B, N, 4, generator=g).to(DEV)
    got_a, got_b = ops.box_head_k256(xa, xb, box.layers, ref)
    con_a, con_b = ops.box_head_k256(xa.contiguous(), xb.contiguous(), box.layers, ref)
    assert torch.equal(got_a, con_a) and torch.equal(got_b, con_b)
    check_box(got_a.reshape(-1, 4), box_want(box, xa.reshape(-1, 256), inverse_sigmoid(ref).reshape(-1, 4)))
    check_box(got_b.reshape(-1, 4), box_want(box, xb.reshape(-1, 256), inverse_sigmoid(ref).reshape(-1, 4)))


def test_a_row_does_not_depend_on_the_call_it_is_computed_in():
    """Exact row independence: the same row alone, at another position of a shorter call, and inside the full call; and a second
    run of the full call."""
    from relation_detr_amd import ops
    head, scale = make_qpos_mlps()
    box = make_box_head()
    g = torch.Generator().manual_seed(10)
    M = 1801
    emb = torch.randn(M, 512, generator=g).to(torch.bfloat16).to(DEV)
    query = torch.randn(M, 256, generator=g).to(torch.bfloat16).to(DEV)
    xa = torch.randn(M, 256, generator=g).to(torch.bfloat16).to(DEV)
    xb = torch.randn(M, 256, generator=g).to(torch.bfloat16).to(DEV)
    ref = torch.rand(M, 4, generator=g).to(DEV)
    for sc in (None, scale.layers):
        pos, qpp = ops.query_pos_k256(emb, query, head.layers, sc)
        again = ops.query_pos_k256(emb, query, head.layers, sc)
        assert torch.equal(pos, again[0]) and torch.equal(qpp, again[1])
        for r in (0, 5, 16, 899, 1799, 1800):
            p1, q1 = ops.query_pos_k256(emb[r:r + 1], query[r:r + 1], head.layers, sc)
            assert torch.equal(p1[0], pos[r]) and torch.equal(q1[0], qpp[r])
        for start, stop in ((3, 700), (1795, 1801), (17, 50)):                # the rows at other lanes, waves' blocks and workgroups
            p2, q2 = ops.query_pos_k256(emb[start:stop], query[start:stop], head.layers, sc)
            assert torch.equal(p2, pos[start:stop]) and torch.equal(q2, qpp[start:stop])
    got_a, got_b = ops.box_head_k256(xa, xb, box.layers, ref)
    again = ops.box_head_k256(xa, xb, box.layers, ref)
    assert torch.equal(got_a, again[0]) and torch.equal(got_b, again[1])
    for r in (0, 5, 16, 31, 32, 899, 1799, 1800):
        a1, b1 = ops.box_head_k256(xa[r:r + 1], xb[r:r + 1], box.layers, ref[r:r + 1])
        assert torch.equal(a1[0], got_a[r]) and torch.equal(b1[0], got_b[r])
    for start, stop in ((3, 700), (1795, 1801), (17, 50)):
        a2, b2 = ops.box_head_k256(xa[start:stop], xb[start:stop], box.layers, ref[start:stop])
        assert torch.equal(a2, got_a[start:stop]) and torch.equal(b2, got_b[start:stop])
    swapped_b, swapped_a = ops.box_head_k256(xb, xa, box.layers, ref)         # a row gives the same box as input A and as input B
    assert torch.equal(swapped_a, got_a) and torch.equal(swapped_b, got_b)


def test_graph_replay_equals_eager():
    from relation_detr_amd import ops
    head, scale = make_qpos_mlps()
    box = make_box_head()
    g = torch.Generator().manual_seed(11)
    M = 1800
    emb = torch.randn(2, M // 2, 512, generator=g).to(torch.bfloat16).to(DEV)
    query = torch.randn(2, M // 2, 256, generator=g).to(torch.bfloat16).to(DEV)
    xa = torch.randn(2, M // 2, 256, generator=g).to(torch.bfloat16).to(DEV)
    xb = torch.randn(2, M // 2, 256, generator=g).to(torch.bfloat16).to(DEV)
    ref = torch.rand(2, M // 2, 4, generator=g).to(DEV)

    def run():
        pos0, qpp0 = ops.query_pos_k256(emb, query, head.layers, None)
        pos, qpp = ops.query_pos_k256(emb, query, head.layers, scale.layers)
        a, b = ops.box_head_k256(xa, xb, box.layers, ref)
        return pos0, qpp0, pos, qpp, a, b

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
