"""The fused bf16 training route of the feed-forward block (csrc/ffn.hip, relation_detr_amd/ffn_train.py) on the device.

Reference: float64 autograd of ``linear2(relu(linear1(x)))`` on the bf16-rounded inputs -- never the code under test.  The
library route (the switch off: two GEMMs and the ReLU passes under autograd) is measured against the same reference in the
same test; both routes round at the same points and differ in fp32 summation order only.

Inputs: x, dY ~ N(0,1), W1 ~ N(0,1)/16, W2 ~ N(0,1)/45, biases ~ 0.1 N(0,1): hidden pre-activations of unit scale, so that next
to none of them lies within a bf16 rounding of zero (the ReLU masks of the routes and of the reference agree).

Every figure is printed before it is asserted (run with ``-s``); profiles/r10/README.md says where a run's output is filed.
"""
import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NAMES = ("dx", "dW1", "db1", "dW2", "db2")


@pytest.fixture(scope="module")
def rd():
    import relation_detr_amd
    from relation_detr_amd import _lib
    _lib.load()
    return relation_detr_amd


def make_inputs(M, Fh, seed=0, wide=False):
    g = torch.Generator(device=DEV).manual_seed(seed)

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, device=DEV) * scale).to(BF)
    if wide:                                        # x as a column slice of a wider tensor (ldx = 768)
        x = rn(M, 768)[:, 256:512]
    else:
        x = rn(M, 256)
    return x, rn(M, 256), rn(Fh, 256, scale=1 / 16), rn(Fh, scale=0.1), rn(256, Fh, scale=1 / 45), rn(256, scale=0.1)


def reference(x, dy, w1, b1, w2, b2, loss_sum=False):
    x, w1, b1, w2, b2 = (t.double().detach().clone().requires_grad_() for t in (x, w1, b1, w2, b2))
    pre = F.linear(x, w1, b1)
    out = F.linear(F.relu(pre), w2, b2)
    if loss_sum:
        out.sum().backward()
    else:
        out.backward(dy.double())
    return out.detach(), pre.detach(), (x.grad, w1.grad, b1.grad, w2.grad, b2.grad)


def run_route(fused, x, dy, w1, b1, w2, b2, loss_sum=False, needs=(True,) * 5):
    """One forward + backward on the fused Function or on the library route -> (out, the five gradients)."""
    from relation_detr_amd.ffn_train import FeedForwardFunction
    leaves = [t.detach().clone().requires_grad_(n) if i else t.detach().requires_grad_(n)
              for i, (t, n) in enumerate(zip((x, w1, b1, w2, b2), needs))]
    if fused:
        out = FeedForwardFunction.apply(*leaves)
    else:
        out = F.linear(F.relu(F.linear(leaves[0], leaves[1], leaves[2])), leaves[3], leaves[4])
    if loss_sum:
        out.sum().backward()
    else:
        out.backward(dy)
    return out.detach(), tuple(t.grad for t in leaves)


def rel_err(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


def within_bf16_form(got, ref):
    """share of elements within 2^-8 |ref| + 1e-3 max(1, max |ref|)"""
    tol = 2.0 ** -8 * ref.abs() + 1e-3 * max(1.0, float(ref.abs().max()))
    return float(((got.double() - ref).abs() <= tol).double().mean())


CASES = [
    pytest.param(20274, 2048, False, False, id="20274x2048"),
    pytest.param(44646, 2048, False, False, id="44646x2048"),
    pytest.param(16391, 1024, False, False, id="16391x1024"),
    pytest.param(257, 64, False, False, id="257x64"),
    pytest.param(1, 64, False, False, id="1x64"),
    pytest.param(16391, 1024, True, False, id="16391x1024-column-slice"),
    pytest.param(20274, 2048, False, True, id="20274x2048-sum-loss"),
]


@pytest.mark.parametrize("M,Fh,wide,loss_sum", CASES)
def test_forward_and_gradients_against_fp64(rd, M, Fh, wide, loss_sum):
    from relation_detr_amd import ffn_train, ops
    x, dy, w1, b1, w2, b2 = make_inputs(M, Fh, seed=M + Fh, wide=wide)
    assert (x.stride(0) == 768) == wide
    ref_out, ref_pre, ref_grads = reference(x, dy, w1, b1, w2, b2, loss_sum)
    ref_h = ref_pre.clamp_min(0)

    # forward: the inference kernel's bits, and the stored hidden activations
    out, hid = ffn_train.ffn_k256_train(x, w1, b1, w2, b2)
    with torch.no_grad():
        assert torch.equal(out, ops.ffn_k256(x, w1, b1, w2, b2))
    share_h, share_o = within_bf16_form(hid, ref_h), within_bf16_form(out, ref_out)
    flips = float(((hid > 0) != (ref_pre > 0)).double().mean())
    print(f"\n[{M} x {Fh}{' slice' if wide else ''}{' sum' if loss_sum else ''}] H within bf16 form {share_h:.6f}  out {share_o:.6f}  "
          f"ReLU mask disagreement {flips:.2e}")
    assert share_h >= 0.999 and share_o >= 0.999
    assert flips <= 1e-3
    del hid, ref_pre, ref_h

    out_f, grads_f = run_route(True, x, dy, w1, b1, w2, b2, loss_sum)
    out_l, grads_l = run_route(False, x, dy, w1, b1, w2, b2, loss_sum)
    assert torch.equal(out_f, out)
    errs_f = [rel_err(g, r) for g, r in zip(grads_f, ref_grads)]
    errs_l = [rel_err(g, r) for g, r in zip(grads_l, ref_grads)]
    for n, ef, el in zip(NAMES, errs_f, errs_l):
        print(f"    {n:4s} fused {ef:.3e}   library {el:.3e}   ratio {ef / el if el else float('inf'):.3f}")
    for n, g, r in zip(NAMES, grads_f, ref_grads):
        assert g.dtype == BF and g.shape == r.shape, n
    for n, ef, el in zip(NAMES, errs_f, errs_l):
        assert ef <= 1e-2, (n, ef)
        assert ef <= 1.5 * el, (n, ef, el)

    # no atomics: a second forward + backward gives the same bits
    out2, hid2 = ffn_train.ffn_k256_train(x, w1, b1, w2, b2)
    out_g, grads_g = run_route(True, x, dy, w1, b1, w2, b2, loss_sum)
    assert torch.equal(out2, out) and torch.equal(out_g, out_f)
    assert torch.equal(hid2, ffn_train.ffn_k256_train(x, w1, b1, w2, b2)[1])
    for n, a, b in zip(NAMES, grads_f, grads_g):
        assert torch.equal(a, b), n


def test_tail_rows_and_wide_hidden_buffers_stay_untouched(rd):
    """Rows at or beyond M are neither read nor written: a launch over the first M rows of larger, poisoned H / dH / dx buffers
    with leading dimensions wider than F leaves everything else as it was."""
    from relation_detr_amd import _lib, ffn_train
    M, Fh, ld = 300, 128, 192
    x, dy, w1, b1, w2, b2 = make_inputs(M, Fh, seed=5)
    _, hid_ref = ffn_train.ffn_k256_train(x, w1, b1, w2, b2)
    dx_ref, dh_ref = ffn_train.ffn_k256_backward(dy, hid_ref, w1, w2)
    stream = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    poison = 0x7FC1                                  # a NaN pattern no kernel writes
    hid = torch.full((M + 40, ld), poison, dtype=torch.int16, device=DEV)
    out = torch.full((M + 40, 256), poison, dtype=torch.int16, device=DEV)
    packed = ffn_train._pack(w1, w2)
    st = lib.rdetr_ffn_k256_train_bf16(x.data_ptr(), 256, packed.data_ptr(), b1.data_ptr(), b2.data_ptr(), M, Fh, out.data_ptr(), 256,
                                       hid.data_ptr(), ld, stream)
    assert st == 0
    assert torch.equal(hid[:M, :Fh].view(BF), hid_ref) and bool((hid[M:] == poison).all()) and bool((hid[:, Fh:] == poison).all())
    assert bool((out[M:] == poison).all())
    dh = torch.full((M + 40, ld), poison, dtype=torch.int16, device=DEV)
    dx = torch.full((M + 40, 256), poison, dtype=torch.int16, device=DEV)
    packed_t = ffn_train._pack(w2.t().contiguous(), w1.t().contiguous())
    st = lib.rdetr_ffn_k256_backward_bf16(dy.data_ptr(), 256, packed_t.data_ptr(), hid.data_ptr(), ld, M, Fh, dh.data_ptr(), ld,
                                          dx.data_ptr(), 256, stream)
    assert st == 0
    assert torch.equal(dh[:M, :Fh].view(BF), dh_ref) and bool((dh[M:] == poison).all()) and bool((dh[:, Fh:] == poison).all())
    assert torch.equal(dx[:M].view(BF), dx_ref) and bool((dx[M:] == poison).all())


def test_backward_kernel_rounding_points(rd):
    """dH is bf16(dY W2) where H > 0 and exactly zero elsewhere; dx is one rounding of the fp32 sum over all of F."""
    from relation_detr_amd import ffn_train
    M, Fh = 1000, 256
    x, dy, w1, b1, w2, b2 = make_inputs(M, Fh, seed=9)
    _, hid = ffn_train.ffn_k256_train(x, w1, b1, w2, b2)
    dx, dh = ffn_train.ffn_k256_backward(dy, hid, w1, w2)
    assert bool((dh[hid <= 0] == 0).all())
    want_dh = (dy.double() @ w2.double()) * (hid > 0)
    assert within_bf16_form(dh, want_dh) >= 0.9999
    want_dx = dh.double() @ w1.double()              # from the kernel's own dH: only the last rounding is left
    assert within_bf16_form(dx, want_dx) == 1.0


@pytest.mark.parametrize("needs", [(False, True, True, True, True), (True, False, False, False, False),
                                   (False, False, False, True, True)],
                         ids=["weights-only", "x-only", "linear2-only"])
def test_needs_input_grad_is_honoured(rd, needs, monkeypatch):
    from relation_detr_amd import ffn_train
    x, dy, w1, b1, w2, b2 = make_inputs(257, 64, seed=3)
    _, full = run_route(True, x, dy, w1, b1, w2, b2)
    calls = []
    real = ffn_train.ffn_k256_backward
    monkeypatch.setattr(ffn_train, "ffn_k256_backward", lambda *a: calls.append(1) or real(*a))
    _, part = run_route(True, x, dy, w1, b1, w2, b2, needs=needs)
    for n, need, got, want in zip(NAMES, needs, part, full):
        if need:
            assert torch.equal(got, want), n
        else:
            assert got is None, n
    assert len(calls) == int(any(needs[:3]))        # nothing upstream of H needs a gradient: the backward kernel does not run


def test_peak_memory_is_not_above_the_library_route(rd):
    M, Fh = 44646, 2048
    x, dy, w1, b1, w2, b2 = make_inputs(M, Fh, seed=1)
    peaks = {}
    for fused in (True, False, True, False):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out, grads = run_route(fused, x, dy, w1, b1, w2, b2)
        torch.cuda.synchronize()
        peaks[fused] = torch.cuda.max_memory_allocated() - base
        del out, grads
    print(f"\npeak memory of one forward + backward above the inputs at {M} x {Fh}: fused {peaks[True] / 2 ** 20:.1f} MiB, "
          f"library {peaks[False] / 2 ** 20:.1f} MiB")
    assert peaks[True] <= peaks[False]


MID_SHAPES = [(75, 101), (38, 51), (19, 26), (10, 13)]       # S = 10,137; B = 2: 20,274 encoder rows


def test_encoder_layer_takes_the_route_only_in_training_with_the_switch_on(rd, monkeypatch):
    from relation_detr_amd import _lib, options
    from relation_detr_amd.transformer import RelationTransformerEncoderLayer

    class Counting:
        """the library object with the two new entry points counted"""

        def __init__(self, lib):
            self._lib, self.calls = lib, {"rdetr_ffn_k256_train_bf16": 0, "rdetr_ffn_k256_backward_bf16": 0}

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if name in self.calls:
                def counted(*a):
                    self.calls[name] += 1
                    return fn(*a)
                return counted
            return fn

    counting = Counting(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: counting)
    torch.manual_seed(0)
    shapes = torch.tensor(MID_SHAPES, dtype=torch.int64)
    areas = shapes[:, 0] * shapes[:, 1]
    start = torch.cat([areas.new_zeros(1), areas.cumsum(0)[:-1]])
    S, B = int(areas.sum()), 2
    assert B * S == 20274
    layer = RelationTransformerEncoderLayer(256, 2048, 8, 4, 4).to(DEV).to(BF).train()
    query = torch.randn(B, S, 256, device=DEV).to(BF)
    pos = torch.randn(B, S, 256, device=DEV).to(BF)
    ref = torch.rand(B, S, 4, 2, device=DEV)

    def step():
        layer.zero_grad()
        q = query.clone().requires_grad_()
        out = layer(q, pos, ref, shapes.to(DEV), start.to(DEV))
        out.float().square().mean().backward()
        return q.grad

    step()                                                                   # the switch off
    assert list(counting.calls.values()) == [0, 0]
    options.apply(layer, ffn_train_fused=True)
    with torch.no_grad():
        layer(query, pos, ref, shapes.to(DEV), start.to(DEV))
    assert list(counting.calls.values()) == [0, 0]                           # inference keeps its own kernel
    gq = step()
    assert list(counting.calls.values()) == [1, 1]
    assert bool(torch.isfinite(gq).all())
    for n, p in layer.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
