"""GPU tests of the mixed-precision training routes (relation_detr_amd/amp_train.py; csrc/layernorm.hip, csrc/ffn.hip): bf16 autocast
over fp32 parameters -- the weight pack from fp32, the feed-forward kernels with fp32 at either end, the add + LayerNorm kernels on
operands of mixed dtypes, the two autograd Functions, and the routing of ``add_norm`` / ``feed_forward`` / the MSDA output stage.

References: the existing same-dtype routes (bit for bit, where the mixed kernel only moves a rounding into the kernel) or float64 on
the STORED operand values, never the code under test.  Errors are norm-wise, ``|got - ref| / |ref|``.  Bounds:
  LayerNorm out, stats, dx (fp32)    1e-5                               } the fp32 bounds of tests/test_gpu_ln_train.py
  LayerNorm dgamma, dbeta (fp32)     1e-6 + 4 * 2^-24 * sqrt(rows)      }
  FFN dx (fp32, unrounded)           1e-6 + 4 * 2^-24 * sqrt(F) against float64 dH_stored @ w1_rounded: the same running-sum form, F terms
  FeedForwardMixedFunction           1e-2, and 1.5 x the library route's error (tests/test_gpu_ffn_train.py)
  layers                             err(on) <= 1.25 x err(off) + 2e-2 against the fp32 run (profiles/r14/README.md)
Every figure is printed before it is asserted (run with ``-s``).
"""
import dataclasses
import functools
import os

import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-5
POISON = 0x7FC1                                     # a NaN pattern no kernel writes (as int16; twice as int32: 0x7FC17FC1)
MID_SHAPES = [(75, 101), (38, 51), (19, 26), (10, 13)]       # S = 10,137; B = 2: 20,274 encoder rows
NEW = ("rdetr_add_layernorm_train_mixed", "rdetr_add_layernorm_backward_mixed", "rdetr_ffn_k256_pack_f32",
       "rdetr_ffn_k256_train_xf32_bf16", "rdetr_ffn_k256_backward_dxf32_bf16")
OLD = ("rdetr_add_layernorm_train_f32", "rdetr_add_layernorm_train_bf16", "rdetr_add_layernorm_backward_f32",
       "rdetr_add_layernorm_backward_bf16", "rdetr_ffn_k256_pack_bf16", "rdetr_ffn_k256_train_bf16", "rdetr_ffn_k256_backward_bf16")


@pytest.fixture(scope="module")
def amp():
    from relation_detr_amd import _lib, amp_train
    _lib.load()
    return amp_train


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def nrel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def stream():
    return torch.cuda.current_stream().cuda_stream


class Counting:
    """The library object with the launches of the named entry points counted (and their arguments kept)."""

    def __init__(self, lib, names=NEW + OLD):
        self._lib, self.calls, self.args = lib, dict.fromkeys(names, 0), {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in self.calls:
            def counted(*a):
                self.calls[name] += 1
                self.args[name] = a
                return fn(*a)
            return counted
        return fn

    def new(self):
        return {n: self.calls[n] for n in NEW}

    def old(self):
        return sum(self.calls[n] for n in OLD)


def counting_lib(monkeypatch):
    from relation_detr_amd import _lib
    counting = Counting(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: counting)
    return counting


# ================================================================================================== feed-forward: operands
@functools.lru_cache(maxsize=None)
def ffn_inputs(M, Fh, wide=False):
    """fp32 operands of the scales of tests/test_gpu_ffn_train.py, and their bf16 roundings; built once, never modified."""
    g = torch.Generator(device=DEV).manual_seed(M + Fh)
    rn = lambda *shape, scale=1.0: torch.randn(*shape, generator=g, device=DEV) * scale
    x = rn(M, 768)[:, 256:512] if wide else rn(M, 256)
    dy = rn(M, 256).to(BF)
    w1, b1, w2, b2 = rn(Fh, 256, scale=1 / 16), rn(Fh, scale=0.1), rn(256, Fh, scale=1 / 45), rn(256, scale=0.1)
    return dict(x=x, dy=dy, w1=w1, b1=b1, w2=w2, b2=b2, lp=tuple(t.to(BF) for t in (x, w1, b1, w2, b2)))


# 1. ------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("Fh", [64, 2048])
def test_pack_from_fp32_has_the_bits_of_the_bf16_pack(amp, Fh):
    from relation_detr_amd import ffn_train
    c = ffn_inputs(257, Fh)
    w1, b1, w2, b2 = c["w1"], c["b1"], c["w2"], c["b2"]
    packed, b1b, b2b = amp.ffn_pack_f32(w1, w2, b1, b2)
    assert same_bits(packed, ffn_train._pack(w1.to(BF), w2.to(BF)))
    assert same_bits(b1b, b1.to(BF)) and same_bits(b2b, b2.to(BF))
    alone, none1, none2 = amp.ffn_pack_f32(w1, w2)
    assert same_bits(alone, packed) and none1 is None and none2 is None
    # the backward's operands, read in place through the strides of the transposed views
    packed_t, _, _ = amp.ffn_pack_f32(w2.t(), w1.t())
    assert same_bits(packed_t, ffn_train._pack(w2.to(BF).t().contiguous(), w1.to(BF).t().contiguous()))
    # ... and any other strides: the rows of a wider matrix
    wide = torch.zeros(Fh, 320, device=DEV)
    wide[:, 32:288] = w1
    assert same_bits(amp.ffn_pack_f32(wide[:, 32:288], w2)[0], packed)


# 2. ---------------------------------------------------------------------------------------------------------- forward
FFN_CASES = [(M, Fh, False) for M in (1, 257, 16391) for Fh in (64, 1024)] + [(257, 64, True), (16391, 1024, True)]
FFN_IDS = [f"{M}x{Fh}{'-column-slice' if wide else ''}" for M, Fh, wide in FFN_CASES]


@pytest.mark.parametrize("M,Fh,wide", FFN_CASES, ids=FFN_IDS)
def test_ffn_forward_has_the_bits_of_the_bf16_route_on_the_rounded_operands(amp, M, Fh, wide):
    from relation_detr_amd import ffn_train
    c = ffn_inputs(M, Fh, wide)
    assert (c["x"].stride(0) == 768) == wide and c["x"].dtype == F32
    out, hid, xlp = amp.ffn_mixed_train(c["x"], c["w1"], c["b1"], c["w2"], c["b2"])
    want_out, want_hid = ffn_train.ffn_k256_train(*c["lp"])
    assert same_bits(out, want_out) and same_bits(hid, want_hid)
    assert same_bits(xlp, c["x"].to(BF)) and xlp.is_contiguous()
    # bf16 x with fp32 parameters: the existing kernel behind the fp32 pack; x is its own bf16 copy
    out_b, hid_b, x_b = amp.ffn_mixed_train(c["lp"][0], c["w1"], c["b1"], c["w2"], c["b2"])
    assert same_bits(out_b, want_out) and same_bits(hid_b, want_hid) and x_b is c["lp"][0]


def test_ffn_tail_rows_and_wider_buffers_stay_untouched(amp):
    """Rows at or beyond M are neither read nor written: launches over the first M rows of larger, poisoned out / H / xlp / dH / dx
    buffers, H and dH with leading dimensions wider than F, leave everything else as it was."""
    from relation_detr_amd import _lib, ffn_train
    M, Fh, ld = 300, 128, 192
    c = ffn_inputs(M, Fh)
    xb, w1b, b1b, w2b, b2b = c["lp"]
    out_ref, hid_ref = ffn_train.ffn_k256_train(xb, w1b, b1b, w2b, b2b)
    dx_ref, dh_ref = ffn_train.ffn_k256_backward(c["dy"], hid_ref, w1b, w2b)
    lib = _lib.load()
    packed, p1, p2 = amp.ffn_pack_f32(c["w1"], c["w2"], c["b1"], c["b2"])
    full = lambda rows, cols: torch.full((rows, cols), POISON, dtype=torch.int16, device=DEV)
    hid, out, xlp = full(M + 40, ld), full(M + 40, 256), full(M + 40, 264)
    st = lib.rdetr_ffn_k256_train_xf32_bf16(c["x"].data_ptr(), 256, packed.data_ptr(), p1.data_ptr(), p2.data_ptr(), M, Fh, out.data_ptr(),
                                            256, hid.data_ptr(), ld, xlp.data_ptr(), 264, stream())
    assert st == 0
    assert torch.equal(hid[:M, :Fh].view(BF), hid_ref) and bool((hid[M:] == POISON).all()) and bool((hid[:, Fh:] == POISON).all())
    assert torch.equal(out[:M].view(BF), out_ref) and bool((out[M:] == POISON).all())
    assert torch.equal(xlp[:M, :256].view(BF), xb) and bool((xlp[M:] == POISON).all()) and bool((xlp[:, 256:] == POISON).all())
    dh = full(M + 40, ld)
    dx = torch.full((M + 40, 260), 0x7FC17FC1, dtype=torch.int32, device=DEV)
    packed_t, _, _ = amp.ffn_pack_f32(c["w2"].t(), c["w1"].t())
    st = lib.rdetr_ffn_k256_backward_dxf32_bf16(c["dy"].data_ptr(), 256, packed_t.data_ptr(), hid.data_ptr(), ld, M, Fh, dh.data_ptr(), ld,
                                                dx.data_ptr(), 260, stream())
    assert st == 0
    assert torch.equal(dh[:M, :Fh].view(BF), dh_ref) and bool((dh[M:] == POISON).all()) and bool((dh[:, Fh:] == POISON).all())
    assert torch.equal(dx[:M, :256].view(F32).to(BF), dx_ref)
    assert bool((dx[M:] == 0x7FC17FC1).all()) and bool((dx[:, 256:] == 0x7FC17FC1).all())


# 3. --------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("M,Fh,wide", FFN_CASES, ids=FFN_IDS)
def test_ffn_backward_keeps_dh_and_leaves_dx_unrounded(amp, M, Fh, wide, monkeypatch):
    from relation_detr_amd import ffn_train
    c = ffn_inputs(M, Fh, wide)
    xb, w1b, b1b, w2b, b2b = c["lp"]
    _, hid = ffn_train.ffn_k256_train(xb, w1b, b1b, w2b, b2b)
    dx_ref, dh_ref = ffn_train.ffn_k256_backward(c["dy"], hid, w1b, w2b)
    dy = c["dy"]
    if wide:                                        # dy as the middle 256 columns of an [M, 768] tensor: lddy = 768 reaches the entry
        dy = torch.zeros(M, 768, dtype=BF, device=DEV)
        dy[:, 256:512] = c["dy"]
        dy = dy[:, 256:512]
    counting = counting_lib(monkeypatch)
    dx, dh = amp.ffn_mixed_backward(dy, hid, c["w1"], c["w2"], fp32_dx=True)
    assert counting.args["rdetr_ffn_k256_backward_dxf32_bf16"][1] == (768 if wide else 256)
    dy = c["dy"]
    assert dx.dtype == F32 and dx.shape == dx_ref.shape
    assert same_bits(dh, dh_ref)
    assert same_bits(dx.to(BF), dx_ref)
    err, bound = nrel(dx, dh.double() @ w1b.double()), 1e-6 + 4 * 2.0 ** -24 * Fh ** 0.5
    print(f"\n[{M} x {Fh}] fp32 dx against float64 dH_stored @ w1_rounded: {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    dx_b, dh_b = amp.ffn_mixed_backward(c["dy"], hid, c["w1"], c["w2"], fp32_dx=False)       # bf16 x: the existing kernel
    assert same_bits(dx_b, dx_ref) and same_bits(dh_b, dh_ref)
    dx2, dh2 = amp.ffn_mixed_backward(c["dy"], hid, c["w1"], c["w2"], fp32_dx=True)          # no atomics
    assert same_bits(dx2, dx) and same_bits(dh2, dh)


# 4. --------------------------------------------------------------------------------------------------------- Function
NAMES = ("dx", "dW1", "db1", "dW2", "db2")


def ffn_route(fused, c, x_dtype, needs=(True,) * 5):
    """One forward + backward under bf16 autocast on fp32 parameters: the mixed Function or the two library GEMMs."""
    from relation_detr_amd.amp_train import FeedForwardMixedFunction
    src = (c["x"].to(x_dtype), c["w1"], c["b1"], c["w2"], c["b2"])
    leaves = [t.detach().clone().requires_grad_(n) for t, n in zip(src, needs)]
    with torch.autocast("cuda", dtype=BF):
        if fused:
            out = FeedForwardMixedFunction.apply(*leaves)
        else:
            out = F.linear(F.relu(F.linear(leaves[0], leaves[1], leaves[2])), leaves[3], leaves[4])
    out.backward(c["dy"])
    return out.detach(), tuple(t.grad for t in leaves)


@pytest.mark.parametrize("x_dtype", [F32, BF], ids=["x-fp32", "x-bf16"])
@pytest.mark.parametrize("M,Fh", [(257, 64), (16391, 1024)], ids=["257x64", "16391x1024"])
def test_function_gradients_against_fp64(amp, M, Fh, x_dtype):
    from relation_detr_amd import ffn_train
    c = ffn_inputs(M, Fh)
    x64, w164, b164, w264, b264 = (t.double().detach().clone().requires_grad_() for t in c["lp"])     # the stored (rounded) values
    F.linear(F.relu(F.linear(x64, w164, b164)), w264, b264).backward(c["dy"].double())
    ref = (x64.grad, w164.grad, b164.grad, w264.grad, b264.grad)
    out_f, grads_f = ffn_route(True, c, x_dtype)
    out_l, grads_l = ffn_route(False, c, x_dtype)
    assert out_f.dtype == BF and out_l.dtype == BF                           # as autocast's linear2 returns
    assert same_bits(out_f, ffn_train.ffn_k256_train(*c["lp"])[0])
    for n, g, r in zip(NAMES, grads_f, ref):
        assert g.dtype == (x_dtype if n == "dx" else F32) and g.shape == r.shape, n      # each leaf's own dtype
    errs_f = [nrel(g, r) for g, r in zip(grads_f, ref)]
    errs_l = [nrel(g, r) for g, r in zip(grads_l, ref)]
    print()
    for n, ef, el in zip(NAMES, errs_f, errs_l):
        print(f"    [{M} x {Fh} {'fp32' if x_dtype == F32 else 'bf16'} x] {n:4s} mixed {ef:.3e}   autocast library route {el:.3e}   "
              f"ratio {ef / el if el else float('inf'):.3f}")
    for n, ef, el in zip(NAMES, errs_f, errs_l):
        assert ef <= 1e-2, (n, ef)
        assert ef <= 1.5 * el, (n, ef, el)
    _, again = ffn_route(True, c, x_dtype)
    for n, a, b in zip(NAMES, grads_f, again):
        assert same_bits(a, b), n


@pytest.mark.parametrize("x_dtype", [F32, BF], ids=["x-fp32", "x-bf16"])
@pytest.mark.parametrize("needs", [(False, True, True, True, True), (True, False, False, False, False),
                                   (False, False, False, True, True)],
                         ids=["weights-only", "x-only", "linear2-only"])
def test_function_honours_needs_input_grad(amp, needs, x_dtype, monkeypatch):
    c = ffn_inputs(257, 64)
    _, full = ffn_route(True, c, x_dtype)
    counting = counting_lib(monkeypatch)
    _, part = ffn_route(True, c, x_dtype, needs=needs)
    for n, need, got, want in zip(NAMES, needs, part, full):
        if need:
            assert same_bits(got, want), n
        else:
            assert got is None, n
    ran = int(any(needs[:3]))                       # nothing upstream of H needs a gradient: the backward kernel does not run
    fwd, bwd = (("rdetr_ffn_k256_train_xf32_bf16", "rdetr_ffn_k256_backward_dxf32_bf16") if x_dtype == F32
                else ("rdetr_ffn_k256_train_bf16", "rdetr_ffn_k256_backward_bf16"))
    assert counting.calls[fwd] == 1 and counting.calls[bwd] == ran
    assert counting.calls["rdetr_ffn_k256_pack_f32"] == 1 + ran and counting.calls["rdetr_ffn_k256_pack_bf16"] == 0
    assert sum(counting.calls.values()) == 2 + 2 * ran


# ================================================================================================= add + LayerNorm: 5.
def _big_rows():
    from relation_detr_amd import ln_train
    return 16 * ln_train.MAX_PARTIALS * 2 + 5            # the grid stride takes more than two trips, with a ragged tail


PAIRS = {"f32+bf16": (F32, BF), "bf16+f32": (BF, F32), "bf16+bf16": (BF, BF), "bf16": (BF, None), "f32": (F32, None)}
LN_CASES = ([(p, n, "plain") for p in PAIRS for n in (1, 15, 16, 17, 257, "big")]
            + [(p, n, v) for p in PAIRS for n in (257, "big") for v in ("sliced_x", "expanded_dy")])
LN_IDS = [f"{p}-{n}-{v}" for p, n, v in LN_CASES]


@functools.lru_cache(maxsize=None)
def ln_case(pair, rows, variant):
    """Operands in their storage dtypes and the float64 reference on their stored values; built once, never modified."""
    xd, rd = PAIRS[pair]
    rows = _big_rows() if rows == "big" else rows
    g = torch.Generator(device=DEV).manual_seed(1000 + rows)                 # the operands of tests/test_gpu_ln_train.py
    randn = lambda *shape: torch.randn(*shape, generator=g, device=DEV)
    wide = randn(rows, 768).to(xd)
    x = wide[:, 256:512] if variant == "sliced_x" else wide[:, 256:512].contiguous()
    r = None if rd is None else randn(rows, 256).to(rd)
    dy = torch.ones((), device=DEV).expand(rows, 256) if variant == "expanded_dy" else randn(rows, 256)
    gamma, beta = 1 + 0.1 * randn(256), 0.1 * randn(256)
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    r64 = None if r is None else r.double().requires_grad_(True)
    s64 = x64 if r64 is None else x64 + r64
    out64 = F.layer_norm(s64, (256,), g64, b64, EPS)
    out64.backward(dy.double())
    with torch.no_grad():
        mean, rstd = s64.mean(-1), (s64.var(-1, unbiased=False) + EPS).rsqrt()
    ref = dict(out=out64.detach(), dx=x64.grad, dgamma=g64.grad, dbeta=b64.grad, mean=mean, rstd=rstd)
    return dict(rows=rows, x=x, r=r, dy=dy, gamma=gamma, beta=beta, ref=ref)


@pytest.mark.parametrize("pair,rows,variant", LN_CASES, ids=LN_IDS)
def test_layernorm_kernels_against_float64(amp, pair, rows, variant):
    c = ln_case(pair, rows, variant)
    n, ref = c["rows"], c["ref"]
    dtypes = {c["x"].dtype} | ({c["r"].dtype} if c["r"] is not None else set())
    out, stats = amp.add_layer_norm_mixed_train(c["x"], c["r"], c["gamma"], c["beta"], EPS)
    assert out.dtype == F32 and out.shape == c["x"].shape and out.is_contiguous()
    assert stats.dtype == F32 and tuple(stats.shape) == (n, 2)
    dx, dxb, dgamma, dbeta = amp.add_layer_norm_mixed_backward(c["dy"], c["x"], c["r"], stats, c["gamma"])
    assert (dx is not None) == (F32 in dtypes) and (dxb is not None) == (BF in dtypes)
    # the raw entry with BOTH gradient tensors: the fp32 dx is checked for every pair, its bf16 twin is its rounding
    from relation_detr_amd import _lib
    from relation_detr_amd.ln_train import _rows
    lib = _lib.load()
    (x, ldx), (dy, lddy) = _rows(c["x"]), _rows(c["dy"])
    both = torch.empty(n, 256, device=DEV), torch.empty(n, 256, dtype=BF, device=DEV)
    dg2, db2 = torch.empty(256, device=DEV), torch.empty(256, device=DEV)
    nbytes = lib.rdetr_add_layernorm_backward_workspace_bytes(n)
    ws = torch.empty(nbytes // 4, device=DEV)
    st = lib.rdetr_add_layernorm_backward_mixed(dy.data_ptr(), lddy, x.data_ptr(), int(x.dtype == BF), ldx,
                                                None if c["r"] is None else c["r"].data_ptr(), int(c["r"] is not None and c["r"].dtype == BF),
                                                256, c["gamma"].data_ptr(), stats.data_ptr(), n, 256, ws.data_ptr(), nbytes,
                                                both[0].data_ptr(), both[1].data_ptr(), dg2.data_ptr(), db2.data_ptr(), stream())
    assert st == 0
    assert same_bits(both[1], both[0].to(BF))
    assert dx is None or same_bits(dx, both[0])
    assert dxb is None or same_bits(dxb, both[1])
    assert same_bits(dgamma, dg2) and same_bits(dbeta, db2)
    bound_p = 1e-6 + 4 * 2.0 ** -24 * n ** 0.5
    err = dict(out=(nrel(out, ref["out"]), 1e-5), mean=(nrel(stats[:, 0], ref["mean"]), 1e-5), rstd=(nrel(stats[:, 1], ref["rstd"]), 1e-5),
               dx=(nrel(both[0], ref["dx"]), 1e-5), dgamma=(nrel(dgamma, ref["dgamma"]), bound_p), dbeta=(nrel(dbeta, ref["dbeta"]), bound_p))
    print("\n" + "  ".join(f"{k} {e:.2e} (bound {b:.2e})" for k, (e, b) in err.items()))
    bad = {k: v for k, v in err.items() if not v[0] <= v[1]}
    assert not bad, bad
    # a second backward: the same bits in every output (no atomics, a fixed summation order)
    dx_2, dxb_2, dgamma_2, dbeta_2 = amp.add_layer_norm_mixed_backward(c["dy"], c["x"], c["r"], stats, c["gamma"])
    assert (dx is None or same_bits(dx, dx_2)) and (dxb is None or same_bits(dxb, dxb_2))
    assert same_bits(dgamma, dgamma_2) and same_bits(dbeta, dbeta_2)


@pytest.mark.parametrize("pair", list(PAIRS))
def test_layernorm_function_hands_each_operand_its_dtype(amp, pair):
    c = ln_case(pair, 257, "plain")
    _, stats = amp.add_layer_norm_mixed_train(c["x"], c["r"], c["gamma"], c["beta"], EPS)
    dx, dxb, dgamma, dbeta = amp.add_layer_norm_mixed_backward(c["dy"], c["x"], c["r"], stats, c["gamma"])
    leaf = lambda t, grad=True: None if t is None else t.detach().clone().requires_grad_(grad)
    x, r, gamma, beta = leaf(c["x"]), leaf(c["r"]), leaf(c["gamma"]), leaf(c["beta"])
    out = amp.AddLayerNormMixedFunction.apply(x, r, gamma, beta, EPS)
    assert out.dtype == F32
    out.backward(c["dy"])
    pick = lambda t: dxb if t.dtype == BF else dx
    assert x.grad.dtype == x.dtype and same_bits(x.grad, pick(x))
    if r is not None:
        assert r.grad.dtype == r.dtype and same_bits(r.grad, pick(r))
    assert gamma.grad.dtype == F32 and same_bits(gamma.grad, dgamma) and same_bits(beta.grad, dbeta)
    # one dtype on both operands: ONE tensor serves both, as AddLayerNormFunction does (a leaf used twice gets it added twice)
    if pair == "bf16+bf16":
        twice = leaf(c["x"])
        amp.AddLayerNormMixedFunction.apply(twice, twice, c["gamma"], c["beta"], EPS).backward(c["dy"])
        _, st2 = amp.add_layer_norm_mixed_train(twice, twice, c["gamma"], c["beta"], EPS)
        _, d2, _, _ = amp.add_layer_norm_mixed_backward(c["dy"], twice, twice, st2, c["gamma"], need_params=False)
        assert same_bits(twice.grad, d2 + d2)


@pytest.mark.parametrize("pair", ["f32+bf16", "bf16"])
def test_layernorm_frozen_parameters_take_one_launch_and_no_workspace(amp, pair, monkeypatch):
    c = ln_case(pair, 257, "plain")
    _, stats = amp.add_layer_norm_mixed_train(c["x"], c["r"], c["gamma"], c["beta"], EPS)
    dx, dxb, _, _ = amp.add_layer_norm_mixed_backward(c["dy"], c["x"], c["r"], stats, c["gamma"])
    counting = counting_lib(monkeypatch)
    x = c["x"].detach().clone().requires_grad_(True)
    out = amp.AddLayerNormMixedFunction.apply(x, c["r"], c["gamma"], c["beta"], EPS)     # parameters and residual without a gradient
    out.backward(c["dy"])
    assert counting.calls["rdetr_add_layernorm_backward_mixed"] == 1
    args = counting.args["rdetr_add_layernorm_backward_mixed"]
    assert args[12] is None and args[13] == 0 and args[16] is None and args[17] is None       # workspace, its size, dgamma, dbeta
    assert same_bits(x.grad, dxb if x.dtype == BF else dx)


def test_layernorm_tail_rows_stay_untouched(amp):
    from relation_detr_amd import _lib
    lib = _lib.load()
    c = ln_case("f32+bf16", 17, "plain")
    n = 17
    want_out, want_stats = amp.add_layer_norm_mixed_train(c["x"], c["r"], c["gamma"], c["beta"], EPS)
    want_dx, want_dxb, _, _ = amp.add_layer_norm_mixed_backward(c["dy"], c["x"], c["r"], want_stats, c["gamma"], need_params=False)
    p32 = 0x7FC17FC1
    out = torch.full((n + 20, 260), p32, dtype=torch.int32, device=DEV)
    stats = torch.full((n + 20, 2), p32, dtype=torch.int32, device=DEV)
    st = lib.rdetr_add_layernorm_train_mixed(c["x"].data_ptr(), 0, 256, c["r"].data_ptr(), 1, 256, c["gamma"].data_ptr(), c["beta"].data_ptr(),
                                             n, 256, EPS, out.data_ptr(), 260, stats.data_ptr(), stream())
    assert st == 0
    assert torch.equal(out[:n, :256].view(F32), want_out) and bool((out[n:] == p32).all()) and bool((out[:, 256:] == p32).all())
    assert torch.equal(stats[:n].view(F32), want_stats) and bool((stats[n:] == p32).all())
    dx = torch.full((n + 20, 256), p32, dtype=torch.int32, device=DEV)
    dxb = torch.full((n + 20, 256), POISON, dtype=torch.int16, device=DEV)
    st = lib.rdetr_add_layernorm_backward_mixed(c["dy"].data_ptr(), 256, c["x"].data_ptr(), 0, 256, c["r"].data_ptr(), 1, 256,
                                                c["gamma"].data_ptr(), want_stats.data_ptr(), n, 256, None, 0, dx.data_ptr(), dxb.data_ptr(),
                                                None, None, stream())
    assert st == 0
    assert torch.equal(dx[:n].view(F32), want_dx) and bool((dx[n:] == p32).all())
    assert torch.equal(dxb[:n].view(BF), want_dxb) and bool((dxb[n:] == POISON).all())


# ====================================================================================================== 6. routing, 7. layers
def _layer_state(layer, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                      # non-trivial projections, distinct LayerNorm parameters
        for m in layer.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
        for p in layer.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.02)
    return layer.state_dict()


@functools.lru_cache(maxsize=None)
def _layer_inputs(kind):
    from helpers import pyramid
    _, _, S = pyramid(MID_SHAPES)
    g = torch.Generator().manual_seed(7)
    B, N = 2, 400
    if kind == "encoder":
        return (torch.randn(B, S, 256, generator=g), torch.randn(B, S, 256, generator=g), torch.rand(B, S, 4, 2, generator=g),
                torch.randn(B, S, 256, generator=g))
    ref = torch.cat([torch.rand(B, N, 4, 2, generator=g), torch.rand(B, N, 4, 2, generator=g) * 0.4 + 0.05], -1)      # fixed: no top-k
    return (torch.randn(B, N, 256, generator=g), torch.randn(B, N, 256, generator=g), ref, torch.randn(B, S, 256, generator=g),
            torch.randn(B, N, 256, generator=g))


def _fresh_state(kind, seed=5):
    from relation_detr_amd.transformer import RelationTransformerDecoderLayer, RelationTransformerEncoderLayer
    torch.manual_seed(0)
    cls = RelationTransformerEncoderLayer if kind == "encoder" else RelationTransformerDecoderLayer
    return _layer_state(cls(256, 2048, 8, 4, 4), seed)


def _make_layer(kind, state=None, dtype=F32, **switches):
    from relation_detr_amd import options
    from relation_detr_amd.transformer import RelationTransformerDecoderLayer, RelationTransformerEncoderLayer
    cls = RelationTransformerEncoderLayer if kind == "encoder" else RelationTransformerDecoderLayer
    with options.override(**switches):
        layer = cls(256, 2048, 8, 4, 4)
    if state is not None:
        layer.load_state_dict(state)
    return layer.to(DEV).to(dtype).train()


def _run_layer(kind, layer, autocast, dtype=F32):
    from helpers import pyramid
    shp, start, _ = pyramid(MID_SHAPES)
    shp, start = shp.to(DEV), start.to(DEV)
    inputs = _layer_inputs(kind)
    cast = lambda t: t.to(DEV).to(dtype).requires_grad_(True)
    layer.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=BF, enabled=autocast):
        if kind == "encoder":
            query, pos, ref, go = inputs
            q, p = cast(query), cast(pos)
            r = ref.to(DEV).requires_grad_(True)
            out = layer(q, p, r, shp, start)
            leaves = {"d/d query": q, "d/d query_pos": p, "d/d reference_points": r}
        else:
            query, pos, ref, value, go = inputs
            q, p, v = cast(query), cast(pos), cast(value)
            r = ref.to(DEV).requires_grad_(True)
            out = layer(q, p, r, v, shp, start)
            leaves = {"d/d query": q, "d/d query_pos": p, "d/d reference_points": r, "d/d value": v}
    out.backward(go.to(DEV).to(out.dtype))
    res = {"output": out.detach()}
    res.update({k: t.grad for k, t in leaves.items()})
    res.update({n: p.grad for n, p in layer.named_parameters()})
    return res


BOTH = dict(ln_train_fused=True, ffn_train_fused=True)


def test_routing_under_autocast(amp, monkeypatch):
    """The new entry points run under bf16 autocast over fp32 parameters with the switches on -- and nowhere else."""
    from relation_detr_amd import options
    from relation_detr_amd.transformer import add_norm
    counting = counting_lib(monkeypatch)
    zero = dict.fromkeys(NEW, 0)

    def launched(fn):
        for k in counting.calls:
            counting.calls[k] = 0
        fn()
        return counting.new(), counting.old()

    state = _fresh_state("encoder")
    on, off = _make_layer("encoder", state, **BOTH), _make_layer("encoder", state)
    # the encoder layer at 20,274 rows: norm1 through the MSDA module's _output(post_norm=), feed_forward, norm2 through add_norm
    new, old = launched(lambda: _run_layer("encoder", on, autocast=True))
    assert new == {"rdetr_add_layernorm_train_mixed": 2, "rdetr_add_layernorm_backward_mixed": 2, "rdetr_ffn_k256_pack_f32": 2,
                   "rdetr_ffn_k256_train_xf32_bf16": 1, "rdetr_ffn_k256_backward_dxf32_bf16": 1}, new
    assert old == 0
    assert launched(lambda: _run_layer("encoder", off, autocast=True)) == (zero, 0)          # the switches off: the default
    new, old = launched(lambda: _run_layer("encoder", on, autocast=False))                   # outside autocast: fp32, today's route
    assert new == zero and old == counting.calls["rdetr_add_layernorm_train_f32"] + counting.calls["rdetr_add_layernorm_backward_f32"] == 4
    del on, off
    # a network converted to bf16: only the same-dtype entry points, with and without autocast around it
    bf = _make_layer("encoder", state, dtype=BF, **BOTH)
    for autocast in (False, True):
        new, old = launched(lambda: _run_layer("encoder", bf, autocast=autocast, dtype=BF))
        assert new == zero, (autocast, new)
        assert (counting.calls["rdetr_add_layernorm_train_bf16"], counting.calls["rdetr_add_layernorm_backward_bf16"],
                counting.calls["rdetr_ffn_k256_train_bf16"], counting.calls["rdetr_ffn_k256_backward_bf16"]) == (2, 2, 1, 1)
    del bf

    # add_norm itself: the fp32 stream + a bf16 sublayer output, a bf16 input alone
    opts_on, opts_off = dataclasses.replace(options.Options(), **BOTH), options.Options()
    norm = torch.nn.LayerNorm(256).to(DEV)
    x = torch.randn(2, 9, 256, device=DEV, requires_grad=True)
    r = torch.randn(2, 9, 256, device=DEV).to(BF).requires_grad_(True)

    def call(opts, autocast, a, b):
        with torch.autocast("cuda", dtype=BF, enabled=autocast):
            y = add_norm(norm, a, b, opts=opts)
            want = norm(a if b is None else a + b)
        assert y.dtype == want.dtype == F32
        assert nrel(y.detach(), want.detach()) <= 1e-5
        y.square().sum().backward()

    new, old = launched(lambda: call(opts_on, True, x, r))
    assert (new["rdetr_add_layernorm_train_mixed"], new["rdetr_add_layernorm_backward_mixed"], old) == (1, 1, 0)
    assert x.grad.dtype == F32 and r.grad.dtype == BF and same_bits(r.grad, x.grad.to(BF))
    new, old = launched(lambda: call(opts_on, True, r, None))
    assert (new["rdetr_add_layernorm_train_mixed"], new["rdetr_add_layernorm_backward_mixed"], old) == (1, 1, 0)
    assert launched(lambda: call(opts_off, True, x, r)) == (zero, 0)
    new, old = launched(lambda: call(opts_on, True, x, None))                # everything fp32: the same-dtype route first, as today
    assert new == zero and old == 2
    new, old = launched(lambda: call(opts_on, False, x, None))               # outside autocast: today's route
    assert new == zero and old == 2


def _layer_table(kind):
    state = _fresh_state(kind)
    want = _run_layer(kind, _make_layer(kind, state), autocast=False)
    got = {"off": _run_layer(kind, _make_layer(kind, state), autocast=True),
           "on": _run_layer(kind, _make_layer(kind, state, **BOTH), autocast=True)}
    lines = [f"{kind + ' layer: tensor':44s} {'err (autocast, off)':>22s} {'err (autocast, on)':>22s}"]
    bad = []
    for name, ref in want.items():
        if ref is None:                                  # a parameter the layer does not use on this call: on no route
            assert got["off"][name] is None and got["on"][name] is None, name
            continue
        assert got["on"][name].dtype == got["off"][name].dtype == ref.dtype, name
        e_off, e_on = nrel(got["off"][name], ref), nrel(got["on"][name], ref)
        lines.append(f"{name:44s} {e_off:22.3e} {e_on:22.3e}")
        if not e_on <= 1.25 * e_off + 2e-2:
            bad.append(name)
    return "\n".join(lines), bad


def test_layers_are_as_accurate_as_autocast_on_the_torch_route(amp):
    """One encoder and one decoder layer, fp32 parameters, B = 2, the mid-size pyramid, d_ffn 2048, 400 decoder queries with fixed
    reference points.  The fp32 run without autocast is the reference; for the output and every gradient the norm-wise error under
    autocast with ``ln_train_fused`` + ``ffn_train_fused`` is at most 1.25 x that under autocast with the defaults + 2e-2."""
    tables, bad = [], []
    for kind in ("encoder", "decoder"):
        table, b = _layer_table(kind)
        tables.append(table)
        bad += [f"{kind}: {n}" for n in b]
    text = "\n\n".join(tables)
    print("\n" + text)
    if os.environ.get("RDETR_ACCURACY_OUT"):
        with open(os.environ["RDETR_ACCURACY_OUT"], "w") as f:
            f.write("RelationTransformerEncoderLayer / RelationTransformerDecoderLayer, fp32 parameters, .train(), levels (75,101),(38,51),"
                    "(19,26),(10,13), B = 2, d_ffn 2048, 400 decoder queries;\nnorm-wise error against the same weights in fp32 without "
                    "autocast: bf16 autocast with the defaults / with ln_train_fused + ffn_train_fused\n" + text + "\n")
    assert not bad, f"the mixed routes are less accurate than autocast on the torch route: {bad}\n{text}"
