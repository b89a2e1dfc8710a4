"""The step order of the fused inference feed-forward kernel (csrc/ffn_k256_body.h) through ``ops.ffn_k256``.

The kernel walks the hidden units in chunks of 64; inside a chunk it runs GEMM 1 of both tile pairs, then GEMM 2 of both, with the
bias + round + ReLU of a pair cut into slices behind the next 16 steps and the next chunk's weights fetched piece by piece.  What
can go wrong is an index map: a W2 fragment paired with the wrong half of the hidden units, a slice reading the wrong accumulator
or bias pair, a weight piece landing in the buffer that is being read.

Reference: float64 with the rounding points of the unfused route, ``h = relu(bf16(x W1^T + b1))``, ``out = bf16(h W2^T + b2)`` --
never the code under test.  Bound (every element): ``2^-8 |ref| + 1e-3 max(1, max |ref|)``, the form of
tests/test_gpu_ffn_train.py::within_bf16_form.

Row counts: 1, 15, 16, 17, 33 (tails inside a wave's two 16-row blocks), 255, 256, 257, 273 (the second tile and its partial
first wave), 513.  F: 64 (one chunk), 128 (both LDS buffers), 192 (a buffer reused), 2048.  Inputs: x ~ N(0,1), W1 ~ N(0,1)/16,
so pre-activations of unit scale, b1 ~ N(0,1): the bias decides the sign of many hidden units and the ReLU cuts about half.
One input set and one reference per F (513 rows); a case with fewer rows takes their first rows.

Scale of the outputs.  The relative part of the bound is HALF a bf16 ulp of the reference at most (an ulp is 2^-8 .. 2^-7 of the
value), and the reference is itself rounded to bf16.  A kernel that adds the same products in fp32 and in another order than
float64 can land on the other side of a rounding boundary and be one whole ulp from the reference: right, and outside the bound
unless the absolute part covers the other half ulp, 2^-8 |v| <= 1e-3, i.e. |v| <= 0.256 (while max |ref| <= 1).  So W2 ~
N(0,1) / (28 sqrt(F)) and b2 ~ 0.02 N(0,1): E[h^2] is about 1 (the ReLU of N(0,2)), out has a standard deviation near 1/28 =
0.036 for every F, and max |ref| < 0.25 is asserted.  A wrong index still shows: one hidden unit read from the wrong place moves
an output by about |W2| = 1 / (28 sqrt(F)), and a wrong map moves at least two units of every chunk -- 6e-3 at F = 64 and at
F = 2048 (64 units, adding in quadrature), against a bound of about 1.2e-3.  With outputs of unit scale (W2 ~ N(0,1)/45) the
first version of this file measured max err / bound 1.03 .. 1.09 at F = 2048 and <= 0.80 below: single elements one ulp (2^-6 at
|v| in [2, 4)) from the reference, on bits equal to those of the kernel before its steps were reordered.

Every figure is printed before it is asserted (run with ``-s``).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
ROWS = (1, 15, 16, 17, 33, 255, 256, 257, 273, 513)
FS = (64, 128, 192, 2048)
WIDE = 1792                                         # leading dimension of the column-slice cases
POISON = -777.0                                     # exactly representable in bf16


@pytest.fixture(scope="module")
def ops():
    from relation_detr_amd import _lib, ops
    _lib.load()
    return ops


def reference(x, w1, b1, w2, b2):
    h = torch.relu((x.double() @ w1.double().t() + b1.double()).to(BF)).double()
    return (h @ w2.double().t() + b2.double()).to(BF).double(), h


_cache = {}


def case(Fh):
    """inputs at 513 rows and their reference, made once per F and never written to"""
    if Fh not in _cache:
        g = torch.Generator(device=DEV).manual_seed(1000 + Fh)

        def rn(*shape, scale=1.0):
            return (torch.randn(*shape, generator=g, device=DEV) * scale).to(BF)
        x, w1, b1 = rn(max(ROWS), 256), rn(Fh, 256, scale=1 / 16), rn(Fh)
        w2, b2 = rn(256, Fh, scale=1 / (28 * Fh ** 0.5)), rn(256, scale=0.02)
        ref, h = reference(x, w1, b1, w2, b2)
        assert float(ref.abs().max()) < 0.25, "outputs too large for the bound to admit a one-ulp difference (module docstring)"
        _cache[Fh] = (x, w1, b1, w2, b2, ref, float((h == 0).double().mean()))
    return _cache[Fh]


def bound(ref):
    return 2.0 ** -8 * ref.abs() + 1e-3 * max(1.0, float(ref.abs().max()))


def worst(got, ref):
    """max over the elements of |got - ref| / bound"""
    return float(((got.double() - ref).abs() / bound(ref)).max())


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("Fh", FS)
@pytest.mark.parametrize("M", ROWS)
def test_against_float64(ops, M, Fh):
    x, w1, b1, w2, b2, ref, cut = case(Fh)
    out = ops.ffn_k256(x[:M], w1, b1, w2, b2)
    again = ops.ffn_k256(x[:M], w1, b1, w2, b2)
    torch.cuda.synchronize()
    w = worst(out, ref[:M])
    print(f"rows {M} F {Fh}: max err / bound {w:.3f}; hidden units cut by the ReLU {cut:.3f}")
    assert 0.4 < cut < 0.6
    assert out.shape == (M, 256) and bool(torch.isfinite(out).all())
    assert w <= 1.0
    assert torch.equal(bits(out), bits(again)), "two launches on the same inputs differ"


@pytest.mark.parametrize("M,Fh", [(273, 128), (513, 192), (17, 64), (257, 2048)])
def test_column_slices_and_poison(ops, M, Fh):
    """x and out as column slices of [rows, 1792] buffers; out's buffer has 40 more rows: nothing outside out[:M] is written"""
    x, w1, b1, w2, b2, ref, _ = case(Fh)
    xbuf = torch.full((M, WIDE), 3.0, dtype=BF, device=DEV)
    xbuf[:, 512:768] = x[:M]
    obuf = torch.full((M + 40, WIDE), POISON, dtype=BF, device=DEV)
    got = ops.ffn_k256(xbuf[:, 512:768], w1, b1, w2, b2, out=obuf[:M, 1024:1280])
    torch.cuda.synchronize()
    assert got.data_ptr() == obuf[:M, 1024:1280].data_ptr()
    w = worst(obuf[:M, 1024:1280], ref[:M])
    dense = ops.ffn_k256(x[:M], w1, b1, w2, b2)
    print(f"rows {M} F {Fh}, ld {WIDE}: max err / bound {w:.3f}")
    assert w <= 1.0
    assert torch.equal(bits(obuf[:M, 1024:1280]), bits(dense)), "a column slice computes other bits than dense rows"
    assert bool((obuf[M:] == POISON).all()), "rows at or beyond M were written"
    assert bool((obuf[:M, :1024] == POISON).all()) and bool((obuf[:M, 1280:] == POISON).all()), "columns outside the slice were written"


@pytest.mark.parametrize("M,Fh", [(273, 128), (513, 192), (33, 64), (257, 2048)])
def test_hidden_unit_order(ops, M, Fh):
    """one permutation of the hidden units applied to W1's rows, b1 and W2's columns: the same function, summed in another order.
    A step map that pairs a W2 fragment with the wrong half of h does not survive it."""
    x, w1, b1, w2, b2, ref, _ = case(Fh)
    perm = torch.randperm(Fh, generator=torch.Generator().manual_seed(Fh)).to(DEV)
    out = ops.ffn_k256(x[:M], w1, b1, w2, b2)
    outp = ops.ffn_k256(x[:M], w1[perm].contiguous(), b1[perm].contiguous(), w2[:, perm].contiguous(), b2)
    torch.cuda.synchronize()
    w = worst(outp, ref[:M])
    apart = float((outp.double() - out.double()).abs().max())
    print(f"rows {M} F {Fh}: permuted max err / bound {w:.3f}; permuted vs unpermuted max |diff| {apart:.4f}")
    assert w <= 1.0
    assert worst(out, ref[:M]) <= 1.0
