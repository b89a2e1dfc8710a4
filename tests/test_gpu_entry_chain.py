"""GPU tests of the two thin phases at the ends of a step's dependency chain: ops.tokens_from_levels (every level of a pyramid
in one launch, csrc/glue.hip) and ops.topk (one launch per selection below kTkOneLaunchMaxN, csrc/topk.hip).  Both are pure
data movement / selection, so every comparison is torch.equal against the torch expression they replace."""
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIXED = [(8, 12), (5, 9), (4, 6), (1, 3)]                       # 96, 45, 24, 3 pixels: multiples of 8 and not, in one call
PYRAMIDS = {
    "mixed4": MIXED,
    "five": [(9, 16), (7, 11), (4, 8), (3, 3), (1, 1)],         # 144 (more than two tiles), 77, 32, 9 and a level of one pixel
    "one": [(5, 13)],
    "one_pixel": [(1, 1)],
    "eight": [(8, 8), (3, 7), (4, 4), (1, 5), (2, 4), (1, 1), (3, 3), (2, 8)],
    "nine": [(8, 8), (3, 7), (4, 4), (1, 5), (2, 4), (1, 1), (3, 3), (2, 8), (1, 2)],      # > 8 levels: the per-level loop
}


def _levels(shapes, B, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    lv = [torch.randn(B, C, h, w, generator=g).to(dtype).to(DEV) for h, w in shapes]
    em = [torch.randn(C, generator=g).to(dtype).to(DEV) for _ in shapes]
    return lv, em


def _reference(lv, em):
    return torch.cat([x.flatten(2).transpose(1, 2) + e if e is not None else x.flatten(2).transpose(1, 2)
                      for x, e in zip(lv, em or [None] * len(lv))], 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_vecs", [False, True])
@pytest.mark.parametrize("name,B,C", [("mixed4", 3, 256), ("mixed4", 2, 72), ("five", 2, 256), ("one", 1, 72), ("one_pixel", 3, 256),
                                      ("eight", 2, 72), ("nine", 2, 256)])
def test_tokens_from_levels_equals_cat_of_transposes(name, B, C, with_vecs, dtype):
    from relation_detr_amd import ops
    lv, em = _levels(PYRAMIDS[name], B, C, dtype, seed=B * 1000 + C)
    out = ops.tokens_from_levels(lv, add_vecs=em if with_vecs else None)
    ref = _reference(lv, em if with_vecs else None)
    assert out.dtype == dtype and out.shape == ref.shape and torch.equal(out, ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("col0", [256, 4])                      # 16-byte aligned rows of the slice, and not
def test_tokens_from_levels_into_a_column_slice(dtype, col0):
    """The destination is columns [col0, col0 + C) of a wider zeroed buffer (the memory-fusion buffer of the stack is 7 C wide):
    the other columns stay zero."""
    from relation_detr_amd import ops
    B, C = 3, 256
    lv, em = _levels(MIXED, B, C, dtype, seed=7)
    S = sum(h * w for h, w in MIXED)
    wide = torch.zeros(B, S, 3 * C, dtype=dtype, device=DEV)
    ops.tokens_from_levels(lv, add_vecs=em, out=wide[:, :, col0:col0 + C])
    assert torch.equal(wide[:, :, col0:col0 + C], _reference(lv, em))
    assert not wide[:, :, :col0].any() and not wide[:, :, col0 + C:].any()


def test_tokens_from_levels_unaligned_vectors_and_levels():
    """bf16 level embeddings that are rows of one [L, C + 1] tensor and levels that are views at odd element offsets: neither is
    16-byte aligned, so the call takes its 2-byte accesses."""
    from relation_detr_amd import ops
    B, C = 2, 72
    g = torch.Generator().manual_seed(11)
    flat = torch.randn(B * C * 96 + 1, generator=g).to(torch.bfloat16).to(DEV)
    lv = [flat[1:].view(B, C, 8, 12), torch.randn(B, C, 5, 9, generator=g).to(torch.bfloat16).to(DEV)]
    table = torch.randn(2, C + 1, generator=g).to(torch.bfloat16).to(DEV)
    em = [table[0, 1:], table[1, 1:]]
    assert torch.equal(ops.tokens_from_levels(lv, add_vecs=em), _reference(lv, em))


def test_tokens_from_levels_captures_into_a_graph():
    from relation_detr_amd import ops
    lv, em = _levels(MIXED, 2, 256, torch.bfloat16, seed=3)
    eager = ops.tokens_from_levels(lv, add_vecs=em)
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.tokens_from_levels(lv, add_vecs=em, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.tokens_from_levels(lv, add_vecs=em, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    for x in lv:                                                # new inputs at the captured addresses
        x.neg_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, _reference(lv, em))


def test_levels_entry_point_limits():
    import ctypes
    from relation_detr_amd import _lib
    lib = _lib.load()
    x = torch.zeros(1, 8, 4, device=DEV)
    out = torch.zeros(1, 36, 8, device=DEV)
    src = (ctypes.c_void_p * 9)(*[x.data_ptr()] * 9)
    pix = (ctypes.c_int * 9)(*[4] * 9)
    assert lib.rdetr_nchw_levels_to_tokens(src, None, pix, 9, 0, 1, 8, 36 * 8, 8, out.data_ptr(), None) == _lib.ERR_UNSUPPORTED
    assert lib.rdetr_nchw_levels_to_tokens(src, None, pix, 8, 0, 65536, 8, 36 * 8, 8, out.data_ptr(), None) == _lib.ERR_UNSUPPORTED
    assert lib.rdetr_nchw_levels_to_tokens(src, None, pix, 8, 2, 1, 8, 36 * 8, 8, out.data_ptr(), None) == _lib.ERR_UNSUPPORTED
    assert lib.rdetr_nchw_levels_to_tokens(src, None, pix, 0, 0, 1, 8, 36 * 8, 8, out.data_ptr(), None) == _lib.ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------------- top-k
def _one_launch_max_n() -> int:
    """kTkOneLaunchMaxN of csrc/topk.hip: the longest row the one-launch kernel takes."""
    path = os.path.join(ROOT, "relation_detr_amd", "csrc", "topk.hip")
    m = re.search(r"constexpr\s+int\s+kTkOneLaunchMaxN\s*=\s*(\d+)\s*;", open(path).read())
    if m is None:
        raise RuntimeError(f"{path}: no `constexpr int kTkOneLaunchMaxN = <number>;` -- these tests place n on both sides of it")
    t = int(m.group(1))
    if not 1024 < t < (1 << 19):
        raise RuntimeError(f"{path}: kTkOneLaunchMaxN = {t} must lie in (1024, 2^19) so that the tests reach both paths")
    return t


T = _one_launch_max_n()


def _check(x, k):
    from relation_detr_amd import ops
    v, i = ops.topk(x, k)
    sv, si = torch.sort(x.float(), dim=1, descending=True, stable=True)        # value descending, equal values by ascending index
    assert v.dtype == torch.float32 and i.dtype == torch.int64
    assert torch.equal(i, si[:, :k])
    nan = sv[:, :k].isnan()
    assert torch.equal(v.isnan(), nan) and torch.equal(v[~nan], sv[:, :k][~nan])


# n on both sides of the threshold T between the one-launch kernel and the four launches; odd n with rows > 1 puts the later rows
# off the 16-byte boundary (scalar head and tail of the row)
TOPK_CASES = [(2, 300, 300), (5, 301, 300), (1, 1, 1), (2, 1024, 1024), (1, 1025, 1024), (2, 4095, 900), (5, 4097, 1024), (1, 4097, 1),
              (2, 22323, 900), (5, 22323, 300), (2, 81900, 300), (1, 81900, 1), (2, 27300, 300), (1, 204098, 900),
              (2, T - 1, 900), (1, T, 1024), (2, T + 1, 900), (5, T + 3, 300), (1, 600000, 1024), (2, 600001, 1)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,n,k", TOPK_CASES)
def test_topk_equals_stable_sort_on_both_paths(rows, n, k, dtype):
    g = torch.Generator().manual_seed(n + k)
    x = torch.randn(rows, n, generator=g)
    if dtype == torch.bfloat16:
        x = (x * 0.05 - 4.0).to(torch.bfloat16)                                # scores around the class prior: thousands of ties
    _check(x.to(DEV), k)


@pytest.mark.parametrize("rows,n,k", [(2, 22323, 900), (5, 4097, 300), (1, T + 1, 1024)])
def test_topk_bf16_scores_of_eight_distinct_values(rows, n, k):
    """The boundary bin holds about n / 8 .. n elements: the candidates are (nearly) the whole row."""
    g = torch.Generator().manual_seed(n)
    vals = torch.tensor([-4.0, -4.03125, -4.0625, -3.96875, -4.125, -3.9375, -4.09375, -3.90625])     # one level-1 bin per two
    x = vals[torch.randint(0, 8, (rows, n), generator=g)].to(torch.bfloat16)
    _check(x.to(DEV), k)
    _check(torch.full((rows, n), -4.0).to(torch.bfloat16).to(DEV), k)                                # all equal


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,n,k", [(2, 5001, 700), (2, T + 1, 700)])
def test_topk_all_equal_and_special_values(rows, n, k, dtype):
    _check(torch.zeros(rows, n, dtype=dtype, device=DEV), k)
    g = torch.Generator().manual_seed(5)
    y = torch.randn(rows, n, generator=g).to(dtype)
    y[:, 17] = float("nan"); y[:, n - 1] = float("nan"); y[0, 400] = float("inf"); y[1, 0] = float("inf")
    y[:, 5] = float("-inf"); y[0, 4999] = float("-inf")
    _check(y.to(DEV), k)
    _check(y[:, :k + 1].contiguous().to(DEV), k + 1)                             # k == n: a full sort with NaN and both infinities


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_topk_rows_off_the_16_byte_boundary(dtype):
    """The matrix itself starts one element past an aligned address and n is odd: every row has a scalar head and tail."""
    g = torch.Generator().manual_seed(9)
    rows, n = 3, 4099
    flat = torch.randn(rows * n + 1, generator=g).to(dtype).to(DEV)
    x = flat[1:].view(rows, n)
    assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    _check(x, 300)
    _check(x[:, :9].contiguous(), 9)                                             # shorter than one 16-byte load


def test_topk_captures_into_a_graph():
    from relation_detr_amd import ops
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(2, 22323, generator=g) * 0.05 - 4.0).to(torch.bfloat16).to(DEV)
    ev, ei = ops.topk(x, 900)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.topk(x, 900)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        v, i = ops.topk(x, 900)
    for _ in range(2):
        v.zero_(); i.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(v, ev) and torch.equal(i, ei)
