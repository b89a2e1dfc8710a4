"""Where every kernel WRITES: the cases of tests/test_gpu_dirty_shapes.py and direct calls of every entry that takes ``out=``, on
guarded allocations (tests/guard.py) under ``Shadow(writes=True)`` (tests/shadow.py).

tests/test_gpu_dirty_shapes.py fills the scratch memory and catches a kernel that reads what it never wrote; here every tensor
the package allocates sits between two 2 MiB bands of 0xA5 (payload 0x42), and after every checked entry
  * every operand that is not in the entry's write set (``shadow.WRITES``) is bit-identical to its copy from before the call,
  * every byte of a declared operand's storage that its elements do not address is unchanged (the neighbour columns and rows of an
    ``out=`` slice), and
  * the bands of the buffers allocated inside the entry and of its operands' storages are intact;
all bands are checked once more when the case ends.

1. The composed cases E1, E2, E3, E4 (bf16, fp32), E5, T1 (atomic, deterministic), T2, T3, T4, once each: the builders of
   tests/test_gpu_dirty_shapes.py themselves (imported, with the guard in the poison's place), so the shapes, the op sets and the
   launch-count route pins are the twins'.  T1 also holds that ``split_merged_projection`` still hands the merged gradient buffer on
   without a copy: guarded tensors are ``set_`` on their buffer, not views of it, so their ``_base`` is None as a fresh tensor's is.
2. Direct calls of every entry that takes ``out=``, with ``out`` a column slice and a row slice of a wider guarded buffer, at 1 row,
   one row below the kernel's row tile, one above it and two tiles + 3 (the tile is read from the kernel, named at each test).
   Where an entry refuses a strided ``out`` by contract the refusal is asserted.
3. The harness's own self-test on the device: the three mistakes, emulated with torch operations through the ``fault`` hook inside
   memory the test itself allocated, are each reported against the right op; the clean run of the same call reports nothing.

With ``RDETR_SHADOW_REPORTS=<directory>`` every composed case writes its table there (``writes_<case>_0x42.txt``; profiles/r29/)."""
import sys

import pytest
import torch

import guard
import shadow
import test_gpu_dirty_shapes as cases
from test_gpu_msda_train_fused import SHAPES4, producer_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
PATTERN = guard.PAYLOAD_BYTE


# ------------------------------------------------------------------------------------------------------------- the harness
class Harness:
    """The guard in the poison's place and ``writes=True`` on every ``shadow.Shadow(monkeypatch)`` the builders make."""

    def __init__(self, monkeypatch):
        self.monkeypatch, self.guard, self.made = monkeypatch, None, []
        real = shadow.Shadow

        def make(mp, fault=None, check=True):
            assert self.guard is not None, "the case built its harness before it installed the scratch memory"
            sh = real(mp, fault=fault, check=check, writes=True, guard=self.guard)
            self.made.append(sh)
            return sh
        monkeypatch.setattr(shadow, "Shadow", make)
        self.how = dict(install=self.install, prefix="writes")

    def install(self, monkeypatch, pattern):
        assert pattern == PATTERN and self.guard is None
        self.guard = guard.guard(monkeypatch)
        return self.guard

    def finish(self, destinations=True):
        """The end of every case, after the builder's own assertions (assert_ok on the twin's op set, the route pins).
        ``destinations=False``: no entry of the case is handed a tensor to write into (T1: every output of the training routes,
        the merged gradient buffer included, is allocated inside its entry), so there is no view to look outside of; that is
        asserted, not assumed, and the bands around every such output stand in for it."""
        (sh,) = self.made
        assert sh.writes and sh.guard is self.guard
        assert not sh.errors, sorted(set(sh.errors))
        bad = [r for r in sh.records if r.kind == "writes" and r.failing]
        assert not bad, "\n".join(f"{r.op} call {r.call}: {r.where}" for r in bad[:20])
        assert sh.finish_bands() == [] and sh._bands_done                     # assert_ok ran the end-of-case pass
        assert self.guard.check() == []                                       # ... and every band, once more, by the guard itself
        values = {r.op for r in sh.records if r.kind == "values"}
        assert {r.op for r in sh.records if r.kind == "writes"} == values == sh.called()
        # the checks cannot pass by not running
        assert sh.write_checks["operand_bits"] > 0 and sh.write_checks["bands"] > 0, sh.write_checks
        assert (sh.write_checks["declared"] > 0) == destinations, sh.write_checks
        assert (sh.write_checks["outside_view"] > 0) == destinations, sh.write_checks
        assert self.guard.fills > 0 and len(self.guard.allocations) == self.guard.fills
        print(f"guard: {self.guard.fills} allocations, {self.guard.bytes / 2 ** 20:.1f} MiB of payload, "
              f"{self.guard.band_bytes() / 2 ** 20:.0f} MiB of bands; write checks {dict(sh.write_checks)}")
        return sh


@pytest.fixture
def harness(monkeypatch):
    return Harness(monkeypatch)


# ------------------------------------------------------------------------------------------------------ 1. the composed cases
def test_e1_resident_gather_odd_batch(monkeypatch, harness):
    cases.e1_case(monkeypatch, PATTERN, **harness.how)
    harness.finish()


def test_e2_below_the_row_threshold_301_queries(monkeypatch, harness):
    cases.e2_case(monkeypatch, PATTERN, **harness.how)
    harness.finish()


def test_e3_five_levels(monkeypatch, harness):
    cases.e3_case(monkeypatch, PATTERN, **harness.how)
    harness.finish()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_e4_short_pyramid_77_queries(monkeypatch, harness, dtype):
    cases.e4_case(monkeypatch, PATTERN, dtype, **harness.how)
    harness.finish()


def test_e5_fp32_entries(monkeypatch, harness):
    cases.e5_case(monkeypatch, PATTERN, **harness.how)
    harness.finish()


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "deterministic"])
def test_t1_all_training_routes(monkeypatch, harness, deterministic):
    from relation_detr_amd import msda_train_hm
    ran = {"forward": 0, "backward": 0, "cat": 0}
    split, cat, backward = msda_train_hm.split_merged_projection, torch.cat, msda_train_hm._SplitMergedProjection.backward.__code__

    def counted_split(both, n_off):
        offsets, logits = split(both, n_off)
        ran["forward"] += 1
        assert offsets.grad_fn is not None and offsets.grad_fn is logits.grad_fn
        offsets.grad_fn.register_hook(lambda *_: ran.__setitem__("backward", ran["backward"] + 1))
        return offsets, logits

    def spied_cat(*args, **kwargs):
        if sys._getframe(1).f_code is backward:                               # the copy route of _SplitMergedProjection.backward
            ran["cat"] += 1
        return cat(*args, **kwargs)
    monkeypatch.setattr(msda_train_hm, "split_merged_projection", counted_split)
    monkeypatch.setattr(torch, "cat", spied_cat)
    cases.t1_case(monkeypatch, PATTERN, deterministic, **harness.how)
    sh = harness.finish(destinations=False)
    # the merged-projection gradient slices: written by the backward into one new buffer, which is the gradient as it is
    assert ran["forward"] == ran["backward"] >= cases.E_LAYERS and ran["cat"] == 0, ran
    assert sh.calls["msda_train_hm.ms_deform_attn_backward_fused_hm"] == cases.E_LAYERS


def test_t2_mixed_precision_detector_two_steps(monkeypatch, harness):
    cases.t2_case(monkeypatch, PATTERN, **harness.how)
    harness.finish()


def test_t3_fp32_detector_step(monkeypatch, harness):
    cases.t3_case(monkeypatch, PATTERN, **harness.how)
    harness.finish()


def test_t4_mixed_precision_detector_step_from_images(monkeypatch, harness):
    cases.t4_case(monkeypatch, PATTERN, **harness.how)
    harness.finish()


# ------------------------------------------------------------------------------------------- 2. every entry that takes out=
def tile_rows(tile):
    """1 row, one below the kernel's row tile, one above it, two tiles + 3."""
    return sorted({1, max(tile - 1, 1), tile + 1, 2 * tile + 3})


@pytest.fixture
def direct(monkeypatch):
    """-> (guard, harness) for direct calls: everything allocated from here on is guarded, every entry checks its write set."""
    g = guard.guard(monkeypatch)
    return g, shadow.Shadow(monkeypatch, writes=True, guard=g)


def dev(t, dtype=None):
    """A guarded device copy: ``torch.empty`` is a covered form, ``Tensor.to`` is not."""
    t = t if dtype is None else t.to(dtype)
    return torch.empty(t.shape, dtype=t.dtype, device=DEV).copy_(t)


def slices(lead, cols, dtype, pad_cols=64, pad_rows=(3, 5)):
    """-> {"columns": lead x cols out of lead x (pad + cols + pad), "rows": rows [3, 3 + n) of a buffer with 8 more rows}, both of
    guarded buffers (payload 0x42 around the slice), 16-byte aligned for every dtype here."""
    *batch, rows = lead
    wide = torch.empty(*batch, rows, pad_cols + cols + pad_cols, dtype=dtype, device=DEV)
    tall = torch.empty(*batch, pad_rows[0] + rows + pad_rows[1], cols, dtype=dtype, device=DEV)
    return {"columns": wide[..., pad_cols:pad_cols + cols], "rows": tall[..., pad_rows[0]:pad_rows[0] + rows, :]}


def end(direct, op, calls, refused=0):
    """`calls` checked calls of `op` and `refused` ones that raised before anything was launched (counted, not recorded)."""
    g, sh = direct
    torch.cuda.synchronize()
    sh.assert_ok({op})
    assert sh.calls[op] == calls + refused and len([r for r in sh.records if r.kind == "values"]) == calls and g.check() == []
    assert sh.write_checks["operand_bits"] > 0 and sh.write_checks["outside_view"] > 0 and sh.write_checks["bands"] > 0
    assert not [r for r in sh.records if r.kind == "writes" and r.failing]


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_add_layer_norm_out_slices(direct, dtype):
    """csrc/layernorm.hip: kLnWaves (4) x kLnRowsPerWave (4) = 16 rows per workgroup."""
    from relation_detr_amd import ops
    g_, calls = gen(1), 0
    w, b = dev(torch.rand(256, generator=g_) + 0.5, dtype), dev(torch.randn(256, generator=g_) * 0.1, dtype)
    for rows in tile_rows(16):
        x, res, pos = (dev(torch.randn(rows, 256, generator=g_), dtype) for _ in range(3))
        for out in slices((rows,), 256, dtype).values():
            got, plus = ops.add_layer_norm(x, res, w, b, out=out, pos=pos)
            assert got.data_ptr() == out.data_ptr() and plus.shape == out.shape
            calls += 1
        got = ops.add_layer_norm(x, None, w, b, out=slices((rows,), 256, dtype)["columns"])      # the kernel without pos
        calls += 1
    end(direct, "add_layer_norm", calls)


def _ffn_weights(g_, F=128):
    return (dev(torch.randn(F, 256, generator=g_) * 0.05, BF16), dev(torch.randn(F, generator=g_) * 0.1, BF16),
            dev(torch.randn(256, F, generator=g_) * 0.05, BF16), dev(torch.randn(256, generator=g_) * 0.1, BF16))


@pytest.mark.parametrize("relu", [False, True])
def test_linear_k256_out_slices(direct, relu):
    """csrc/linear.hip: kLinThreads / 64 (8 waves) x kLinRows (32) = 256 rows per workgroup."""
    from relation_detr_amd import ops
    g_, calls = gen(2), 0
    w, b = dev(torch.randn(96, 256, generator=g_) * 0.05, BF16), dev(torch.randn(96, generator=g_) * 0.1, BF16)
    for rows in tile_rows(256):
        x = dev(torch.randn(rows, 256, generator=g_), BF16)
        for out in slices((rows,), 96, BF16).values():
            assert ops.linear_k256(x, w, b, relu=relu, out=out).data_ptr() == out.data_ptr()
            calls += 1
    end(direct, "linear_k256", calls)


def test_ffn_k256_out_slices(direct):
    """csrc/ffn.hip: kFfnWaves (8) x kFfnRows (32) = 256 rows per workgroup."""
    from relation_detr_amd import ops
    g_, calls = gen(3), 0
    weights = _ffn_weights(g_)
    for rows in tile_rows(256):
        x = dev(torch.randn(rows, 256, generator=g_), BF16)
        for out in slices((rows,), 256, BF16).values():
            assert ops.ffn_k256(x, *weights, out=out).data_ptr() == out.data_ptr()
            calls += 1
    end(direct, "ffn_k256", calls)


def test_ffn_ln_k256_out_slices(direct):
    """csrc/ffn.hip: the same 256-row tile, the LayerNorm epilogue and the second output ``out + pos``."""
    from relation_detr_amd import ops
    g_, calls = gen(4), 0
    weights = _ffn_weights(g_)
    gamma, beta = dev(torch.rand(256, generator=g_) + 0.5, BF16), dev(torch.randn(256, generator=g_) * 0.1, BF16)
    for rows in tile_rows(256):
        x, pos = (dev(torch.randn(rows, 256, generator=g_), BF16) for _ in range(2))
        for name, out in slices((rows,), 256, BF16).items():
            got = ops.ffn_ln_k256(x, *weights, gamma, beta, out=out, pos=pos if name == "columns" else None)
            assert (got[0] if name == "columns" else got).data_ptr() == out.data_ptr()
            calls += 1
    end(direct, "ffn_ln_k256", calls)


def test_linear_ln_k256_out_slices(direct):
    """csrc/rowtail.hip: kRtRows = 32 rows per workgroup up to rowtail.MAX_ROWS rows, with the ``extra`` outputs; above that the
    256-row tiles of csrc/linear.hip (8 waves x kLinRows), at the first row count that takes them + 2: 112 tiles and 131 rows."""
    from relation_detr_amd import ops, rowtail
    g_, calls = gen(5), 0
    w, b = dev(torch.randn(256, 256, generator=g_) * 0.05, BF16), dev(torch.randn(256, generator=g_) * 0.1, BF16)
    gamma, beta = dev(torch.rand(256, generator=g_) + 0.5, BF16), dev(torch.randn(256, generator=g_) * 0.1, BF16)
    for rows in tile_rows(32) + [rowtail.MAX_ROWS + 3]:
        short = rowtail.takes(rows)
        x, res, pos = (dev(torch.randn(rows, 256, generator=g_), BF16) for _ in range(3))
        for name, out in slices((rows,), 256, BF16).items():
            extra = {"pos": pos, "out_plus_pos": slices((rows,), 256, BF16)[name]} if short else None
            got = ops.linear_ln_k256(x, w, b, res, gamma, beta, out=out, extra=extra)
            assert got.data_ptr() == out.data_ptr() and (not short or extra["out"] is got)
            calls += 1
    assert direct[1].launches["rdetr_linear_ln_rows_bf16"] == 8 and direct[1].launches["rdetr_linear_ln_k256_bf16"] == 2
    end(direct, "linear_ln_k256", calls)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_tokens_from_levels_out_slices(direct, dtype):
    """csrc/glue.hip (nchw_levels_to_tokens_kernel): 64-pixel x 64-channel tiles; two levels per call, so the second level starts
    at a row that is no multiple of the tile."""
    from relation_detr_amd import ops
    g_, calls = gen(6), 0
    B, C = 2, 256
    for pixels in tile_rows(64):
        levels = [dev(torch.randn(B, C, 1, pixels, generator=g_), dtype), dev(torch.randn(B, C, 3, 5, generator=g_), dtype)]
        vecs = [dev(torch.randn(C, generator=g_), dtype) for _ in levels]
        for out in slices((B, pixels + 15), C, dtype).values():
            assert ops.tokens_from_levels(levels, vecs, out=out).data_ptr() == out.data_ptr()
            calls += 1
    end(direct, "tokens_from_levels", calls)


def test_assign_match_out_slices(direct):
    """csrc/assign.hip: one workgroup solves one row of the match table, so the "tile" is one row: 1, 2 and 5 rows, with and without
    the denoising prefix, whose columns are written too."""
    from relation_detr_amd import criterion
    g_, calls = gen(7), 0
    N, Gmax = 37, 5
    for R in tile_rows(1):
        cost = dev(torch.rand(R, N, Gmax, generator=g_))
        count = dev(torch.tensor([3], dtype=torch.int32))
        for skip, meta in ((0, None), (6, (2, 3))):
            table = slices((R,), skip + N, torch.int32, pad_cols=4)
            for out in (table["columns"], table["rows"]):
                match, status = criterion.assign_match(cost, count, skip=skip, dn_meta=meta, out=out)
                assert match.data_ptr() == out.data_ptr() and tuple(match.shape) == (R, skip + N)
                calls += 1
    end(direct, "criterion.assign_match", calls)


def test_grad_value_from_head_major_out_slices(direct):
    """csrc/glue.hip (grad_value_from_head_major_kernel): 32 pixel rows per workgroup over the B * S rows of all images, which it
    addresses with ONE row stride: a column slice at B = 2 (the image boundary inside a tile), a row slice at B = 1, and the
    refusal of a row slice at B = 2, whose images are not evenly strided."""
    from relation_detr_amd import _lib, msda_train_hm
    g_, calls, refused = gen(8), 0, 0
    for S in tile_rows(32):
        for B, which in ((2, "columns"), (1, "rows")):
            grad = dev(torch.randn(B, 8, S, 32, generator=g_))
            mask = torch.zeros(B, S, dtype=torch.bool)
            mask[B - 1, S // 2:] = True
            mask = dev(mask)
            out = slices((B, S), 256, BF16)[which]
            assert msda_train_hm.grad_value_from_head_major(grad, mask, out=out).data_ptr() == out.data_ptr()
            calls += 1
        with pytest.raises(_lib.RdetrError, match="evenly strided"):
            msda_train_hm.grad_value_from_head_major(dev(torch.randn(2, 8, S, 32, generator=g_)), None, out=slices((2, S), 256, BF16)["rows"])
        refused += 1
    end(direct, "msda_train_hm.grad_value_from_head_major", calls, refused)


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "deterministic"])
def test_msda_backward_hm_merged_gradient_buffer(direct, deterministic):
    """csrc/msda_bwd.hip: one block of the backward serves 8 queries.  ``grad_producer_out`` [B, Nq, W] is contiguous by contract
    and wider than the 3n columns the kernel writes (the column slice); the row slice is a batch slice of a taller buffer; a
    buffer with strided rows is refused."""
    from relation_detr_amd import _lib, msda_train_hm
    calls, refused, B = 0, 0, 2
    for Nq in tile_rows(8):
        value, shp, start, off, lg, ref, go, _ = producer_inputs(B, Nq, SHAPES4, 2, seed=40 + Nq, dtype=BF16, nan=False)
        vh = dev(value.permute(0, 2, 1, 3).contiguous())
        shp, start, off, lg, ref, go = (dev(t) for t in (shp, start, off, lg, ref, go))
        n = 8 * len(SHAPES4) * 4
        wide = torch.empty(B, Nq, 3 * n + 10, dtype=BF16, device=DEV)
        tall = torch.empty(B + 2, Nq, 3 * n, dtype=BF16, device=DEV)
        for buf in (wide, tall[1:1 + B]):
            got = msda_train_hm.ms_deform_attn_backward_fused_hm(vh, shp, start, off, lg, ref, go, deterministic=deterministic,
                                                                 need_ref_grad=True, grad_producer_out=buf)
            assert got[1].data_ptr() == buf.data_ptr() and got[2].data_ptr() == buf[..., 2 * n:].data_ptr()
            calls += 1
        with pytest.raises(_lib.RdetrError, match="contiguous"):
            msda_train_hm.ms_deform_attn_backward_fused_hm(vh, shp, start, off, lg, ref, go, grad_producer_out=wide[..., :3 * n])
        refused += 1
    end(direct, "msda_train_hm.ms_deform_attn_backward_fused_hm", calls, refused)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_frozen_bn_act_forward_in_place_and_out(direct, dtype, channels_last):
    """csrc/backbone.hip: elementwise in 16-byte pieces (V = 8 bf16 / 4 fp32 elements); a plane (NCHW) or a pixel's channel run
    (channels-last) of 1, V - 1, V + 1 and 2 V + 3 elements.  ``out`` is dense by contract: ``out=x`` (in place, x counts as
    written through its byte range), a batch slice of a taller buffer (the row slice), and the refusal of a channel slice."""
    from relation_detr_amd.backbones import epilogue
    g_, calls, refused = gen(9), 0, 0
    V = 16 // torch.empty(0, dtype=dtype).element_size()
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    for n in tile_rows(V):
        B, C, H, W = (2, n, 3, 5) if channels_last else (2, 3, 1, n)
        scale, shift = dev(torch.rand(C, generator=g_) + 0.5), dev(torch.randn(C, generator=g_))
        src = torch.randn(B, C, H, W, generator=g_).to(dtype)
        x = torch.empty(B, C, H, W, dtype=dtype, device=DEV, memory_format=fmt).copy_(src)
        res = torch.empty_like(x).copy_(torch.randn(B, C, H, W, generator=g_).to(dtype))
        assert direct[0].of(x) is not None and direct[0].of(res) is not None and x.is_contiguous(memory_format=fmt)
        tall = torch.empty(8 + B + 3, C, H, W, dtype=dtype, device=DEV, memory_format=fmt)
        out = tall[8:8 + B]                                                   # eight images in: on the 16-byte grid whatever an image holds
        assert epilogue.frozen_bn_act_forward(x, scale, shift, res, out=out).data_ptr() == out.data_ptr()
        assert epilogue.frozen_bn_act_forward(x, scale, shift, None, relu=False, out=x) is x                 # in place
        calls += 2
        if C > 1 and H * W > 1:
            wide = torch.empty(B, C + 2, H, W, dtype=dtype, device=DEV, memory_format=fmt)
            with pytest.raises(ValueError, match="dense"):
                epilogue.frozen_bn_act_forward(x, scale, shift, out=wide[:, 1:1 + C])
            refused += 1
    end(direct, "backbones.epilogue.frozen_bn_act_forward", calls, refused)


# --------------------------------------------------------------------------------------------------- 3. the harness, on the device
def _past_the_end(name, call, args, result, fn):
    """One bf16 element behind the returned tensor's last one, through a byte view of its own guarded storage."""
    raw = shadow.storage_bytes(result)
    at = (result.storage_offset() + result.numel()) * result.element_size()
    raw[at:at + 2] = 0
    return result


def _flip_a_weight_bit(name, call, args, result, fn):
    args["weight"].view(torch.int16)[5, 7] ^= 1
    return result


def _neighbour_column(name, call, args, result, fn):
    out = args["out"]
    wide = out._base
    wide[2, out.storage_offset() - wide.storage_offset() + out.shape[1]] = 1.0       # the first column right of the slice, row 2
    return result


MISTAKES = {"past the end of a result": (_past_the_end, False, "back band of allocation"),
            "a bit of an operand": (_flip_a_weight_bit, False, "operand `weight` is not in the write set and changed in 1 elements"),
            "the neighbour column of out": (_neighbour_column, True, "2 bytes of the storage of `out` changed outside the view")}


def test_the_harness_reports_the_three_mistakes_on_the_device(monkeypatch):
    """Every write lands inside memory this test allocated (the guarded buffer of the result, the weight, the wide buffer around
    ``out``); nothing is launched out of bounds."""
    from relation_detr_amd import ops
    g_ = gen(10)
    x_host, w_host, b_host = torch.randn(37, 256, generator=g_), torch.randn(64, 256, generator=g_) * 0.05, torch.randn(64, generator=g_) * 0.1
    for label, (fault, with_out, said) in [("clean", (None, False, "")), ("clean, out=", (None, True, ""))] + list(MISTAKES.items()):
        with pytest.MonkeyPatch.context() as mp:
            g = guard.guard(mp)
            only_second = (lambda name, call, *rest: fault(name, call, *rest) if (name, call) == ("linear_k256", 1) else rest[1]) if fault else None
            sh = shadow.Shadow(mp, fault=only_second, writes=True, guard=g)
            x, w, b = dev(x_host, BF16), dev(w_host, BF16), dev(b_host, BF16)
            for call in range(3):                                             # the mistake is made in the second of three calls
                out = slices((37,), 64, BF16)["columns"] if with_out else None
                ops.linear_k256(x, w, b, out=out)
            ops.row_max(dev(torch.randn(5, 91, generator=g_)))                # another op in the same run stays clean
            torch.cuda.synchronize()
            bad = sh.failures()
            if fault is None:
                sh.assert_ok({"linear_k256", "row_max"})
                assert not bad and g.check() == [] and sh.write_checks["operand_bits"] > 0 and sh.write_checks["bands"] > 0, label
                assert sh.write_checks["outside_view"] > 0 or not with_out
                continue
            assert [(r.op, r.call, r.kind) for r in bad] == [("linear_k256", 1, "writes")], (label, bad)
            assert said in bad[0].where and bad[0].failing in (1, 2), (label, bad[0])
            if label == "past the end of a result":
                assert "(allocated in linear_k256)" in bad[0].where and "the nearest at +0" in bad[0].where
            with pytest.raises(AssertionError):
                sh.assert_ok()
            assert not sh.errors, label                                       # reported once, against the call: not again at the end
