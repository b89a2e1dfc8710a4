"""GPU tests of the short-row projection + residual + LayerNorm kernel (rdetr_linear_ln_rows_bf16, csrc/rowtail.hip) behind
ops.linear_ln_k256, and of the decoder route through it.

Rows 1, 31, 33 and 600 put the last row in a partial 32-row block (and 600 takes 19 workgroups).  K is 256 only: the K = d_ffn
form with a second LayerNorm (linear2 + norm3 + the decoder's norm) measured slower than the launches it replaced and was taken
out with its instantiations (csrc/rowtail.hip "dropped"), and its K = 512 / 2048 and `normed` cases with it.

  * `out` against float64 on the bf16 operand values within tests/shadow.py's chk_linear_ln_k256 bound, and against
    ops.add_layer_norm(residual, bf16(fp32 product)) within tests/test_gpu_glue.py's bound for the tall kernel;
  * `out_plus_pos` bit-equal to the bf16 sum of `out` and `pos`;
  * strided operands and outputs give the contiguous call's bits and touch nothing else (sentinel-filled buffers);
  * HIP-graph replay equals eager, and a second call into the same buffers leaves nothing stale;
  * the refusals; the 2-layer decoder of tests/test_gpu_decoder_absorb.py through the new route and with proj_ln off."""
import collections
import functools

import pytest
import torch
from torch.nn import functional as F

from test_gpu_decoder_absorb import FLOOR, _decoder_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
ROWS = (1, 31, 33, 600)
EPS = 1e-5
GUARD = -7.0                                           # exactly representable in bf16; no output of these inputs equals it


@functools.lru_cache(maxsize=None)
def case(rows, seed=0):
    """Operands and every reference of one row count, computed once.  LayerNorm parameters and the bias distinct from 1 / 0, as
    tests/test_gpu_shadow_stack.py::_ab_build makes them."""
    from relation_detr_amd import ops
    g = torch.Generator().manual_seed(1000 * rows + seed)
    K = 256
    t = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(BF).to(DEV)                  # noqa: E731
    d = dict(x=t(rows, K), res=t(rows, 256), pos=t(rows, 256), w=t(256, K, scale=K ** -0.5), b=t(256, scale=0.2))
    d["g1"] = (1.0 + 0.2 * torch.randn(256, generator=g)).to(BF).to(DEV)
    d["b1"] = (0.2 * torch.randn(256, generator=g)).to(BF).to(DEV)
    proj64 = d["x"].double() @ d["w"].double().t() + d["b"].double()
    s = d["res"].double() + proj64.float().to(BF).double()                     # the projection as the unfused route stores it
    d["ref64"] = F.layer_norm(s, (256,), d["g1"].double(), d["b1"].double(), EPS)
    proj32 = (d["x"].float() @ d["w"].float().t() + d["b"].float()).to(BF)
    d["ref_unfused"] = ops.add_layer_norm(d["res"], proj32, d["g1"], d["b1"], EPS)
    extra = {"pos": d["pos"]}
    d["out"] = ops.linear_ln_k256(d["x"], d["w"], d["b"], d["res"], d["g1"], d["b1"], EPS, extra=extra)
    d["out_plus_pos"] = extra["out_plus_pos"]
    assert extra["out"] is d["out"]
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("rows", ROWS)
def test_against_float64_and_the_unfused_route(rows):
    from relation_detr_amd import ops
    d = case(rows)
    out, ref = d["out"].double(), d["ref64"]
    err = (out - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -5 + 1e-3                           # chk_linear_ln_k256
    un = (d["out"].float() - d["ref_unfused"].float()).abs()
    print(f"rows {rows}: out vs float64 max err/bound {(err / bound).max().item():.3f}; vs GEMM + add_layer_norm max "
          f"{un.max().item():.4f} mean {un.mean().item():.2e}")
    assert torch.isfinite(out).all() and (err <= bound).all()
    assert un.max().item() <= 2.0 ** -5 and un.mean().item() <= 2e-4           # test_linear_ln_k256_is_linear_then_add_layer_norm
    assert torch.equal(d["out_plus_pos"], (d["out"].float() + d["pos"].float()).to(BF))
    # the instantiation without pos, and no bias: the same bits / the same bound
    assert torch.equal(ops.linear_ln_k256(d["x"], d["w"], d["b"], d["res"], d["g1"], d["b1"], EPS), d["out"])
    nb = ops.linear_ln_k256(d["x"], d["w"], None, d["res"], d["g1"], d["b1"], EPS).double()
    s = d["res"].double() + (d["x"].double() @ d["w"].double().t()).float().to(BF).double()
    ref_nb = F.layer_norm(s, (256,), d["g1"].double(), d["b1"].double(), EPS)
    assert ((nb - ref_nb).abs() <= 2.0 ** -8 * ref_nb.abs() + 2.0 ** -5 + 1e-3).all()


@pytest.mark.parametrize("rows", (33, 600))
def test_strided_operands_and_untouched_neighbours(rows):
    """x, residual, pos and the two outputs as column slices of wider buffers, with guard rows behind the last row."""
    from relation_detr_amd import ops
    d = case(rows)

    def wide(t, left, right):
        buf = torch.full((rows + 3, left + t.shape[1] + right), GUARD, dtype=BF, device=DEV)
        buf[:rows, left:left + t.shape[1]] = t
        return buf, buf[:rows, left:left + t.shape[1]]
    _, x = wide(d["x"], 8, 24)
    _, res = wide(d["res"], 256, 8)
    _, pos = wide(d["pos"], 16, 0)
    bufs = {k: wide(torch.full((rows, 256), GUARD, dtype=BF, device=DEV), l, r) for k, (l, r) in
            {"out": (0, 256), "out_plus_pos": (264, 8)}.items()}
    extra = {"pos": pos, "out_plus_pos": bufs["out_plus_pos"][1]}
    out = ops.linear_ln_k256(x, d["w"], d["b"], res, d["g1"], d["b1"], EPS, out=bufs["out"][1], extra=extra)
    assert out.data_ptr() == bufs["out"][1].data_ptr()
    for key, (buf, view) in bufs.items():
        assert torch.equal(view, d[key]), key
        probe = buf.clone()
        probe[:rows, view.storage_offset() % buf.shape[1]:view.storage_offset() % buf.shape[1] + 256] = GUARD
        assert (probe == GUARD).all(), f"{key}: written outside its rows / columns"


def test_graph_replay_and_no_stale_results():
    from relation_detr_amd import ops
    a, b = case(600), case(600, seed=1)
    bufs = {k: torch.empty(600, 256, dtype=BF, device=DEV) for k in ("out", "out_plus_pos")}

    def run(d):
        extra = {"pos": d["pos"], "out_plus_pos": bufs["out_plus_pos"]}
        ops.linear_ln_k256(d["x"], d["w"], d["b"], d["res"], d["g1"], d["b1"], EPS, out=bufs["out"], extra=extra)
    run(a)                                                                      # also packs the weight outside the capture
    run(b)
    for k in bufs:                                                              # the second call overwrote every element of the first
        assert torch.equal(bufs[k], b[k]), k
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(a)
    for t in bufs.values():
        t.fill_(GUARD)
    graph.replay()
    torch.cuda.synchronize()
    for k in bufs:
        assert torch.equal(bufs[k], a[k]), k


def test_refusals(monkeypatch):
    """Return codes of the C entry for a misaligned pointer or row stride and an empty problem -- none of them launches (a launch
    with these arguments would write: the output keeps its guard values); K != 256 and `extra` above the row threshold are
    refused by the ops entry, without a launch either."""
    from relation_detr_amd import _lib, ops, rowtail
    lib = _lib.load()
    d = case(33)
    out = torch.full((33, 256), GUARD, dtype=BF, device=DEV)
    packed = torch.zeros(256 * 256, dtype=BF, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def entry(x=d["x"].data_ptr(), ldx=256, M=33, res=d["res"].data_ptr(), pos=None, ldp=0):
        return lib.rdetr_linear_ln_rows_bf16(x, ldx, packed.data_ptr(), d["b"].data_ptr(), res, 256, d["g1"].data_ptr(), d["b1"].data_ptr(),
                                             EPS, pos, ldp, M, out.data_ptr(), 256, None if pos is None else out.data_ptr(), 256, st)
    assert entry(x=d["x"].data_ptr() + 2) == _lib.ERR_UNSUPPORTED
    assert entry(res=d["res"].data_ptr() + 8) == _lib.ERR_UNSUPPORTED
    assert entry(pos=d["pos"].data_ptr() + 4, ldp=256) == _lib.ERR_UNSUPPORTED
    assert entry(ldx=260) == _lib.ERR_UNSUPPORTED
    assert entry(ldx=128) == _lib.ERR_INVALID_ARG
    assert entry(pos=d["pos"].data_ptr(), ldp=128) == _lib.ERR_INVALID_ARG
    assert entry(M=-1) == _lib.ERR_INVALID_ARG
    assert entry(M=0) == 0
    torch.cuda.synchronize()
    assert (out == GUARD).all()
    rows = rowtail.MAX_ROWS + 1
    x, res = torch.zeros(rows, 256, dtype=BF, device=DEV), torch.zeros(rows, 256, dtype=BF, device=DEV)
    launched = collections.Counter()
    for sym in ("rdetr_linear_ln_rows_bf16", "rdetr_linear_ln_k256_bf16"):
        monkeypatch.setattr(lib, sym, lambda *a, sym=sym: launched.update([sym]) or 0)
    with pytest.raises(_lib.RdetrError, match="not supported above"):
        ops.linear_ln_k256(x, d["w"], d["b"], res, d["g1"], d["b1"], EPS, extra={"pos": res})
    x300, w300 = torch.zeros(33, 304, dtype=BF, device=DEV)[:, :300], torch.zeros(256, 300, dtype=BF, device=DEV)
    assert not ops.linear_ln_k256_supported(x300, w300, res[:33])
    with pytest.raises(_lib.RdetrError):
        ops.linear_ln_k256(x300, w300, d["b"], res[:33], d["g1"], d["b1"], EPS)
    with pytest.raises(_lib.RdetrError, match="unknown extra"):
        ops.linear_ln_k256(d["x"], d["w"], d["b"], d["res"], d["g1"], d["b1"], EPS, extra={"norm2": None})
    assert not launched
    ops.linear_ln_k256(x, d["w"], d["b"], res, d["g1"], d["b1"], EPS)          # above the threshold without extras: the tall kernel
    assert launched == {"rdetr_linear_ln_k256_bf16": 1}


# --------------------------------------------------------------------------------------------------------------------- decoder level
# what the parent commit launches for this 2-layer decoder call (one entry per rdetr_* symbol), which proj_ln = False must reproduce
# on freshly built modules: the 17 packing launches are the first call's (12 box-head and query-position weights, 3 in-projection
# blocks, 2 class heads)
PARENT_LAUNCHES = {"rdetr_add_layernorm_pos_bf16": 2, "rdetr_add_layernorm_strided_bf16": 6, "rdetr_box_head_cls_k256_bf16": 2,
                   "rdetr_decoder_reference": 2, "rdetr_linear_pack_k256_bf16": 17, "rdetr_msda_forward_fused_opt_bf16": 2,
                   "rdetr_query_pos_inproj_k256_bf16": 2, "rdetr_relation_attention_bf16": 1, "rdetr_relation_attention_boxes_bf16": 1}
PACK = "rdetr_linear_pack_k256_bf16"


def test_decoder_through_the_row_tails_against_the_library_route():
    """tests/test_gpu_decoder_absorb.py's rule -- the bound is relative to the route replaced: new <= 1.25 x library + that file's
    FLOOR, both against the fp32 CPU oracle -- and the launch counts of both routes."""
    import shadow
    from relation_detr_amd import options
    cpu, gpu, inputs = _decoder_case()
    with torch.no_grad():
        want_cls, want_box = cpu.decoder(**inputs)
    dev_in = {k: (v.to(DEV).to(BF) if k in ("query", "value") else v.to(DEV)) for k, v in inputs.items()}

    def run(proj_ln):
        options.apply(gpu, proj_ln=proj_ln)
        mp = pytest.MonkeyPatch()
        try:
            sh = shadow.Shadow(mp, check=False)
            with torch.no_grad():
                c, b = gpu.decoder(**dev_in)
            torch.cuda.synchronize()
        finally:
            mp.undo()
            options.apply(gpu, proj_ln=True)
        return c.float().cpu(), b.float().cpu(), +sh.launches
    lib_cls, lib_box, lib_launches = run(False)                                 # first: the modules are fresh, as in the parent's count
    new_cls, new_box, new_launches = run(True)
    print("launches, new route:", dict(sorted(new_launches.items())))
    print("launches, proj_ln = False:", dict(sorted(lib_launches.items())))
    for name, new, lib, want in (("classes", new_cls, lib_cls, want_cls), ("coords", new_box, lib_box, want_box)):
        e_new, e_lib = (new - want).abs().max().item(), (lib - want).abs().max().item()
        print(f"decoder {name} vs fp32 CPU oracle: row tails {e_new:.4e}, library route {e_lib:.4e}, "
              f"routes apart {(new - lib).abs().max().item():.4e}")
        assert e_new <= 1.25 * e_lib + FLOOR
    assert new_launches["rdetr_linear_ln_rows_bf16"] == 2 * 2                   # two tails per layer, two layers
    assert "rdetr_linear_ln_rows_bf16" not in lib_launches
    assert dict(lib_launches) == PARENT_LAUNCHES
    assert new_launches[PACK] == 2 * 2                                          # out_proj and output_proj of both layers, once
    gone = {k: v - new_launches[k] for k, v in lib_launches.items() if v != new_launches[k] and k != PACK}
    assert gone == {"rdetr_add_layernorm_pos_bf16": 2, "rdetr_add_layernorm_strided_bf16": 2}, gone      # norm2, norm1
