"""Time Swin's shifted-window attention with and without the fused kernel (csrc/attn_win.hip), alone and inside ``swin_l``.

    python tools/time_swin.py [--size 800x1344] [--batches 1,2,4] [--windows 7] [--iters 4] [--budget-seconds 600] [--out FILE]
                              [--no-operator] [--no-network]

The operator alone.  Swin-L's four stages at the given image size (window 7; heads 6 / 12 / 24 / 48; maps 200 x 336 ... 25 x 42 at
800 x 1344), each with the shift of an odd block (3, 3) and of an even one (0, 0), and ``swin_l_384``'s window 12 with shift (6, 6)
on the same maps.  ``fused`` is one ``ops.relation_attention(..., window=..., pad=...)`` call on the qkv GEMM's [B, H*W, 3C] output.
``torch`` is everything the reference runs around its two GEMMs for the same block (swin.py:133-221): pad, roll and window partition
of the C-channel input in front of the qkv GEMM; behind it the head permute, ``q * scale``, the scores, the bias gather and add, the
mask add, softmax, ``P V``, transpose; and behind the proj GEMM window reverse, roll back, unpad + contiguous.  Neither side runs
the qkv or the proj GEMM.  Achieved bytes per second count q, k, v and out once each (4 x B x H*W x C x 2 bytes) and are set
against 8 TB/s: the kernel's share of its memory bound; for ``torch`` the same bytes over its time, i.e. how far the chain is from it.

The network.  ``SwinTransformerBackbone("swin_l", return_indices=(1, 2, 3), freeze_indices=(0,))`` as a ``.to(bfloat16)`` model in eval
mode under ``no_grad``, ``fused=True`` against ``fused=False`` on the same module and input.

A point is timed as device events around windows of ``--iters`` runs behind a warm-up, the two routes ALTERNATING window by window;
reported are the median window per run and [min .. max].  ``fused`` wins a point when its slowest window is faster than the other
route's fastest (non-overlapping run sets).  ``--budget-seconds`` stops starting new points; what is left out is listed."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd import ops                                            # noqa: E402
from relation_detr_amd.backbones import SwinTransformerBackbone               # noqa: E402
from relation_detr_amd.backbones import window as wgeo                       # noqa: E402

DEV = "cuda:0"
PEAK = 8.0e12
BF16 = torch.bfloat16


def alternating_ms(fns, windows, iters, warmup=3):
    """{name: (median, min, max) ms per run}; the routes take turns window by window."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / iters)
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def torch_chain(x, qkv_windows, proj_windows, table, index, heads, H, W, wh, ww, sh, sw):
    """The reference's operators around the two GEMMs of one block; the GEMMs' results are given (``qkv_windows``, ``proj_windows``)."""
    B, _, _, C = x.shape
    xp = F.pad(x, (0, 0, 0, (ww - W % ww) % ww, 0, (wh - H % wh) % wh))
    _, pH, pW, _ = xp.shape
    if sh + sw > 0:
        xp = torch.roll(xp, shifts=(-sh, -sw), dims=(1, 2))
    nW = (pH // wh) * (pW // ww)
    N = wh * ww
    xw = xp.view(B, pH // wh, wh, pW // ww, ww, C).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, N, C)          # the qkv GEMM's input
    qkv = qkv_windows.reshape(xw.size(0), N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    q = q * (C // heads) ** -0.5
    attn = q.matmul(k.transpose(-2, -1))
    attn = attn + table[index].view(N, N, -1).permute(2, 0, 1).contiguous().unsqueeze(0)
    if sh + sw > 0:
        m = xw.new_zeros((pH, pW))
        count = 0
        for hs in ((0, -wh), (-wh, -sh), (-sh, None)):
            for ws in ((0, -ww), (-ww, -sw), (-sw, None)):
                m[hs[0]:hs[1], ws[0]:ws[1]] = count
                count += 1
        m = m.view(pH // wh, wh, pW // ww, ww).permute(0, 2, 1, 3).reshape(nW, N)
        m = m.unsqueeze(1) - m.unsqueeze(2)
        m = m.masked_fill(m != 0, float(-100.0)).masked_fill(m == 0, float(0.0))
        attn = (attn.view(B, nW, heads, N, N) + m.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    attn = F.softmax(attn, dim=-1)
    y = attn.matmul(v).transpose(1, 2).reshape(xw.size(0), N, C)                                             # the proj GEMM's input
    o = proj_windows.view(B, pH // wh, pW // ww, wh, ww, C).permute(0, 1, 3, 2, 4, 5).reshape(B, pH, pW, C)
    if sh + sw > 0:
        o = torch.roll(o, shifts=(sh, sw), dims=(1, 2))
    return y, o[:, :H, :W, :].contiguous()


def operator_points(args, size, emit, out_of_time):
    emit("# the attention operator alone: ms per call, fused | torch chain; GB/s = (q + k + v + out) bytes / median; share of 8 TB/s")
    lost, skipped = [], []
    g = torch.Generator().manual_seed(0)
    stages = [(i, 6 * 2 ** i, size[0] // (4 * 2 ** i), size[1] // (4 * 2 ** i)) for i in range(4)]
    for (wh, shifts) in ((7, ((3, 3), (0, 0))), (12, ((6, 6),))):
        for stage, heads, H, W in stages:
            for shift in shifts:
                for B in args.batches:
                    label = f"stage {stage} {H}x{W} heads {heads} window {wh} shift {shift[0]} B={B}"
                    if out_of_time():
                        skipped.append(label)
                        continue
                    C = 32 * heads
                    sh, sw = wgeo.effective_shift(H, W, wh, wh, *shift)
                    pH, pW = wgeo.padded_size(H, W, wh, wh)
                    nW, N = (pH // wh) * (pW // wh), wh * wh
                    x = torch.randn(B, H, W, C, generator=g).to(DEV, BF16)
                    qkv = torch.randn(B, H * W, 3 * C, generator=g).to(DEV, BF16)
                    qkv_windows = torch.randn(B * nW, N, 3 * C, generator=g).to(DEV, BF16)
                    proj_windows = torch.randn(B * nW, N, C, generator=g).to(DEV, BF16)
                    table = (torch.randn((2 * wh - 1) ** 2, heads, generator=g) * 0.5).to(DEV, BF16)
                    index = wgeo.bias_index(wh, wh).flatten().to(DEV)
                    pad = (torch.randn(C, generator=g).to(DEV, BF16), torch.randn(C, generator=g).to(DEV, BF16))
                    window = (H, W, wh, wh, sh, sw)
                    with torch.no_grad():
                        r = alternating_ms({
                            "fused": lambda: ops.relation_attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads, bias=table,
                                                                    window=window, pad=pad),
                            "torch": lambda: torch_chain(x, qkv_windows, proj_windows, table, index, heads, H, W, wh, wh, sh, sw)},
                            args.windows, args.iters)
                    nbytes = 4 * B * H * W * C * 2
                    (fm, flo, fhi), (tm, tlo, thi) = r["fused"], r["torch"]
                    if not fhi < tlo:
                        lost.append(label)
                    emit(f"{label:58s} fused {fm:8.4f} [{flo:.4f} .. {fhi:.4f}] {nbytes / fm / 1e6:7.0f} GB/s {nbytes / fm * 1e3 / PEAK:5.3f} | "
                         f"torch {tm:8.4f} [{tlo:.4f} .. {thi:.4f}] {nbytes / tm / 1e6:7.0f} GB/s {nbytes / tm * 1e3 / PEAK:5.3f}  ratio {tm / fm:6.2f}")
                    del x, qkv, qkv_windows, proj_windows
                    torch.cuda.empty_cache()
    return lost, skipped


def network_points(args, size, emit, out_of_time):
    emit("# swin_l, return_indices=(1, 2, 3), freeze_indices=(0,), bf16 model, eval: ms per forward, fused=True | fused=False")
    lost, skipped = [], []
    with torch.device(DEV):
        model = SwinTransformerBackbone("swin_l", return_indices=(1, 2, 3), freeze_indices=(0,))
    model = model.to(BF16).eval()
    g = torch.Generator().manual_seed(1)
    for B in args.batches:
        label = f"swin_l {size[0]}x{size[1]} B={B} bf16 eval"
        if out_of_time():
            skipped.append(label)
            continue
        x = torch.randn(B, 3, *size, generator=g).to(DEV, BF16)

        def run(fused):
            model.fused = fused
            with torch.no_grad():
                return model(x)
        r = alternating_ms({"fused": lambda: run(True), "torch": lambda: run(False)}, args.windows, max(1, args.iters // 2), warmup=2)
        model.fused = True
        (fm, flo, fhi), (tm, tlo, thi) = r["fused"], r["torch"]
        if not fhi < tlo:
            lost.append(label)
        emit(f"{label:36s} fused {fm:9.3f} [{flo:.3f} .. {fhi:.3f}] | torch {tm:9.3f} [{tlo:.3f} .. {thi:.3f}]  ratio {tm / fm:5.2f}")
        torch.cuda.empty_cache()
    return lost, skipped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="800x1344")
    ap.add_argument("--batches", default="1,2,4")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--budget-seconds", type=float, default=600.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-operator", action="store_true")
    ap.add_argument("--no-network", action="store_true")
    args = ap.parse_args()
    args.batches = [int(b) for b in args.batches.split(",")]
    size = tuple(int(v) for v in args.size.split("x"))
    if not torch.cuda.is_available():
        sys.exit("tools/time_swin.py times on the device: no GPU visible")
    started, sink = time.time(), open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    out_of_time = lambda: time.time() - started > args.budget_seconds                                      # noqa: E731
    emit(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {args.windows} windows x {args.iters} runs per route, alternating; "
         "median [min .. max] per run")
    lost, skipped = [], []
    if not args.no_network:                                   # first: the figure the default hangs on
        l, s = network_points(args, size, emit, out_of_time)
        lost, skipped = lost + l, skipped + s
    if not args.no_operator:
        l, s = operator_points(args, size, emit, out_of_time)
        lost, skipped = lost + l, skipped + s
    emit(f"# points where fused did not win with non-overlapping run sets: {lost if lost else 'none'}")
    emit(f"# points not measured (time budget of {args.budget_seconds:.0f} s): {skipped if skipped else 'none'}")


if __name__ == "__main__":
    main()
