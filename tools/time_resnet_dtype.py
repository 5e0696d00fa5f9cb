"""ResNet-18 forward + backward time in the two storage modes of cnn.py (bf16 / fp32), and the
fp32 conv family's share of the fp32-MFMA peak.  For the record in DESIGN.md; no gate.

    python tools/time_resnet_dtype.py [--batch 32] [--iters 5]

Times cnn.ResNet18 (train mode, autograd forward + backward) at the cfg-3 inputs, 1x128x256 mels
and 3x224x224 covers, with hipEvents around ``iters`` steps after a warm-up; then each conv of the
fp32 mode alone (FWD, DGRAD, WGRAD at the network's shapes) for its FLOP rate.
"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("music-recommendation-multimodal_amd")
cnn, ops = pkg.cnn, pkg.ops
DEV = "cuda:0"
F32_MFMA_PEAK = 157.3e12      # MI355X fp32 matrix peak (v_mfma_f32_16x16x4_f32), FLOP/s


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters          # ms


def net_time(in_ch, H, W, B, dtype, iters):
    torch.manual_seed(0)
    net = cnn.ResNet18(in_ch, 128, dtype=dtype).to(DEV)
    x = torch.randn(B, in_ch, H, W, device=DEV)
    up = torch.randn(B, 128, device=DEV)

    def step():
        net.zero_grad(set_to_none=True)
        (net(x) * up).sum().backward()
    return timed(step, iters)


def conv_family(in_ch, H, W, B, iters):
    """Every conv of the fp32-mode network alone: (FLOPs, ms) summed per mode."""
    tot = {"fwd": [0.0, 0.0], "dgrad": [0.0, 0.0], "wgrad": [0.0, 0.0]}
    # input size of each conv: the stem sees the image; a block's conv1 and downsample see the
    # block input, its conv2 the block output
    blk_in = ops.conv_out_hw(*ops.conv_out_hw(H, W, 7, 2, 3), 3, 2, 1)
    blk_out = blk_in
    for sp in cnn.resnet18_convs(in_ch):
        C = max(sp.cin, 8)
        if sp.name == "conv1.weight":
            hi, wi = H, W
        elif sp.name.endswith(".conv1.weight"):
            blk_in = blk_out
            blk_out = ops.conv_out_hw(*blk_in, sp.k, sp.stride, sp.pad)
            hi, wi = blk_in
        elif sp.name.endswith(".conv2.weight"):
            hi, wi = blk_out
        else:
            hi, wi = blk_in
        ho, wo = ops.conv_out_hw(hi, wi, sp.k, sp.stride, sp.pad)
        x = torch.randn(B, hi, wi, C, device=DEV)
        dy = torch.randn(B, ho, wo, sp.cout, device=DEV)
        wt = torch.randn(sp.cout, sp.cin, sp.k, sp.k, device=DEV)
        wf = torch.empty(sp.cout, sp.k, sp.k, C, device=DEV)
        wd = torch.empty(C, sp.k, sp.k, sp.cout, device=DEV) if sp.cin >= 8 else None
        ops.conv_weight_prep(wt, C, wf, wd)
        y = torch.empty_like(dy)
        dx = torch.empty_like(x)
        dw = torch.zeros_like(wt)
        flops = 2.0 * B * ho * wo * sp.cout * sp.k * sp.k * sp.cin
        runs = {"fwd": lambda: ops.conv2d(ops.FWD, B, hi, wi, C, sp.cin, sp.cout, sp.k, sp.stride, sp.pad,
                                          x=x, w=wf, out=y),
                "wgrad": lambda: ops.conv2d(ops.WGRAD, B, hi, wi, C, sp.cin, sp.cout, sp.k, sp.stride, sp.pad,
                                            x=x, dy=dy, out=dw)}
        if wd is not None:
            runs["dgrad"] = lambda: ops.conv2d(ops.DGRAD, B, hi, wi, C, sp.cin, sp.cout, sp.k, sp.stride,
                                               sp.pad, dy=dy, w=wd, out=dx)
        for mode, fn in runs.items():
            ms = timed(fn, iters)
            tot[mode][0] += flops
            tot[mode][1] += ms
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    pkg.lib.load()
    for in_ch, H, W in ((1, 128, 256), (3, 224, 224)):
        t16 = net_time(in_ch, H, W, a.batch, torch.bfloat16, a.iters)
        t32 = net_time(in_ch, H, W, a.batch, torch.float32, a.iters)
        print(f"resnet18 fwd+bwd {in_ch}x{H}x{W} B={a.batch}: bf16 {t16:.2f} ms, fp32 {t32:.2f} ms "
              f"({t32 / t16:.1f}x)", flush=True)
        fam = conv_family(in_ch, H, W, a.batch, a.iters)
        fl = sum(v[0] for v in fam.values())
        ms = sum(v[1] for v in fam.values())
        for mode, (f, m) in fam.items():
            print(f"  fp32 conv {mode}: {f / 1e9:.1f} GFLOP in {m:.2f} ms = {f / m / 1e9:.1f} TFLOP/s "
                  f"({100 * f / (m * 1e-3) / F32_MFMA_PEAK:.1f}% of the fp32-MFMA peak)", flush=True)
        print(f"  fp32 conv family: {fl / ms / 1e9:.1f} TFLOP/s = "
              f"{100 * fl / (ms * 1e-3) / F32_MFMA_PEAK:.1f}% of {F32_MFMA_PEAK / 1e12:.1f} TFLOP/s", flush=True)


if __name__ == "__main__":
    main()
