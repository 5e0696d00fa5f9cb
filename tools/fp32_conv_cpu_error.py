"""How far torch's own CPU fp32 conv2d (forward, dx, dx + addend, dW) sits from float64 on the
inputs of tests/test_gpu_cnn_fp32.py::test_conv_f32_vs_float64 — the yardstick behind that test's
CONV_TOL (max-abs error over the float64 result's max-abs).  CPU only:

    python tools/fp32_conv_cpu_error.py
"""
import os
import sys

import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_cnn_fp32 as t  # noqa: E402


def main():
    worst = {}
    for name, *_ in t.CONV_GEOMS:
        c = t.conv_case(name)
        x = c["x"].clone().requires_grad_(True)
        w = c["w"].clone().requires_grad_(True)
        y = TF.conv2d(x, w, stride=c["s"], padding=c["p"])
        dx, dw = torch.autograd.grad(y, (x, w), c["dy"])
        e = {"fwd": t.mrel(y, c["y"]), "dgrad": t.mrel(dx, c["dx"]),
             "dgrad+addend": t.mrel(dx + c["addend"], c["dx"] + c["addend"].double()),
             "wgrad": t.mrel(dw, c["dw"])}
        print(name, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst", " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    print("4 x worst", f"{4 * max(worst.values()):.2e}", "(the test's bound is max(1e-5, this))")


if __name__ == "__main__":
    main()
