#!/usr/bin/env python3
"""SHA-256 digests of the raw outputs of fused_ln_head_qv (K10+K11+K12).

Prints one JSON object. Two builds compute the same thing bit for bit iff
their JSONs are identical; used to compare a change to how the kernel's
operands arrive against its parent commit. Inputs are drawn on the CPU
with fixed seeds. tests/golden/ln_head_digests.json is this script's output
on the wave-per-position kernel that re-loaded gamma / beta / w_head per row.
"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepconsensus_amd import ops as dc_ops

# 8197 > 4 * 2048: the persistent grid strides a second trip.
NS = (1, 3, 5, 257, 8197)
# (dtype, H): the serving shape, then one / two (partial) / eight slots.
WIDTHS = (("bf16", 280), ("fp32", 64), ("fp32", 100), ("fp32", 512))
# (threshold, w, b): calibration off, always on, on above QV 20.
CALIBS = ((-1.0, 1.0, 0.0), (0.0, 0.9, 1.5), (20.0, 1.1, -2.0))
MAX_QUAL = 40.0


def inputs(dtype, h, n):
    g = torch.Generator().manual_seed(7919 * h + n)
    # Rows with an offset well above their spread, and a scale that puts
    # the winning probability on both sides of the calibration threshold.
    x = torch.randn(n, h, generator=g) * 0.8 + torch.randn(n, 1, generator=g)
    x = x.to(torch.bfloat16 if dtype == "bf16" else torch.float32)
    gamma = 1.0 + 0.1 * torch.randn(h, generator=g)
    beta = 0.1 * torch.randn(h, generator=g)
    w_head = torch.randn(5, h, generator=g) * (4.0 / h ** 0.5)
    b_head = 0.2 * torch.randn(5, generator=g)
    return x, gamma, beta, w_head, b_head


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def compute(ext):
    out = {}
    for dtype, h in WIDTHS:
        for n in NS:
            ops = [t.cuda() for t in inputs(dtype, h, n)]
            for thr, cw, cb in CALIBS:
                bases, quals, probs = ext.fused_ln_head_qv(
                    *ops, thr, cw, cb, MAX_QUAL, True)
                key = f"{dtype}/H{h}/N{n}/thr{thr:g}"
                out[f"{key}/bases"] = digest(bases)
                out[f"{key}/quals"] = digest(quals)
                out[f"{key}/probs"] = digest(probs)
    torch.cuda.synchronize()
    return out


def main():
    out = compute(dc_ops.get_ext(required=True))
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
