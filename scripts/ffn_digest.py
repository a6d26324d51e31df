#!/usr/bin/env python3
"""SHA-256 digests of the raw output bytes of the 256-row FFN kernels.

Prints one JSON object. Two builds compute the same thing bit for bit iff
their JSONs are identical; used to compare a refactor against its parent
commit. Inputs are drawn on the CPU with fixed seeds (weights and x as in
tests/test_gpu_ffn_v5.py).
"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepconsensus_amd import ops as dc_ops

ALPHA = 0.7
MS = (1, 33, 255, 256, 257, 513)


def weights():
    g = torch.Generator().manual_seed(41)
    w1 = torch.zeros(2048, 296)
    w1[:, :280] = torch.randn(2048, 280, generator=g) * 0.05
    w1[:, 287] = torch.randn(2048, generator=g) * 0.1  # folded b1
    w2 = torch.zeros(320, 2048)
    w2[:280] = torch.randn(280, 2048, generator=g) * 0.05
    b2 = torch.zeros(320)
    b2[:280] = torch.randn(280, generator=g) * 0.1
    return w1.to(torch.bfloat16).cuda(), w2.to(torch.bfloat16).cuda(), b2.cuda()


def x_of(M, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, 280, generator=g) * 0.5).to(torch.bfloat16).cuda()


def digest(t):
    raw = t.contiguous().view(torch.int16).cpu().numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def main():
    ext = dc_ops.get_ext(required=True)
    w1, w2, b2 = weights()
    # dgrad weight images: W2^T as [2048, 296] (column 287 zero), W1^T as
    # padded [320, 2048].
    w2t = torch.zeros(2048, 296, dtype=torch.bfloat16, device="cuda")
    w2t[:, :280] = w2[:280].t()
    w1t = torch.zeros(320, 2048, dtype=torch.bfloat16, device="cuda")
    w1t[:280] = w1[:, :280].t()
    out = {}
    for M in MS:
        x = x_of(M, 1000 + M)
        out[f"v3/M{M}"] = digest(ext.fused_ffn_v3(x, w1, w2, b2, ALPHA))
        out[f"v5/M{M}/mb0"] = digest(ext.fused_ffn_v5(x, w1, w2, b2, ALPHA, 0))
    x = x_of(1297, 1000 + 1297)
    for mb in (1, 2, 4):
        out[f"v5/M1297/mb{mb}"] = digest(
            ext.fused_ffn_v5(x, w1, w2, b2, ALPHA, mb))
    for M in (257, 513):
        x, dy = x_of(M, 1000 + M), x_of(M, 2000 + M)
        for p, seed in ((0.0, 0), (0.25, 99)):
            y, hd = ext.ffn_train_fwd(x, w1, w2, b2, p, seed)
            dx, dh = ext.ffn_train_dgrad(dy, hd, w2t, w1t, p)
            nx, nh = ext.ffn_train_dgrad_nomask(dy, hd, w2t, w1t, p)
            key = f"train/M{M}/p{p}"
            for name, t in (("y", y), ("hd", hd), ("dx", dx), ("dh", dh),
                            ("nomask_dx", nx), ("nomask_dh", nh)):
                out[f"{key}/{name}"] = digest(t)
    torch.cuda.synchronize()
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
