"""Micro-benchmark: fused_condense (K3+K4) vs hipBLASLt matmul + pos add.

Production serving shape: M = 16384*100 rows, K -> 280, pos [100, 280].
K is the concat width of the input layout (--k: 560 default, 568 = ccs_bq,
872 / 880 = max_passes 32 without / with ccs_bq).

The fused op and the fallback (x @ wt, then + pos) alternate in one
process; each call is timed with HIP events and the median of --iters
calls after --warmup warm-ups is reported, with the min..max spread of
each arm.
Run on a GPU box:  python scripts/condense_bench.py [--k 568]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from deepconsensus_amd import ops as dc_ops
from deepconsensus_amd.models.runner import build_condense_image


def time_alternating(fns, iters=50, warmup=10):
    """Per-call HIP-event times (us) of each fn, the fns taking turns."""
    times = [[] for _ in fns]
    for it in range(warmup + iters):
        for j, fn in enumerate(fns):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if it >= warmup:
                times[j].append(t0.elapsed_time(t1) * 1e3)
    return times


def summarize(ts):
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=560,
                    choices=[560, 568, 872, 880])
    ap.add_argument("--windows", type=int, default=16384,
                    help="batch of 100-position windows (M = windows*100)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()

    ext = dc_ops.get_ext(required=True)
    torch.manual_seed(0)
    K, L = args.k, 100
    M = args.windows * L
    x = (torch.randn(M, K, device="cuda") * 0.5).to(torch.bfloat16)
    w = torch.randn(280, K, device="cuda") * 0.05
    w_img = build_condense_image(w.cpu()).cuda()
    wt = w.to(torch.bfloat16).t().contiguous()
    pos = (torch.randn(L, 280, device="cuda") * 0.3).contiguous()
    pos_bf = pos.to(torch.bfloat16)

    def fused():
        return ext.fused_condense(x, w_img, pos, 280, L)

    def plain():
        y = (x @ wt).view(-1, L, 280)
        return y + pos_bf

    def mm():
        return x @ wt

    t_fused, t_plain, t_mm = time_alternating(
        [fused, plain, mm], args.iters, args.warmup
    )
    f_med, f_lo, f_hi = summarize(t_fused)
    p_med, p_lo, p_hi = summarize(t_plain)
    m_med, _, _ = summarize(t_mm)

    out = fused().float()
    idx = torch.arange(M, device="cuda") % L
    err = 0.0
    for r0 in range(0, M, 1 << 18):  # chunked: no second [M, 280] fp32 copy
        sl = slice(r0, min(M, r0 + (1 << 18)))
        ref = x[sl].float() @ w.t() + pos[idx[sl]]
        err = max(err, (out[sl] - ref).abs().max().item())
    print(
        f"fused_condense {f_med:.0f} us | hipBLASLt+add {p_med:.0f} us "
        f"(mm alone {m_med:.0f} us) | max err {err:.4f}"
    )
    print(
        f"K={K} M={M} median of {args.iters} after {args.warmup} warm-ups, "
        f"alternating | fused min..max {f_lo:.0f}..{f_hi:.0f} us | "
        f"fallback min..max {p_lo:.0f}..{p_hi:.0f} us | "
        f"fallback - fused = {p_med - f_med:.0f} us "
        f"(fallback spread {p_hi - p_lo:.0f} us)"
    )


if __name__ == "__main__":
    main()
