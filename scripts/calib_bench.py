#!/usr/bin/env python3
"""Times alignment_calib against the K14 path it extends.

Same inputs for both: `alignment_calib` on window-coordinate uint8 rows,
and left_shift_sequence x2 + alignment_metric_counts (which returns the
four counts only). HIP events, the two alternated in one process, median
over --runs after warm-up. Prints one JSON line.

  python scripts/calib_bench.py --batch 4096 --length 100 --runs 50
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from deepconsensus_amd import ops as dc_ops
from deepconsensus_amd.models import losses as losses_lib


def make_inputs(batch: int, length: int, seed: int):
    """Truth with 20 % gaps; prediction = truth with 2 % substitutions,
    1 % dropped and 1 % spurious bases; QVs uniform in 0..93."""
    rng = np.random.default_rng(seed)
    label = rng.integers(1, 5, size=(batch, length)).astype(np.uint8)
    label[rng.random((batch, length)) < 0.2] = 0
    bases = label.copy()
    sub = rng.random((batch, length)) < 0.02
    bases[sub] = rng.integers(1, 5, size=int(sub.sum())).astype(np.uint8)
    bases[rng.random((batch, length)) < 0.01] = 0
    spurious = (label == 0) & (rng.random((batch, length)) < 0.05)
    bases[spurious] = rng.integers(
        1, 5, size=int(spurious.sum())
    ).astype(np.uint8)
    quals = rng.integers(0, 94, size=(batch, length)).astype(np.uint8)
    return label, bases, quals


def main(argv=None):
    ap = argparse.ArgumentParser("calib_bench")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("calib_bench needs a GPU")
    ext = dc_ops.get_ext(required=True)
    metric = losses_lib.AlignmentMetric()
    scores = (metric.matching_score, metric.mismatch_penalty,
              metric.gap_open_penalty, metric.gap_extend_penalty)
    label, bases, quals = (
        torch.from_numpy(a).cuda()
        for a in make_inputs(args.batch, args.length, args.seed)
    )

    def run_calib():
        return ext.alignment_calib(label, bases, quals, *scores)

    def run_k14():
        yt = losses_lib.left_shift_sequence(label.long()).int()
        yp = losses_lib.left_shift_sequence(bases.long()).int()
        return ext.alignment_metric_counts(
            yt, yp, (yt != 0).sum(-1).int(), (yp != 0).sum(-1).int(),
            *scores,
        )

    def timed(fn):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop), out

    for _ in range(args.warmup):
        run_calib()
        run_k14()
    torch.cuda.synchronize()
    t_calib, t_k14 = [], []
    for _ in range(args.runs):
        ms, out_c = timed(run_calib)
        t_calib.append(ms)
        ms, out_k = timed(run_k14)
        t_k14.append(ms)
    same = bool(torch.equal(out_c[1], out_k[1])
                and torch.equal(out_c[0], out_k[0]))
    result = {
        "batch": args.batch, "length": args.length, "runs": args.runs,
        "alignment_calib_ms_median": float(np.median(t_calib)),
        "alignment_calib_ms_min": float(np.min(t_calib)),
        "k14_path_ms_median": float(np.median(t_k14)),
        "k14_path_ms_min": float(np.min(t_k14)),
        "ratio_calib_over_k14": float(np.median(t_calib) / np.median(t_k14)),
        "counts_and_v_opt_equal": same,
        "table_bases": int(out_c[3].sum()),
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
