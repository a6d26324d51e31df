#!/usr/bin/env python3
"""Whole-pipeline benchmark: `deepconsensus run` on synthetic BAMs.

Unlike bench.py (which times the serving step on pre-featurized windows),
this drives the COMPLETE production path — BAM reading, expand/spacing,
windowing, featurization, batched model execution, stitching, FASTQ
writing — and reports end-to-end ZMWs/sec. Synthetic subreads carry
insertions so the gap-aware spacing machinery does real work.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deepconsensus_amd.dcio import bam as bam_lib
from deepconsensus_amd.utils.synth import make_synth_bams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=100)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--subreads", type=int, default=8)
    # Worker forks copy the parent's page tables; beyond ~16 the pool
    # costs more to spin up than it returns for this workload.
    ap.add_argument("--cpus", type=int,
                    default=min(os.cpu_count() or 4, 16))
    ap.add_argument("--batch-size", type=int, default=2048)
    ap.add_argument("--batch-zmws", type=int, default=50)
    ap.add_argument("--device", default=None)
    # The synthetic CCS qualities are uniform in 20..39: a 100-column
    # window averages about Q26.2 (avg_phred), so 26 sends most windows
    # through the CCS passthrough and 0 (the default here) none.
    ap.add_argument("--skip_windows_above", type=int, default=0)
    ap.add_argument("--stitch_mode", default=None)
    ap.add_argument("--featurize_mode", default=None)
    ap.add_argument("--passthrough_mode", default=None)
    ap.add_argument("--spacing_mode", default=None)
    ap.add_argument("--expand_mode", default=None)
    args = ap.parse_args()

    import torch

    from deepconsensus_amd.inference import quick_inference as qi

    # Model / passthrough window counts of the run, from the worker output.
    n_windows = {"model": 0, "passthrough": 0}
    for fn in ("run_model_on_zmws", "run_model_and_stitch_on_zmws"):
        real = getattr(qi, fn)

        def counting(zmws, runner, options, real=real):
            n_windows["model"] += sum(z.n_model for z in zmws)
            n_windows["passthrough"] += sum(z.n_skipped for z in zmws)
            return real(zmws, runner, options)

        setattr(qi, fn, counting)

    # Deterministic random-init weights: success/only_gaps outcome
    # counts are then stable for a given device RNG.
    torch.manual_seed(1234)

    with tempfile.TemporaryDirectory() as td:
        t0 = time.perf_counter()
        sub, ccs, _ = make_synth_bams(td, args.zmws, args.length, args.subreads, 3)
        gen_s = time.perf_counter() - t0
        out = os.path.join(td, "out.fastq")
        options = qi.InferenceOptions(
            batch_size=args.batch_size, batch_zmws=args.batch_zmws,
            cpus=args.cpus, min_quality=0,
            skip_windows_above=args.skip_windows_above,
            stitch_mode=args.stitch_mode,
            featurize_mode=args.featurize_mode,
            passthrough_mode=args.passthrough_mode,
            spacing_mode=args.spacing_mode,
            expand_mode=args.expand_mode,
        )
        t0 = time.perf_counter()
        counter = qi.run(subreads_to_ccs=sub, ccs_bam=ccs,
                         checkpoint="random", output=out, options=options,
                         device=args.device)
        run_s = time.perf_counter() - t0
        print(f"generated {args.zmws} ZMWs x {args.subreads} subreads x "
              f"{args.length} bp in {gen_s:.1f}s")
        print(f"pipeline: {args.zmws / run_s:.2f} ZMW/s wall "
              f"({run_s:.1f}s, success={counter.success}, "
              f"cpus={args.cpus}, batch={args.batch_size})")
        total = max(sum(n_windows.values()), 1)
        print(f"windows: model={n_windows['model']} "
              f"passthrough={n_windows['passthrough']} "
              f"({100.0 * n_windows['passthrough'] / total:.1f}% "
              f"passthrough), modes: stitch={qi.resolve_stitch_mode(options)}"
              f" featurize={qi.resolve_featurize_mode(options)} "
              f"passthrough={qi.resolve_passthrough_mode(options)} "
              f"spacing={qi.resolve_spacing_mode(options)} "
              f"expand={qi.resolve_expand_mode(options)}")
        # Per-stage main-thread time (preprocess overlaps via the prefetch
        # thread, so its visible share should be ~0 when pipelining works).
        stage_s = {}
        with open(os.path.join(td, "out.runtime.csv")) as f:
            next(f)
            for line in f:
                parts = line.strip().split(",")
                stage_s[parts[1]] = stage_s.get(parts[1], 0.0) + float(
                    parts[2]
                )
        print("stage seconds (main thread): " + ", ".join(
            f"{k}={v:.2f}" for k, v in sorted(stage_s.items())))


if __name__ == "__main__":
    import logging

    logging.basicConfig(level=logging.INFO)
    main()
