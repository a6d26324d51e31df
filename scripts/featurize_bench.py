#!/usr/bin/env python3
"""featurize_mode host vs device: worker cost and kernel time.

  --worker   any machine: preprocess_one_zmw ms/ZMW and pickled bytes per
             ZMW in both modes on a synthetic corpus (no model, no pool).
  --kernel   GPU: HIP-event time of window_featurize at N windows next to
             a device-to-device copy_ of an equally sized int16 tensor.
"""
import argparse
import os
import pickle
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def worker_main(args):
    from deepconsensus_amd.inference import quick_inference as qi
    from deepconsensus_amd.preprocess import feeder as pre_feeder
    from deepconsensus_amd.preprocess.windows import DcConfig
    from deepconsensus_amd.utils.synth import make_synth_bams

    with tempfile.TemporaryDirectory() as td:
        sub, ccs, _ = make_synth_bams(
            td, args.zmws, args.length, args.subreads, 3)
        dc_config = DcConfig(20, 100, False)
        for mode in ("host", "device", "host", "device"):
            options = qi.InferenceOptions(featurize_mode=mode)
            proc_feeder, _ = pre_feeder.create_proc_feeder(
                subreads_to_ccs=sub, ccs_bam=ccs, dc_config=dc_config,
                defer_expansion=True,
            )
            jobs = [(zmw, subreads, dcc, ww, options)
                    for subreads, zmw, dcc, _, ww in proc_feeder()]
            t0 = time.perf_counter()
            outs = [qi.preprocess_one_zmw(j) for j in jobs]
            work_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            blobs = [pickle.dumps(z, pickle.HIGHEST_PROTOCOL) for z in outs]
            for b in blobs:
                pickle.loads(b)
            pickle_s = time.perf_counter() - t0
            n = len(jobs)
            print(f"{mode:6s}: {1e3 * work_s / n:7.2f} ms/ZMW worker, "
                  f"{1e3 * pickle_s / n:6.2f} ms/ZMW pickle round trip, "
                  f"{sum(map(len, blobs)) / n / 1e3:8.1f} kB pickled/ZMW, "
                  f"{sum(z.n_model for z in outs) / n:.0f} model "
                  f"windows/ZMW ({n} ZMWs)")


def kernel_main(args):
    import torch

    from deepconsensus_amd import ops
    from deepconsensus_amd.preprocess import featurize_device as fd

    ext = ops.get_ext(required=True)
    mp, L, n_sub, W = 20, 100, args.subreads, 15000
    R = fd.tensor_height(mp, False)
    rng = np.random.default_rng(0)
    n_zmw = -(-args.windows // (W // L))
    tab = np.zeros((n_zmw, fd.TAB_FIXED + mp + 4), np.int64)
    tab[:, fd.TAB_SUB_OFF] = np.arange(n_zmw) * 3 * n_sub * W
    tab[:, fd.TAB_CCS_OFF] = np.arange(n_zmw) * W
    tab[:, fd.TAB_N_SUB] = n_sub
    tab[:, fd.TAB_W] = W
    tab[:, fd.TAB_FIXED : fd.TAB_FIXED + n_sub] = 1
    tab[:, fd.TAB_FIXED + mp :] = 12
    win = np.zeros((args.windows, 3), np.int32)
    win[:, 0] = np.arange(args.windows) // (W // L)
    win[:, 1] = (np.arange(args.windows) % (W // L)) * L
    win[:, 2] = L
    dev = [torch.from_numpy(a).cuda() for a in (
        rng.integers(0, 256, n_zmw * 3 * n_sub * W, dtype=np.uint8),
        rng.integers(0, 5, n_zmw * W, dtype=np.uint8),
        np.empty(0, np.int16), tab, win)]
    out = torch.empty((args.windows, R, L), dtype=torch.int16, device="cuda")
    src = torch.randint(0, 500, out.shape, dtype=torch.int16, device="cuda")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    k = timed(lambda: ext.window_featurize_into(*dev, out, mp, False))
    c = timed(lambda: out.copy_(src))
    gb = out.numel() * 2 / 1e9
    print(f"N={args.windows} R={R} L={L} n_sub={n_sub}: output {gb:.3f} GB, "
          f"{args.repeats} launches after {args.warmup} warm-up")
    print(f"window_featurize: median {k[0]:.3f} ms (min {k[1]:.3f}, max "
          f"{k[2]:.3f}) = {gb / k[0] * 1e3:.0f} GB/s written")
    print(f"d2d copy_       : median {c[0]:.3f} ms (min {c[1]:.3f}, max "
          f"{c[2]:.3f}) = {gb / c[0] * 1e3:.0f} GB/s written")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--zmws", type=int, default=20)
    ap.add_argument("--length", type=int, default=15000)
    ap.add_argument("--subreads", type=int, default=8)
    ap.add_argument("--windows", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=50)
    args = ap.parse_args()
    if args.worker:
        worker_main(args)
    if args.kernel:
        kernel_main(args)


if __name__ == "__main__":
    main()
