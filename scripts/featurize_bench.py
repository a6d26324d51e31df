#!/usr/bin/env python3
"""featurize_mode host vs device: worker cost and kernel time.

  --worker   any machine: preprocess_one_zmw ms/ZMW and pickled bytes per
             ZMW in both modes on a synthetic corpus (no model, no pool).
  --kernel   GPU: HIP-event time of window_featurize at N windows next to
             a device-to-device copy_ of an equally sized int16 tensor.
  --worker --passthrough --skip_windows_above Q
             the same worker numbers for passthrough_mode host vs device.
  --passthrough-kernel
             GPU: HIP-event time of passthrough_fill_into at N windows next
             to a device-to-device copy_ of the same byte count.
  --worker --spacing_mode host|device
             the same worker numbers for one spacing_mode under
             featurize_mode device (alternate the two by hand); the host
             pass is split into decode, expand, spacing + put_spacing, and
             DcExample + build_planes + triage.
  --spacing-kernel
             GPU: HIP-event time of subread_space_into on --zmws ZMWs next
             to a device-to-device copy_ of the bytes it writes.
  --worker --spacing_mode device --expand_mode host|device
             the same split for one expand_mode; under device the subreads'
             share is build_raw.
  --expand-kernel
             GPU: HIP-event time of cigar_expand_into on --zmws ZMWs next to
             a device-to-device copy_ of the bytes it writes.
"""
import argparse
import collections
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
            if args.passthrough:
                # passthrough_mode host vs device under the device pipeline.
                options = qi.InferenceOptions(
                    featurize_mode="device", stitch_mode="device",
                    passthrough_mode=mode,
                    skip_windows_above=args.skip_windows_above)
            else:
                options = qi.InferenceOptions(
                    featurize_mode=mode,
                    skip_windows_above=args.skip_windows_above)
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
                  f"{sum(z.n_model for z in outs) / n:.0f} model + "
                  f"{sum(z.n_skipped for z in outs) / n:.0f} passthrough "
                  f"windows/ZMW ({n} ZMWs)")


def spacing_worker_main(args):
    """Worker cost of one spacing_mode: --passes passes over the corpus,
    the first one cold."""
    from deepconsensus_amd.dcio import bam
    from deepconsensus_amd.inference import quick_inference as qi
    from deepconsensus_amd.preprocess import feeder as pre_feeder
    from deepconsensus_amd.preprocess import read as read_lib
    from deepconsensus_amd.preprocess.windows import DcConfig
    from deepconsensus_amd.utils.synth import make_synth_bams

    mode = args.spacing_mode
    split = collections.defaultdict(float)

    def timed(name, fn):
        def wrapper(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                split[name] += time.perf_counter() - t0
        return wrapper

    # Nested timers: decode and expand run inside materialize, spacing
    # inside subreads_to_dc_example; the rest of preprocess_one_zmw is
    # DcExample + build_planes + triage (host) or build_unspaced + triage
    # (device).
    bam.decode_record = timed("decode", bam.decode_record)
    pre_feeder.expand_clip_indent = timed(
        "expand", pre_feeder.expand_clip_indent)
    pre_feeder.space_out_subreads = timed(
        "spacing+put_spacing", read_lib.space_out_subreads)
    # expand_mode device: neither decode nor expand runs for the subreads;
    # build_raw holds the record parse and the CCS decode.
    qi.expand_device.build_raw = timed(
        "build_raw", qi.expand_device.build_raw)

    with tempfile.TemporaryDirectory() as td:
        sub, ccs, _ = make_synth_bams(
            td, args.zmws, args.length, args.subreads, 3)
        dc_config = DcConfig(20, 100, False)
        options = qi.InferenceOptions(
            featurize_mode="device", stitch_mode="device",
            passthrough_mode=args.passthrough_mode, spacing_mode=mode,
            expand_mode=args.expand_mode,
            skip_windows_above=args.skip_windows_above)
        for p in range(args.passes):
            proc_feeder, _ = pre_feeder.create_proc_feeder(
                subreads_to_ccs=sub, ccs_bam=ccs, dc_config=dc_config,
                defer_expansion=True,
            )
            jobs = [(zmw, subreads, dcc, ww, options)
                    for subreads, zmw, dcc, _, ww in proc_feeder()]
            split.clear()
            t0 = time.perf_counter()
            outs = [qi.preprocess_one_zmw(j) for j in jobs]
            work_s = time.perf_counter() - t0
            blobs = [pickle.dumps(z, pickle.HIGHEST_PROTOCOL) for z in outs]
            n = len(jobs)
            rest = work_s - sum(split.values())
            parts = ", ".join(f"{k} {1e3 * v / n:.2f}"
                              for k, v in sorted(split.items()))
            unspaced = sum(getattr(z.planes, "unspaced", False)
                           for z in outs)
            raw = sum(getattr(z.planes, "raw_records", False) for z in outs)
            print(f"spacing={mode:6s} expand={args.expand_mode or 'host':6s} "
                  f"pass {p}: {1e3 * work_s / n:7.2f} "
                  f"ms/ZMW worker [{parts}, rest {1e3 * rest / n:.2f}], "
                  f"{sum(map(len, blobs)) / n / 1e3:8.1f} kB pickled/ZMW, "
                  f"{unspaced}/{n} ZMWs unspaced, {raw} of them raw")


def spacing_kernel_main(args):
    """subread_space_into on a packed batch of --zmws unspaced ZMWs next
    to a device-to-device copy_ of the plane bytes it fills."""
    import torch

    from deepconsensus_amd import ops
    from deepconsensus_amd.inference import quick_inference as qi
    from deepconsensus_amd.preprocess import featurize_device as fd
    from deepconsensus_amd.preprocess import feeder as pre_feeder
    from deepconsensus_amd.preprocess.windows import DcConfig
    from deepconsensus_amd.utils.synth import make_synth_bams

    ext = ops.get_ext(required=True)
    with tempfile.TemporaryDirectory() as td:
        sub, ccs, _ = make_synth_bams(
            td, args.zmws, args.length, args.subreads, 3)
        dc_config = DcConfig(20, 100, False)
        options = qi.InferenceOptions(
            featurize_mode="device", stitch_mode="device",
            spacing_mode="device", skip_windows_above=0)
        proc_feeder, _ = pre_feeder.create_proc_feeder(
            subreads_to_ccs=sub, ccs_bam=ccs, dc_config=dc_config,
            defer_expansion=True)
        outs = [qi.preprocess_one_zmw((zmw, subreads, dcc, ww, options))
                for subreads, zmw, dcc, _, ww in proc_feeder()]
    batch = fd.pack_batch(outs)
    sp = batch.spacing
    dev = [torch.from_numpy(a.copy()).cuda() for a in (
        sp.src, sp.ins_max.view(np.int16), sp.sp_tab, sp.read_tab,
        batch.zmw_tab)]
    col_ref = torch.empty(len(sp.ins_max), dtype=torch.int32, device="cuda")
    planes = [torch.zeros(len(a), dtype=getattr(torch, a.dtype.name),
                          device="cuda")
              for a in (batch.sub, batch.ccs, batch.ccs_q, batch.ccs_bq)]
    n_written = sum(3 * int(n) for n in sp.read_tab[:, 2]) + int(
        sp.sp_tab[:, 3].sum())
    n_planes = sum(p.numel() * p.element_size() for p in planes)
    src_copy = torch.empty(n_planes, dtype=torch.uint8, device="cuda")
    dst_copy = torch.empty_like(src_copy)

    def timed(fn):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    run = lambda: ext.subread_space_into(  # noqa: E731
        *dev, col_ref, *planes, batch.use_ccs_bq)
    copy = lambda: dst_copy.copy_(src_copy)  # noqa: E731
    for _ in range(args.warmup):
        run()
        copy()
    t = {"kernel": [], "copy": []}
    for _ in range(args.repeats):  # alternating, one process
        t["kernel"].append(timed(run))
        t["copy"].append(timed(copy))
    print(f"{len(outs)} ZMWs x {args.subreads} subreads x {args.length} bp:"
          f" {len(sp.src) / 1e6:.2f} MB unspaced source, {n_written / 1e6:.2f}"
          f" MB scattered into {n_planes / 1e6:.2f} MB of planes; "
          f"{args.repeats} launches each after {args.warmup} warm-up")
    for name, label in (("kernel", "subread_space_into (both phases)"),
                        ("copy", "copy_ of the plane bytes")):
        v = sorted(t[name])
        print(f"  {label:34s} median {statistics.median(v):8.1f} us  "
              f"min {v[0]:8.1f}  max {v[-1]:8.1f}")


def expand_kernel_main(args):
    """cigar_expand_into on a packed batch of --zmws raw ZMWs next to a
    device-to-device copy_ of the bytes it writes."""
    import torch

    from deepconsensus_amd import ops
    from deepconsensus_amd.inference import quick_inference as qi
    from deepconsensus_amd.preprocess import expand_device as xd
    from deepconsensus_amd.preprocess import featurize_device as fd
    from deepconsensus_amd.preprocess import feeder as pre_feeder
    from deepconsensus_amd.preprocess.windows import DcConfig
    from deepconsensus_amd.utils.synth import make_synth_bams

    ext = ops.get_ext(required=True)
    with tempfile.TemporaryDirectory() as td:
        sub, ccs, _ = make_synth_bams(
            td, args.zmws, args.length, args.subreads, 3)
        dc_config = DcConfig(20, 100, False)
        options = qi.InferenceOptions(
            featurize_mode="device", stitch_mode="device",
            spacing_mode="device", expand_mode="device",
            skip_windows_above=0)
        proc_feeder, _ = pre_feeder.create_proc_feeder(
            subreads_to_ccs=sub, ccs_bam=ccs, dc_config=dc_config,
            defer_expansion=True)
        outs = [qi.preprocess_one_zmw((zmw, subreads, dcc, ww, options))
                for subreads, zmw, dcc, _, ww in proc_feeder()]
    sp = fd.pack_batch(outs).spacing
    ex = sp.expand
    if ex is None:
        raise SystemExit("no ZMW took the expand path")
    dev = [torch.from_numpy(a.copy()).cuda()
           for a in (ex.raw, ex.op_tab, ex.xr_tab)]
    src = torch.zeros(sp.n_src, dtype=torch.uint8, device="cuda")
    lut = torch.from_numpy(xd.NT16_LUT.copy())
    n_written = 3 * int(ex.xr_tab[:, xd.XR_N].sum())
    src_copy = torch.randint(0, 255, (n_written,), dtype=torch.uint8,
                             device="cuda")
    dst_copy = torch.empty_like(src_copy)

    def timed(fn):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    run = lambda: ext.cigar_expand_into(*dev, src, lut)  # noqa: E731
    copy = lambda: dst_copy.copy_(src_copy)  # noqa: E731
    for _ in range(args.warmup):
        run()
        copy()
    torch.cuda.synchronize()
    t = {"kernel": [], "copy": []}
    for _ in range(args.repeats):  # alternating, one process
        t["kernel"].append(timed(run))
        t["copy"].append(timed(copy))
    print(f"{len(outs)} ZMWs x {args.subreads} subreads x {args.length} bp:"
          f" {len(ex.xr_tab)} reads, {len(ex.op_tab)} op rows, "
          f"{len(ex.raw) / 1e6:.2f} MB operands -> {n_written / 1e6:.2f} MB "
          f"written; {args.repeats} launches each after {args.warmup} "
          f"warm-up")
    for name, label in (("kernel", "cigar_expand_into"),
                        ("copy", "copy_ of the bytes written")):
        v = sorted(t[name])
        med = statistics.median(v)
        print(f"  {label:28s} median {med:8.1f} us  min {v[0]:8.1f}  "
              f"max {v[-1]:8.1f}  = {n_written / med / 1e3:7.1f} GB/s "
              f"written")


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


def passthrough_kernel_main(args):
    import torch

    from deepconsensus_amd import ops

    ext = ops.get_ext(required=True)
    L, W = 100, 15000
    P = args.windows
    rng = np.random.default_rng(0)
    n_zmw = -(-P // (W // L))
    tab = np.zeros((n_zmw, 5 + 20 + 4), np.int64)
    tab[:, 1] = np.arange(n_zmw) * W
    tab[:, 4] = W
    pt = np.zeros((P, 5), np.int32)
    pt[:, 0] = np.arange(P) // (W // L)
    pt[:, 1] = (np.arange(P) % (W // L)) * L
    pt[:, 2] = pt[:, 3] = L
    pt[:, 4] = np.arange(P) * L
    n = P * L
    base = 7 * L  # the region starts at a multiple of row_length only
    dev = [torch.from_numpy(a).cuda() for a in (
        rng.integers(0, 5, n_zmw * W, dtype=np.uint8),
        rng.integers(0, 95, n_zmw * W, dtype=np.uint8), tab, pt,
        np.minimum(np.arange(256), 93).astype(np.uint8))]
    acc = torch.empty((2, base + n), dtype=torch.uint8, device="cuda")
    src = torch.randint(0, 5, (2, n), dtype=torch.uint8, device="cuda")
    ms = {"kernel": [], "copy": []}

    def once(name, fn):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms[name].append(a.elapsed_time(b))

    def kernel():
        ext.passthrough_fill_into(*dev, acc[0, base:], acc[1, base:])

    def copy():
        acc[:, base:].copy_(src)

    for _ in range(args.warmup):
        kernel()
        copy()
    torch.cuda.synchronize()
    for _ in range(args.repeats):  # alternating, one process
        once("kernel", kernel)
        once("copy", copy)
    mb = 2 * n / 1e6
    print(f"P={P} windows x {L} columns: {mb:.2f} MB written (both rows), "
          f"{args.repeats} launches each after {args.warmup} warm-up, "
          f"alternating")
    for name, label in (("kernel", "passthrough_fill_into"),
                        ("copy", "d2d copy_ [2, n]     ")):
        v = ms[name]
        med = statistics.median(v)
        print(f"{label}: median {med * 1e3:.1f} us (min {min(v) * 1e3:.1f}, "
              f"max {max(v) * 1e3:.1f}) = {mb / med:.1f} GB/s written")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--passthrough-kernel", action="store_true",
                    help="GPU: passthrough_fill_into at N windows next to "
                    "a device-to-device copy_ of the same bytes")
    ap.add_argument("--passthrough", action="store_true",
                    help="with --worker: compare passthrough_mode host and "
                    "device (featurize and stitch mode device in both)")
    ap.add_argument("--spacing_mode", default=None,
                    choices=["host", "device"],
                    help="with --worker: worker cost and its split for this "
                    "spacing_mode (featurize_mode device)")
    ap.add_argument("--spacing-kernel", action="store_true",
                    help="GPU: subread_space_into on --zmws ZMWs next to "
                    "a copy_ of the plane bytes")
    ap.add_argument("--expand_mode", default=None,
                    choices=["host", "device"],
                    help="with --worker --spacing_mode device: the worker "
                    "cost under this expand_mode")
    ap.add_argument("--expand-kernel", action="store_true",
                    help="GPU: cigar_expand_into on --zmws ZMWs next to a "
                    "copy_ of the bytes it writes")
    ap.add_argument("--passthrough_mode", default="host",
                    choices=["host", "device"])
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--skip_windows_above", type=int, default=45)
    ap.add_argument("--zmws", type=int, default=20)
    ap.add_argument("--length", type=int, default=15000)
    ap.add_argument("--subreads", type=int, default=8)
    ap.add_argument("--windows", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=50)
    args = ap.parse_args()
    if args.worker and args.spacing_mode:
        spacing_worker_main(args)
        return
    if args.spacing_kernel:
        spacing_kernel_main(args)
        return
    if args.expand_kernel:
        expand_kernel_main(args)
        return
    if args.worker:
        worker_main(args)
    if args.kernel:
        kernel_main(args)
    if args.passthrough_kernel:
        passthrough_kernel_main(args)


if __name__ == "__main__":
    main()
