#!/usr/bin/env python3
"""Training input benchmark: --input_mode host against device.

Builds a multi-file gzip TFRecord corpus of synthetic examples in the
production layout (85 x 100 x 1 fp32 subreads, a 100-float label, name,
window_pos, num_passes and the 100-entry ccs_base_quality_scores list) and
reports, for the two input modes, arms alternating over --rounds:

  * loader-only examples/s: the iterator drained, no model;
  * train steps/s: models/train.train_model on the corpus, timed from a
    batch hook between the first measured step and the last.

It then times the stages of a device-mode step in isolation (one reader's
gunzip + framing + scan + copy, the feeder's slot copy, the pinned upload,
the two kernels) and prints everything as JSON lines and as markdown tables
(--out). The resident-batch ceiling is scripts/train_bench.py, run in the
same session.
"""
import argparse
import gzip
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deepconsensus_amd.dcio import example_codec as codec  # noqa: E402
from deepconsensus_amd.dcio import tfrecord  # noqa: E402
from deepconsensus_amd.models import config as cfg  # noqa: E402
from deepconsensus_amd.models import data as data_lib  # noqa: E402
from deepconsensus_amd.models import data_device as dd  # noqa: E402

DISTINCT = 64  # distinct records; the corpus repeats them


def synth_record(rng, params, i):
    R, L, mp = params.total_rows, params.max_length, params.max_passes
    rows = np.zeros((R, L, 1), dtype=np.float32)
    rows[0:mp] = rng.integers(0, 5, size=(mp, L, 1))
    rows[mp:3 * mp] = rng.integers(0, 300, size=(2 * mp, L, 1))
    rows[3 * mp:4 * mp] = rng.integers(0, 3, size=(mp, L, 1))
    rows[4 * mp] = rng.integers(0, 5, size=(L, 1))
    rows[-4:] = rng.integers(5, 30, size=(4, 1, 1))
    label = rng.integers(0, 5, size=L).astype(np.float32)
    return codec.encode_example({
        "name": (codec.BYTES, [f"m64011_000000_000000/{i}/ccs".encode()]),
        "subreads/encoded": (codec.BYTES, [rows.tobytes()]),
        "subreads/shape": (codec.INT64, [R, L, 1]),
        "subreads/num_passes": (codec.INT64, [mp]),
        "window_pos": (codec.INT64, [100 * i]),
        "ccs_base_quality_scores": (
            codec.INT64, rng.integers(1, 94, size=L).tolist()),
        "label/encoded": (codec.BYTES, [label.tobytes()]),
        "label/shape": (codec.INT64, [L]),
    })


def frame(record):
    length = struct.pack("<Q", len(record))
    return b"".join([
        length, struct.pack("<I", tfrecord._masked_crc(length)), record,
        struct.pack("<I", tfrecord._masked_crc(record))])


def build_corpus(out_dir, params, n_files, per_file, prefix="train"):
    rng = np.random.default_rng(0)
    frames = [frame(synth_record(rng, params, i)) for i in range(DISTINCT)]
    for f in range(n_files):
        body = b"".join(frames[(f + i) % DISTINCT] for i in range(per_file))
        path = os.path.join(out_dir, f"{prefix}-{f:03d}.tfrecord.gz")
        with open(path, "wb") as fh:
            fh.write(gzip.compress(body, 1))
    return os.path.join(out_dir, f"{prefix}-*.tfrecord.gz"), len(frames[0])


def sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def loader_rate(mode, pattern, params, B, device, workers, max_batches):
    """examples/s from the first batch's arrival to the last one's."""
    from deepconsensus_amd.models.train import _prepare_batch

    if mode == "host":
        ds = data_lib.DatasetIterator([pattern], params, B, seed=1)
        it = (_prepare_batch(b, device) for b in ds.iterate(0))
    else:
        ds = dd.DeviceInputIterator([pattern], params, B, device=device,
                                    seed=1, input_workers=workers)
        it = ds.iterate(0)
    t_start = time.perf_counter()
    n = 0
    t_first = None
    for rows, _label in it:
        sync(device)
        n += 1
        if t_first is None:
            t_first = time.perf_counter()
        if n >= max_batches:
            break
    t_end = time.perf_counter()
    if hasattr(it, "close"):
        it.close()
    out = {"first_batch_s": t_first - t_start, "batches": n}
    if n > 1:
        out["examples_per_s"] = (n - 1) * B / (t_end - t_first)
    if mode == "device":
        out["wait_s_per_batch"] = ds.wait_s / max(n, 1)
        ds.close()
    return out


def train_rate(mode, train_pat, eval_pat, params_name, B, device, workers,
               steps, warm, bf16, buffer_size, n_train):
    from deepconsensus_amd.models import train as train_lib

    params = cfg.get_config(params_name)
    params.train_path = [train_pat]
    params.eval_path = [eval_pat]
    params.batch_size = B
    params.num_epochs = 1000
    params.buffer_size = buffer_size
    params.n_examples_train = n_train
    params.n_examples_eval = B
    cfg.modify_params(params)
    stamps = []

    def hook(rows, label):
        sync(device)
        stamps.append(time.perf_counter())

    with tempfile.TemporaryDirectory() as out_dir:
        train_lib.train_model(
            out_dir, params, device=device, eval_every=10 ** 9,
            limit_steps=warm + steps + 1, use_bf16=bf16, input_mode=mode,
            input_workers=workers, batch_hook=hook)
    # stamps[i] is taken when step i's batch is in hand, after step i-1 has
    # finished on the device: stamps[warm] .. stamps[warm + steps] spans
    # `steps` full steps, input included.
    dt = stamps[warm + steps] - stamps[warm]
    return {"steps_per_s": steps / dt, "examples_per_s": steps * B / dt}


def stage_split(pattern, params, B, device):
    """Stages of a device-mode step, each alone, per batch of B."""
    import glob

    path = sorted(glob.glob(pattern))[0]
    spec = dd.SlotSpec(params.total_rows, params.max_length)
    out = {}
    t0 = time.perf_counter()
    data = dd.read_file_bytes(path)
    t1 = time.perf_counter()
    spans = dd.frame_records(data, path)
    t2 = time.perf_counter()
    n = min(len(spans), 1024)
    buf = np.zeros((n, spec.slot_bytes), dtype=np.uint8)
    data_u8 = np.frombuffer(data, dtype=np.uint8)
    for i in range(n):
        dd.copy_record(data, data_u8, *spans[i], spec, buf[i], path, i)
    t3 = time.perf_counter()
    out["reader_gunzip_us_per_record"] = (t1 - t0) / len(spans) * 1e6
    out["reader_frame_us_per_record"] = (t2 - t1) / len(spans) * 1e6
    out["reader_scan_copy_us_per_record"] = (t3 - t2) / n * 1e6
    stage = np.zeros((n, spec.slot_bytes), dtype=np.uint8)
    planner = dd.ShufflePlanner(8, 1 << 30, True, 1, 0)
    t0 = time.perf_counter()
    for i in range(n):
        stage[i] = buf[i]
        planner.add()
    out["feeder_copy_plan_us_per_record"] = (
        (time.perf_counter() - t0) / n * 1e6)
    if torch.device(device).type != "cuda":
        return out
    from deepconsensus_amd import ops

    ext = ops.get_ext(required=True)
    S = dd.slot_floats(spec.R, spec.L)
    pinned = torch.zeros((B, S)).pin_memory()
    dev = torch.zeros((B, S), device=device)
    pool = torch.zeros((2 * B, S), device=device)
    rng = np.random.default_rng(0)
    gather = torch.from_numpy(
        rng.integers(0, 2 * B, size=B).astype(np.int32)).to(device)
    scatter = torch.from_numpy(
        rng.permutation(2 * B)[:B].astype(np.int32)).to(device)
    rows = torch.empty((B, spec.R, spec.L), device=device)
    label = torch.empty((B, spec.L), device=device)

    def timed(fn, reps=10):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    out["h2d_ms_per_batch"] = timed(
        lambda: dev.copy_(pinned, non_blocking=True))
    out["batch_assemble_ms_per_batch"] = timed(
        lambda: ext.batch_assemble_into(
            pool, dev, B, gather, rows, label, int(params.max_passes),
            bool(params.use_ccs_bq), float(params.PW_MAX),
            float(params.IP_MAX), float(params.SN_MAX), False))
    out["pool_store_ms_per_batch"] = timed(
        lambda: ext.pool_store(pool, dev, scatter))
    out["d2d_copy_same_bytes_ms"] = timed(
        lambda: rows.copy_(pool[:B, :spec.R * spec.L].view_as(rows)))
    out["batch_bytes"] = B * S * 4
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--records-per-file", type=int, default=1536)
    ap.add_argument("--buffer-size", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-loader-batches", type=int, default=3)
    ap.add_argument("--input_workers", type=int, default=None)
    ap.add_argument("--params", default="transformer_learn_values+custom")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--device", default=None)
    ap.add_argument("--out", default=None, help="markdown tables go here")
    args = ap.parse_args()
    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    B = args.batch_size
    workers = (dd.default_input_workers() if args.input_workers is None
               else args.input_workers)

    params = cfg.get_config(args.params)
    cfg.modify_params(params)
    params.buffer_size = args.buffer_size
    results = {"loader": {"host": [], "device": []},
               "train": {"host": [], "device": []}}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        pattern, rec_bytes = build_corpus(tmp, params, args.files,
                                          args.records_per_file)
        eval_pat, _ = build_corpus(tmp, params, 1, B, prefix="eval")
        n_train = args.files * args.records_per_file
        print(json.dumps({"corpus_records": n_train,
                          "record_bytes": rec_bytes, "files": args.files,
                          "build_s": time.perf_counter() - t0,
                          "input_workers": workers, "batch": B,
                          "device": device}), flush=True)
        for rnd in range(args.rounds):
            for mode in ("host", "device"):
                r = loader_rate(
                    mode, pattern, params, B, device, workers,
                    args.host_loader_batches if mode == "host" else 10 ** 9)
                results["loader"][mode].append(r)
                print(json.dumps({"what": "loader", "mode": mode,
                                  "round": rnd, **r}), flush=True)
        if not args.skip_train:
            for rnd in range(args.rounds):
                for mode in ("host", "device"):
                    r = train_rate(mode, pattern, eval_pat, args.params, B,
                                   device, workers, args.steps, args.warmup,
                                   args.bf16, args.buffer_size, n_train)
                    results["train"][mode].append(r)
                    print(json.dumps({"what": "train", "mode": mode,
                                      "round": rnd, **r}), flush=True)
        split = stage_split(pattern, params, B, device)
        print(json.dumps({"what": "stages", **split}), flush=True)

    if args.out:
        with open(args.out, "w") as f:
            f.write(f"batch {B}, {args.files} files x "
                    f"{args.records_per_file} records, buffer_size "
                    f"{args.buffer_size}, {workers} input workers, "
                    f"device {device}\n\n")
            for what, key in (("loader", "examples_per_s"),
                              ("train", "steps_per_s")):
                if not results[what]["host"]:
                    continue
                f.write(f"| {what} {key} | " + " | ".join(
                    f"round {i}" for i in range(args.rounds)) + " |\n")
                f.write("|---|" + "---|" * args.rounds + "\n")
                for mode in ("host", "device"):
                    f.write(f"| {mode} | " + " | ".join(
                        f"{r.get(key, float('nan')):.2f}"
                        for r in results[what][mode]) + " |\n")
                f.write("\n")
            f.write("| stage | value |\n|---|---|\n")
            for k, v in split.items():
                f.write(f"| {k} | {v:.3f} |\n")


if __name__ == "__main__":
    main()
