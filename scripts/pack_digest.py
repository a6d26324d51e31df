#!/usr/bin/env python3
"""SHA-256 digests of what the host packs for the device-mode kernels.

Prints one JSON object. Two trees pack the same bytes iff their JSONs are
identical; used to compare a host-side refactor against its parent commit.
tests/golden/pack_digests.json is this script's output and
tests/test_pack_digests.py holds the code to it.

The ZMWs are those of the end-to-end test of tests/test_expand_device.py
(make_test_bams(n_zmws=4, length=350, seed=3), skip_windows_above 27). They
go through preprocess_one_zmw and pack_batch in four mode sets, each packed
plainly and with ``device_planes`` and ``pad_multiple``. Every named view of
FeaturizeBatch, SpacingBatch and ExpandBatch is digested (not the blob, whose
bytes between views are whatever np.empty left), with the offsets, the plane
layout and the host plane pieces.

``--pickle`` prints instead the summed ``len(pickle.dumps(ZmwWindows))`` per
mode set: what crosses the worker pool pipe.
"""
import hashlib
import json
import os
import pathlib
import pickle
import sys
import tempfile

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))
from deepconsensus_amd.inference import quick_inference as qi
from deepconsensus_amd.preprocess import featurize_device as fd
from deepconsensus_amd.preprocess import feeder as pre_feeder
from deepconsensus_amd.preprocess.windows import DcConfig

MODE_SETS = {
    "featurize": dict(featurize_mode="device", stitch_mode="serial"),
    "passthrough": dict(featurize_mode="device", stitch_mode="device",
                        passthrough_mode="device"),
    "spacing": dict(featurize_mode="device", stitch_mode="device",
                    passthrough_mode="device", spacing_mode="device"),
    "expand": dict(featurize_mode="device", stitch_mode="device",
                   passthrough_mode="device", spacing_mode="device",
                   expand_mode="device"),
}
PACKINGS = {
    "host": dict(),
    "device": dict(device_planes=True, pad_multiple=4),
}
SCALARS = ("n_windows", "n_rows", "max_length", "max_passes", "use_ccs_bq",
           "n_pt_bytes", "device_planes")


def _sha(array) -> str:
    a = np.ascontiguousarray(array)
    head = f"{a.dtype.str}{a.shape}".encode()
    return hashlib.sha256(head + a.tobytes()).hexdigest()


def _sha_json(value) -> str:
    return hashlib.sha256(
        json.dumps(value, sort_keys=True).encode()).hexdigest()


def preprocess(tmp_dir, modes):
    """ZmwWindows of the fixture's ZMWs under one mode set."""
    from test_io_and_pipeline import make_test_bams

    sub, ccs = make_test_bams(pathlib.Path(tmp_dir), n_zmws=4, length=350,
                              seed=3)
    options = qi.InferenceOptions(min_quality=0, skip_windows_above=27,
                                  batch_size=4, **modes)
    config = DcConfig(options.max_passes, options.max_length,
                      options.use_ccs_bq)
    feeder, _ = pre_feeder.create_proc_feeder(
        subreads_to_ccs=sub, ccs_bam=ccs, dc_config=config,
        defer_expansion=True)
    return [
        qi.preprocess_one_zmw((zmw, subreads, dcc, widths, options))
        for subreads, zmw, dcc, _, widths in feeder()
    ]


def digest_batch(batch) -> dict:
    out = {}
    for name in ("zmw_tab", "win_tab", "pt_tab", "ccs_bq", "sub", "ccs",
                 "ccs_q", "fallback_idx"):
        out[name] = _sha(getattr(batch, name))
    if batch.fallback_rows is not None:
        out["fallback_rows"] = _sha(batch.fallback_rows)
    out["offsets"] = _sha_json(batch.offsets)
    out["plane_layout"] = _sha_json({
        k: [int(lo), np.dtype(dtype).str, int(count)]
        for k, (lo, dtype, count) in batch.plane_layout.items()})
    out["host_planes"] = _sha_json([
        [name, int(off), _sha(array)]
        for name, off, array in batch.host_planes])
    out["scalars"] = _sha_json(
        {k: int(getattr(batch, k)) for k in SCALARS})
    sp = batch.spacing
    if sp is not None:
        for name in ("sp_tab", "read_tab", "ins_max", "src"):
            out[f"spacing/{name}"] = _sha(getattr(sp, name))
        out["spacing/offsets"] = _sha_json(sp.offsets)
        out["spacing/scalars"] = _sha_json(
            [int(sp.n_src), int(sp.n_src_host)])
        ex = sp.expand
        if ex is not None:
            for name in ("xr_tab", "op_tab", "raw"):
                out[f"expand/{name}"] = _sha(getattr(ex, name))
            out["expand/offsets"] = _sha_json(ex.offsets)
    return out


def compute() -> dict:
    out = {}
    with tempfile.TemporaryDirectory() as tmp_dir:
        for mode_name, modes in MODE_SETS.items():
            zmws = preprocess(tmp_dir, modes)
            for pack_name, kw in PACKINGS.items():
                batch = fd.pack_batch(zmws, **kw)
                for key, value in digest_batch(batch).items():
                    out[f"{mode_name}/{pack_name}/{key}"] = value
    return out


def pickle_sizes() -> dict:
    with tempfile.TemporaryDirectory() as tmp_dir:
        return {
            mode_name: sum(len(pickle.dumps(z))
                           for z in preprocess(tmp_dir, modes))
            for mode_name, modes in MODE_SETS.items()
        }


if __name__ == "__main__":
    result = pickle_sizes() if "--pickle" in sys.argv[1:] else compute()
    print(json.dumps(result, indent=1, sort_keys=True))
