"""`deepconsensus eval`: evaluate a checkpoint over labeled TFRecords.

Parity with reference model_inference.py:79-145 /
model_utils.run_inference_and_write_results (:379-421): runs eval metrics
over a labeled dataset and writes inference.csv with one metric per row.
"""
from __future__ import annotations

import argparse
import json
import logging
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from deepconsensus_amd.models import checkpoint as ckpt_lib
from deepconsensus_amd.models import config as cfg
from deepconsensus_amd.models import data as data_lib
from deepconsensus_amd.models import losses as losses_lib
from deepconsensus_amd.models.model import get_model
from deepconsensus_amd.models.train import _prepare_batch
from deepconsensus_amd.utils import constants

log = logging.getLogger(__name__)


def ccs_path(path: str) -> str:
    """PATH with a `.ccs` infix: out.csv -> out.ccs.csv."""
    root, ext = os.path.splitext(path)
    return f"{root}.ccs{ext}"


class EmqEvaluator:
    """Feeds labeled batches through the serving path (InferenceRunner:
    native HIP on a GPU, torch on a CPU, `run`'s calibration and clamp)
    and accumulates the per-QV table and per-molecule emQ sums for the
    model and for the CCS input row."""

    def __init__(self, params, model, device, dc_calibration=None,
                 max_base_quality=None,
                 emq_thresholds: Sequence[float] = (20, 30, 40)):
        from deepconsensus_amd.calibration import window_calibration as wc
        from deepconsensus_amd.models.runner import InferenceRunner

        self._wc = wc
        if dc_calibration is None:
            dc_calibration = params.get("dc_calibration", "skip")
        self.dc_calibration = dc_calibration or "skip"
        self.max_base_quality = (
            constants.MAX_QUAL if max_base_quality is None
            else int(max_base_quality)
        )
        self.thresholds = tuple(emq_thresholds)
        self.params = params
        self.runner = InferenceRunner(
            params, model, device=device, calibration=self.dc_calibration,
            max_qual=self.max_base_quality,
        )
        self.acc_model = wc.WindowCalibrationAccumulator()
        self.acc_ccs = wc.WindowCalibrationAccumulator()

    def update(self, batch, rows: torch.Tensor, label: torch.Tensor):
        bases, quals = self.runner.forward_windows(rows)
        label_u8 = label.to(torch.uint8)
        name, pos = batch["name"], batch["window_pos"]
        self.acc_model.update(name, pos, label_u8, bases, quals)
        ccs_bases = rows[:, 4 * self.params.max_passes, :].to(torch.uint8)
        ccs_quals = torch.from_numpy(
            np.clip(batch["ccs_base_quality_scores"], 0, 255).astype(np.uint8)
        ).to(rows.device)
        self.acc_ccs.update(name, pos, label_u8, ccs_bases, ccs_quals)
        return bases, quals

    def result(self) -> dict:
        out = {
            "backend": self.acc_model.backend,
            "dc_calibration": self.dc_calibration,
            "max_base_quality": self.max_base_quality,
            "emq_thresholds": list(self.thresholds),
        }
        for key, acc in (("model", self.acc_model), ("ccs", self.acc_ccs)):
            out[key] = acc.yield_metrics(self.thresholds)
            out[key]["fitted_calibration"] = (
                self._wc.fit_linear_calibration(acc.hist)
            )
        for t in self.thresholds:
            k = f"yield@emQ{t:g}"
            denom = out["ccs"][k]
            out[f"{k}/ccs"] = out["model"][k] / denom if denom else None
        return out

    def write(self, calibration_csv: Optional[str],
              yield_json: Optional[str]) -> dict:
        result = self.result()
        if calibration_csv:
            os.makedirs(os.path.dirname(os.path.abspath(calibration_csv)),
                        exist_ok=True)
            self.acc_model.write_csv(calibration_csv)
            self.acc_ccs.write_csv(ccs_path(calibration_csv))
        if yield_json:
            os.makedirs(os.path.dirname(os.path.abspath(yield_json)),
                        exist_ok=True)
            with open(yield_json, "w") as f:
                json.dump(result, f, indent=2)
        return result


def run_inference(
    out_dir: str,
    checkpoint: str,
    eval_path: List[str],
    params: Optional[cfg.Params] = None,
    device: str = "cpu",
    limit: int = -1,
    calibration_csv: Optional[str] = None,
    yield_json: Optional[str] = None,
    dc_calibration: Optional[str] = None,
    max_base_quality: Optional[int] = None,
    emq_thresholds: Sequence[float] = (20, 30, 40),
) -> dict:
    if params is None:
        params = ckpt_lib.load_params(checkpoint)
        cfg.modify_params(params)
    model = get_model(params).to(device)
    if checkpoint != "random":
        ckpt_lib.load_checkpoint(checkpoint, model)
    model.eval()

    ds = data_lib.DatasetIterator(
        eval_path, params, params.batch_size, shuffle=False, limit=limit,
    )
    loss_fn = losses_lib.AlignmentLoss(
        del_cost=params.del_cost, loss_reg=params.loss_reg,
        width=params.get("band_width"), reduction="mean",
    )
    acc = losses_lib.PerExampleAccuracy()
    per_class = {
        v: losses_lib.PerClassAccuracy(k)
        for k, v in enumerate(" ATCG")
    }
    emq = None
    if calibration_csv or yield_json:
        emq = EmqEvaluator(params, model, device, dc_calibration,
                           max_base_quality, emq_thresholds)
    total_loss, n = 0.0, 0
    with torch.no_grad():
        for batch in ds.iterate():
            rows, label = _prepare_batch(batch, device)
            probs = model(rows, training=False)
            total_loss += float(loss_fn(label, probs.float()))
            n += 1
            acc.update_state(label.cpu(), probs.cpu())
            for m in per_class.values():
                m.update_state(label.cpu(), probs.cpu())
            if emq is not None:
                emq.update(batch, rows, label)
    metrics = {"loss": total_loss / max(n, 1),
               "per_example_accuracy": acc.result()}
    for sym, m in per_class.items():
        key = "gap_or_pad" if sym == " " else sym.lower()
        metrics[f"per_class_accuracy_{key}"] = m.result()

    os.makedirs(out_dir, exist_ok=True)
    csv_path = os.path.join(out_dir, "inference.csv")
    with open(csv_path, "w") as f:
        f.write("metric,value\n")
        for k, v in metrics.items():
            f.write(f"{k},{v}\n")
    log.info("wrote %s: %s", csv_path, metrics)
    if emq is not None:
        emq_result = emq.write(calibration_csv, yield_json)
        log.info("emQ: %s", emq_result)
    return metrics


def main(argv: Optional[List[str]] = None) -> None:
    ap = argparse.ArgumentParser("deepconsensus eval")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--eval_path", required=True)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--limit", type=int, default=-1)
    ap.add_argument("--device", default=None)
    ap.add_argument("--calibration_csv", default=None,
                    help="write the per-QV match/mismatch table of the "
                    "serving path here (and of CCS with a .ccs infix)")
    ap.add_argument("--yield_json", default=None,
                    help="write yield@emQ for model and CCS here")
    ap.add_argument("--dc_calibration", default=None,
                    help="threshold,w,b or skip (default: the checkpoint's)")
    ap.add_argument("--max_base_quality", type=int, default=None)
    ap.add_argument("--emq_thresholds", default="20,30,40")
    args = ap.parse_args(argv)
    device = args.device or (
        "cuda" if torch.cuda.is_available() else "cpu"
    )
    run_inference(args.out_dir, args.checkpoint, [args.eval_path],
                  device=device, limit=args.limit,
                  calibration_csv=args.calibration_csv,
                  yield_json=args.yield_json,
                  dc_calibration=args.dc_calibration,
                  max_base_quality=args.max_base_quality,
                  emq_thresholds=tuple(
                      float(t) for t in args.emq_thresholds.split(",")
                  ))


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
