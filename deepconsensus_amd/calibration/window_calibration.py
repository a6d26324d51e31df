"""Empirical QV calibration and emQ yield from labeled windows.

`deepconsensus calibrate` needs polished reads aligned to a genome. A
labeled window already has both sides of that alignment problem: the
truth label and the predicted (base, QV) pairs. This module aligns the
two with AlignmentMetric's PBMM2-like affine scores and walks the path
the way get_quality_calibration_stats walks a cigar: an aligned equal
base counts as a match in its QV bin, an aligned unequal base or an
inserted base as a mismatch, a deleted truth base as nothing.

Three layers:
  * window_calibration_numpy: the numpy twin built on
    AlignmentMetric.alignment's `paths` (oracle and CPU backend);
  * window_calibration: dispatch to ops/hip/alignment_calib.hip for CUDA
    tensors, the twin otherwise;
  * WindowCalibrationAccumulator: running table + per-molecule sums,
    `calibrate`-compatible CSV, yield@emQ, and a linear fit of the table.

Known bias: the alignment is per window, so a base that slid across a
window edge is charged as an insertion in one window (and a deletion in
its neighbour). The table is slightly pessimistic against a read-level
one.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from deepconsensus_amd.models import losses as losses_lib
from deepconsensus_amd.utils import constants

MAX_BASEQ = 100  # calibrate's table height

CLASS_NONE = 0
CLASS_MATCH = 1
CLASS_MISMATCH = 2
CLASS_INSERTION = 3

# The oracle materializes [2L-1, L, B] float64 wavefronts; bound its batch.
_TWIN_CHUNK = 256


def _as_numpy_u8(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x)).astype(np.uint8)


def _metric_values(counts: np.ndarray) -> Dict[str, np.ndarray]:
    """AlignmentMetric's mv dict from [B, 4] (matches, ins, del, correct)."""
    c = counts.astype(np.int64)
    mv = {
        "num_matches": c[:, 0],
        "num_insertions": c[:, 1],
        "num_deletions": c[:, 2],
        "num_correct_matches": c[:, 3],
    }
    mv["alignment_length"] = (
        mv["num_matches"] + mv["num_insertions"] + mv["num_deletions"]
    )
    with np.errstate(divide="ignore", invalid="ignore"):
        unsafe = mv["num_correct_matches"] / mv["alignment_length"]
    mv["pid"] = np.where(mv["alignment_length"] > 0, unsafe, 1.0)
    return mv


def _twin_chunk(label, bases, quals, metric):
    b, length = bases.shape
    onehot = np.eye(constants.SEQ_VOCAB_SIZE, dtype=np.float32)[bases]
    v_opt, paths, mv = metric.alignment(label, onehot)
    base_class = np.zeros((b, length), dtype=np.uint8)
    hist = np.zeros((MAX_BASEQ, 2), dtype=np.int64)
    for r in range(b):
        yt = label[r][label[r] != 0]
        pcol = np.nonzero(bases[r])[0]
        yp = bases[r][pcol]
        # paths[i, j]: 1 = M edge (pred j-1 on truth i-1), 2/3 = I edge
        # (pred j-1 alone), 4/5 = D edge (truth i-1 alone).
        mi, mj = np.nonzero(paths[r] == 1)
        equal = yt[mi - 1] == yp[mj - 1]
        base_class[r, pcol[mj - 1]] = np.where(
            equal, CLASS_MATCH, CLASS_MISMATCH
        )
        _, ij = np.nonzero((paths[r] == 2) | (paths[r] == 3))
        base_class[r, pcol[ij - 1]] = CLASS_INSERTION
    binned = quals < MAX_BASEQ
    np.add.at(hist[:, 0], quals[binned & (base_class == CLASS_MATCH)], 1)
    np.add.at(
        hist[:, 1],
        quals[binned & (base_class >= CLASS_MISMATCH)],
        1,
    )
    return v_opt, mv, base_class, hist


def window_calibration_numpy(
    label, bases, quals,
    metric: Optional[losses_lib.AlignmentMetric] = None,
) -> Tuple[np.ndarray, Dict[str, np.ndarray], np.ndarray, np.ndarray]:
    """Numpy twin of ops/hip/alignment_calib.hip.

    label, bases, quals: [B, L] in window coordinates (id 0 = gap, not
    left-shifted). Returns (v_opt [B], mv, base_class u8 [B, L],
    hist i64 [100, 2]); hist[q] = (matches, mismatches + insertions) of
    the bases carrying QV q; q >= 100 is dropped.
    """
    metric = metric or losses_lib.AlignmentMetric()
    label = _as_numpy_u8(label)
    bases = _as_numpy_u8(bases)
    quals = _as_numpy_u8(quals)
    if not (label.shape == bases.shape == quals.shape and label.ndim == 2):
        raise ValueError("label, bases and quals must share one [B, L] shape")
    b, length = bases.shape
    v_parts, count_parts = [], []
    base_class = np.zeros((b, length), dtype=np.uint8)
    hist = np.zeros((MAX_BASEQ, 2), dtype=np.int64)
    for lo in range(0, b, _TWIN_CHUNK):
        hi = min(lo + _TWIN_CHUNK, b)
        v, mv, cls, h = _twin_chunk(
            label[lo:hi], bases[lo:hi], quals[lo:hi], metric
        )
        v_parts.append(v)
        count_parts.append(np.stack(
            [mv["num_matches"], mv["num_insertions"], mv["num_deletions"],
             mv["num_correct_matches"]], axis=1,
        ))
        base_class[lo:hi] = cls
        hist += h
    v_opt = np.concatenate(v_parts) if v_parts else np.zeros(0)
    counts = (np.concatenate(count_parts) if count_parts
              else np.zeros((0, 4), dtype=np.int64))
    return v_opt, _metric_values(counts), base_class, hist


def _use_device(*tensors) -> bool:
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
        return False
    from deepconsensus_amd import ops as dc_ops

    return dc_ops.have_ext()


def window_calibration(
    label, bases, quals,
    metric: Optional[losses_lib.AlignmentMetric] = None,
):
    """(v_opt, mv, base_class, hist) as numpy; the HIP kernel for CUDA
    tensors when the extension is present, the numpy twin otherwise."""
    metric = metric or losses_lib.AlignmentMetric()
    if _use_device(label, bases, quals):
        from deepconsensus_amd import ops as dc_ops

        ext = dc_ops.get_ext(required=True)
        v_opt, counts, base_class, hist = ext.alignment_calib(
            label.to(torch.uint8), bases.to(torch.uint8),
            quals.to(torch.uint8),
            metric.matching_score, metric.mismatch_penalty,
            metric.gap_open_penalty, metric.gap_extend_penalty,
        )
        return (
            v_opt.cpu().numpy(),
            _metric_values(counts.cpu().numpy()),
            base_class.cpu().numpy(),
            hist.cpu().numpy(),
        )
    return window_calibration_numpy(label, bases, quals, metric)


def emq_reaches(correct: int, alignment_length: int, threshold: float) -> bool:
    """emQ = -10*log10(1 - correct/alignment_length) >= threshold,
    decided on the counts: errors * 10^(t/10) <= alignment_length. This
    keeps identity 0.99 / 0.999 exactly on Q20 / Q30, which the rounded
    logarithm does not; identity 1 (no errors) reaches every threshold."""
    errors = alignment_length - correct
    return errors * 10.0 ** (threshold / 10.0) <= alignment_length


def empirical_quality(correct: int, alignment_length: int) -> float:
    if alignment_length <= 0:
        return float("nan")
    if correct >= alignment_length:
        return float("inf")
    return -10.0 * math.log10(1.0 - correct / alignment_length)


def fit_linear_calibration(hist, min_count: int = 100) -> Optional[str]:
    """Fits emp_q = w*q + b over the table and returns "0,w,b".

    Bins with M + X >= min_count and X > 0 take part (a bin without a
    mismatch has no finite empirical quality); least squares weighted by
    M + X. None when fewer than two bins qualify.
    """
    hist = np.asarray(hist, dtype=np.float64)
    total = hist[:, 0] + hist[:, 1]
    use = (total >= min_count) & (hist[:, 1] > 0)
    if int(use.sum()) < 2:
        return None
    q = np.nonzero(use)[0].astype(np.float64)
    wt = total[use]
    emp_q = -10.0 * np.log10(hist[use, 1] / wt)
    q_mean = (wt * q).sum() / wt.sum()
    e_mean = (wt * emp_q).sum() / wt.sum()
    var = (wt * (q - q_mean) ** 2).sum()
    w = (wt * (q - q_mean) * (emp_q - e_mean)).sum() / var
    b = e_mean - w * q_mean
    return f"0,{float(w)!r},{float(b)!r}"


class WindowCalibrationAccumulator:
    """Running per-QV table and per-molecule sums over labeled windows."""

    def __init__(self, metric: Optional[losses_lib.AlignmentMetric] = None):
        self.metric = metric or losses_lib.AlignmentMetric()
        self.hist = np.zeros((MAX_BASEQ, 2), dtype=np.int64)
        # name -> [num_correct_matches, alignment_length, emitted bases]
        self.molecules: Dict[str, list] = {}
        self.n_windows = 0
        self.backend: Optional[str] = None

    def update(self, name, window_pos, label, bases, quals):
        """Feeds one batch; name / window_pos are per-window sequences."""
        del window_pos  # windows of a molecule simply add up
        backend = "device" if _use_device(label, bases, quals) else "numpy"
        if self.backend is None:
            self.backend = backend
        elif self.backend != backend:
            self.backend = "mixed"
        _, mv, base_class, hist = window_calibration(
            label, bases, quals, self.metric
        )
        self.hist += hist
        emitted = mv["num_matches"] + mv["num_insertions"]
        for r, nm in enumerate(name):
            if isinstance(nm, bytes):
                nm = nm.decode()
            m = self.molecules.setdefault(str(nm), [0, 0, 0])
            m[0] += int(mv["num_correct_matches"][r])
            m[1] += int(mv["alignment_length"][r])
            m[2] += int(emitted[r])
        self.n_windows += len(name)
        return mv, base_class

    def write_csv(self, path: str) -> None:
        """`deepconsensus calibrate`'s output format, rows 0..99."""
        with open(path, "w") as f:
            f.write("baseq,total_match,total_mismatch\n")
            for q in range(MAX_BASEQ):
                f.write(f"{q},{int(self.hist[q, 0])},{int(self.hist[q, 1])}\n")

    def yield_metrics(
        self, thresholds: Sequence[float] = (20, 30, 40)
    ) -> dict:
        """Bases emitted in molecules at or above each empirical quality."""
        out = {f"yield@emQ{t:g}": 0 for t in thresholds}
        n_empty = 0
        for correct, aln_len, emitted in self.molecules.values():
            if aln_len == 0:
                n_empty += 1
                continue
            for t in thresholds:
                if emq_reaches(correct, aln_len, t):
                    out[f"yield@emQ{t:g}"] += emitted
        out["n_molecules"] = len(self.molecules)
        out["n_molecules_empty"] = n_empty
        out["n_windows"] = self.n_windows
        out["emitted_bases"] = sum(m[2] for m in self.molecules.values())
        out["table_bases"] = int(self.hist.sum())
        return out
