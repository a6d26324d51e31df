"""`deepconsensus run`: BAM -> polished FASTQ/BAM inference orchestrator.

Behavioral parity with reference quick_inference.py:238-984 — ZMW streaming,
multiprocess window preprocessing, skip-window fast path (overflow windows
and windows whose average CCS base quality exceeds --skip_windows_above adopt
the CCS sequence + calibrated CCS qualities), batched model execution,
stitching, FASTQ/BAM output with ec/np/rq/RG/zm tags, a per-stage runtime CSV
and an inference-stats JSON.

MI355X-native differences: the model path is the InferenceRunner HIP pipeline
(fused embed gather -> bf16 encoder with MFMA banded attention -> fused
LN+head+QV kernel), windows cross to the device as int16 tensors, and
preprocessing of the NEXT ZMW batch overlaps model execution of the current
one (the reference serialized these stages).
"""
from __future__ import annotations

import collections
import concurrent.futures
import dataclasses
import enum
import functools
import itertools
import json
import logging
import os
import time
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from deepconsensus_amd.calibration import calibration as calibration_lib
from deepconsensus_amd.inference import model_chunks as model_chunks_lib
from deepconsensus_amd.models import checkpoint as ckpt_lib
from deepconsensus_amd.models import config as cfg
from deepconsensus_amd.models.model import get_model
from deepconsensus_amd.models.runner import InferenceRunner
from deepconsensus_amd.postprocess import stitch as stitch_utils
from deepconsensus_amd.postprocess import stitch_device
from deepconsensus_amd.preprocess import featurize_device
from deepconsensus_amd.preprocess import feeder as pre_feeder
from deepconsensus_amd.preprocess import expand_device
from deepconsensus_amd.preprocess import spacing_device
from deepconsensus_amd.preprocess import windows as windows_lib
from deepconsensus_amd.preprocess.windows import DcConfig
from deepconsensus_amd.utils import constants, phred

log = logging.getLogger(__name__)


@enum.unique
class DebugStage(enum.Enum):
    """Stage to end after, for debugging and runtime testing
    (quick_inference.py:68-75)."""

    DC_INPUT = 1
    TF_EXAMPLES = 2
    RUN_MODEL = 3
    FULL = 4


@dataclasses.dataclass
class InferenceOptions:
    """Options shared across inference stages (quick_inference.py:238-275)."""

    max_length: int = 100
    example_height: int = 85
    max_passes: int = 20
    min_quality: int = 20
    min_length: int = 0
    batch_size: int = 1024
    use_ccs_bq: bool = False
    cpus: int = 0
    skip_windows_above: int = 45
    max_base_quality: int = constants.MAX_QUAL
    dc_calibration_values: calibration_lib.QualityCalibrationValues = (
        dataclasses.field(
            default_factory=lambda: calibration_lib.parse_calibration_string(
                "skip"
            )
        )
    )
    ccs_calibration_values: calibration_lib.QualityCalibrationValues = (
        dataclasses.field(
            default_factory=lambda: calibration_lib.parse_calibration_string(
                "skip"
            )
        )
    )
    batch_zmws: int = 100
    # ZMW batches preprocessed ahead of the model loop. >1 hides device/
    # runner startup (~20 s HIP context + extension init on a cold box)
    # and model-time jitter behind the worker pool; memory cost is
    # ~batch_zmws x windows x height x width x 2 bytes per slot.
    prefetch_batches: int = 3
    ins_trim: int = 0
    use_ccs_smart_windows: bool = False
    # ZMW sharding for multi-process / multi-GPU runs ("i/N", like the
    # reference's `ccs --chunk` sharding, docs/quick_start.md:216-248):
    # this process handles ZMWs with index % N == i.
    shard_index: int = 0
    shard_count: int = 1
    # Stop the pipeline early for debugging/runtime testing
    # (quick_inference.py:501,559,715).
    end_after_stage: DebugStage = DebugStage.FULL
    # Stitcher: "serial" | "pool" | "device". None reads DC_STITCH_MODE
    # (default "serial"). "device" gap-compacts the model output on the
    # GPU (postprocess/stitch_device.py) instead of building one
    # DCModelOutput per window.
    stitch_mode: Optional[str] = None
    # Featurizer: "host" | "device". None reads DC_FEATURIZE_MODE (default
    # "host"). "device" has the workers ship compact per-ZMW planes and
    # expands them into the model input on the GPU
    # (preprocess/featurize_device.py) instead of building one int16
    # matrix per window in the worker.
    featurize_mode: Optional[str] = None
    # CCS passthrough of skipped windows: "host" | "device". None reads
    # DC_PASSTHROUGH_MODE (default "host"). "device" has the workers ship
    # one passthrough table entry per skipped window instead of one
    # DCModelOutput, and fills the stitch buffer from the CCS planes on
    # the GPU. Only defined with featurize_mode and stitch_mode "device".
    passthrough_mode: Optional[str] = None
    # Subread spacing: "host" | "device". None reads DC_SPACING_MODE
    # (default "host"). "device" has the workers ship unspaced reads
    # (preprocess/spacing_device.py) and builds the per-ZMW planes on the
    # GPU instead of spacing every read in the worker. Only defined with
    # featurize_mode "device".
    spacing_mode: Optional[str] = None
    # Alignment expansion of the subread records: "host" | "device". None
    # reads DC_EXPAND_MODE (default "host"). "device" has the workers ship
    # the records' packed sequence, pw / ip arrays and an op table
    # (preprocess/expand_device.py) and expands them on the GPU instead of
    # decoding and expanding every record in the worker. Only defined with
    # spacing_mode "device".
    expand_mode: Optional[str] = None


STITCH_MODES = ("serial", "pool", "device")
FEATURIZE_MODES = ("host", "device")
PASSTHROUGH_MODES = ("host", "device")
SPACING_MODES = ("host", "device")
EXPAND_MODES = ("host", "device")

# The device stages: InferenceOptions field -> (environment knob read when
# the field is None, choices, default, modes that must be "device" for this
# one to be "device"). In the order `run` reports a bad value.
MODE_TABLE = {
    "featurize_mode": ("DC_FEATURIZE_MODE", FEATURIZE_MODES, "host", ()),
    "passthrough_mode": ("DC_PASSTHROUGH_MODE", PASSTHROUGH_MODES, "host",
                         ("featurize_mode", "stitch_mode")),
    "spacing_mode": ("DC_SPACING_MODE", SPACING_MODES, "host",
                     ("featurize_mode",)),
    "expand_mode": ("DC_EXPAND_MODE", EXPAND_MODES, "host",
                    ("spacing_mode",)),
    "stitch_mode": ("DC_STITCH_MODE", STITCH_MODES, "serial", ()),
}


class Modes(NamedTuple):
    """The five modes of a run, resolved and checked."""

    featurize_mode: str
    passthrough_mode: str
    spacing_mode: str
    expand_mode: str
    stitch_mode: str


def _resolve_mode(options: InferenceOptions, field: str) -> str:
    """The option if set, else the environment knob, else the default; a
    value outside the choices or a "device" without its prerequisites is a
    ValueError."""
    knob, choices, default, requires = MODE_TABLE[field]
    mode = getattr(options, field)
    if mode is None:
        mode = os.environ.get(knob, default)
        if field == "stitch_mode":
            return mode  # the knob's value has never been checked
    if mode not in choices:
        raise ValueError(f"{field} must be one of {choices}, got {mode!r}")
    if mode == "device" and requires:
        others = [_resolve_mode(options, r) for r in requires]
        if others != ["device"] * len(requires):
            needs = " and ".join(f"{r} 'device'" for r in requires)
            got = " and ".join(
                f"{r} {other!r}" for r, other in zip(requires, others))
            raise ValueError(f"{field} 'device' needs {needs}, got {got}")
    return mode


def resolve_modes(options: InferenceOptions) -> Modes:
    return Modes(*(_resolve_mode(options, field) for field in MODE_TABLE))


# One resolver per mode, for callers that ask for a single one.
(resolve_featurize_mode, resolve_passthrough_mode, resolve_spacing_mode,
 resolve_expand_mode, resolve_stitch_mode) = (
    functools.partial(_resolve_mode, field=field) for field in MODE_TABLE)


@dataclasses.dataclass
class ZmwWindows:
    """Worker output for one ZMW: model windows pre-stacked, skipped
    windows pre-resolved to DCModelOutput.

    The reference crossed the pool boundary with one feature dict per
    window and ran skip triage + CCS passthrough serially
    (quick_inference.py:655-677). Here the worker does the triage
    (avg-Phred + overflow), builds the CCS passthrough outputs, and
    stacks the model-bound windows into ONE int16 [n, R, L] array — the
    serial batch loop only concatenates arrays and runs the model.
    """

    name: str
    window_pos: np.ndarray  # [n_model] int64, model-bound windows only
    rows: Optional[np.ndarray]  # [n_model, R, L] int16, format_rows'd
    skipped: List["stitch_utils.DCModelOutput"]
    counter: collections.Counter
    ec: Optional[float] = None
    np_num_passes: Optional[int] = None
    rq: Optional[float] = None
    rg: Optional[str] = None
    # featurize_mode "device": the model-bound windows as a window table
    # over compact planes (a ZmwPlanes); ``rows`` is then None.
    # passthrough_mode "device": the tables also carry the skipped windows
    # (``skipped`` is then empty), and stay when no window is model-bound.
    # spacing_mode "device": over unspaced reads (a ZmwUnspaced);
    # expand_mode "device": over undecoded records (a ZmwRaw).
    planes: Optional[featurize_device.ZmwTables] = None

    @property
    def n_model(self) -> int:
        return featurize_device.n_model_windows(self)

    @property
    def n_skipped(self) -> int:
        """Skipped windows, as objects or as passthrough table entries."""
        return len(self.skipped) + featurize_device.n_table_passthrough(self)

    @property
    def n_examples(self) -> int:
        return self.n_skipped + self.n_model


def preprocess_one_zmw(one_zmw) -> ZmwWindows:
    """Windows + counters for one ZMW (quick_inference.py:535-564).

    ``subreads`` may be a deferred ZmwJob/RawZmwJob (raw BAM records):
    record decode and expansion then run HERE — i.e. in the worker
    pool — instead of the serial feeder.
    """
    zmw, subreads, dc_config, window_widths, options = one_zmw
    stage = options.end_after_stage
    modes = resolve_modes(options)
    expand_counter = None
    if isinstance(subreads, pre_feeder.ZmwJob):
        expand_counter = collections.Counter()
        if stage != DebugStage.DC_INPUT and modes.expand_mode == "device":
            # No record is decoded or expanded here. None for a ZMW off
            # this path: it is materialized below, as in expand_mode "host".
            raw = expand_device.build_raw(
                subreads, dc_config, window_widths, subreads.ins_trim,
                expand_counter,
            )
            if raw is not None:
                ccs, raw.ccs_read = raw.ccs_read, None
                return _unspaced_zmw_windows(
                    zmw, raw, ccs, options, modes, expand_counter
                )
        subreads = subreads.materialize(expand_counter)
    if (stage != DebugStage.DC_INPUT and modes.spacing_mode == "device"
            and isinstance(subreads, list)):
        # No read is spaced here. None for a ZMW off this path: it is
        # spaced below and ships planes, as in spacing_mode "host".
        fallback_counter = collections.Counter()
        unspaced = spacing_device.build_unspaced(
            subreads[:-1], subreads[-1], dc_config, window_widths,
            fallback_counter,
        )
        if unspaced is not None:
            return _unspaced_zmw_windows(
                zmw, unspaced, subreads[-1], options, modes, expand_counter
            )
        expand_counter = (expand_counter or collections.Counter())
        expand_counter.update(fallback_counter)
    dc_whole = pre_feeder.subreads_to_dc_example(
        subreads=subreads,
        ccs_seqname=zmw,
        dc_config=dc_config,
        window_widths=window_widths,
    )
    empty = ZmwWindows(name=zmw, window_pos=np.empty(0, np.int64),
                       rows=None, skipped=[], counter=dc_whole.counter)
    if stage == DebugStage.DC_INPUT:
        if expand_counter:
            empty.counter.update(expand_counter)
        return empty
    ccs = dc_whole.ccs
    planes = None
    if modes.featurize_mode == "device":
        # None for a ZMW off the fast path: it keeps the host rows.
        planes = featurize_device.build_planes(dc_whole)
    if planes is not None:
        # Same windows, counters and triage as below; a model-bound
        # window is two table entries instead of an [R, L] matrix.
        # Device passthrough: a skipped window is a table entry as well,
        # when the ZMW's CCS qualities fit the uint8 code.
        if modes.passthrough_mode == "device":
            planes.ccs_q = featurize_device.encode_ccs_qualities(
                ccs.base_quality_scores
            )
            if (planes.ccs_q is not None
                    and planes.ccs_q.shape != planes.ccs.shape):
                planes.ccs_q = None
        return _plane_zmw_windows(
            zmw, planes, dc_whole.iter_window_specs(), planes.ccs,
            planes.ccs_q is not None, dc_whole.name, ccs, options,
            dc_whole.counter, expand_counter,
        )
    # Worker-side finishing, keeping the serial batch loop thin: the
    # fast path applies format_rows' PW/IP/SN clipping at ZMW level and
    # emits int16 matrices directly (integral-after-truncation for the
    # model — the embedding casts to int, SN fractions truncate
    # identically — and int16 halves the pickle + H2D volume).
    model_rows: List[np.ndarray] = []
    window_pos: List[int] = []
    skipped: List[stitch_utils.DCModelOutput] = []
    for f in dc_whole.iter_feature_dicts(
        pw_max=featurize_device.PW_MAX, ip_max=featurize_device.IP_MAX,
        sn_max=featurize_device.SN_MAX,  # config.py:89-92 defaults
        out_dtype=np.int16,
    ):
        if _skip_window(
            f["overflow"], f["ccs_base_quality_scores"], options
        ):
            skipped.append(process_skipped_window(f, options))
            continue
        model_rows.append(f["subreads"][:, :, 0])
        window_pos.append(int(f["window_pos"]))
    counter = dc_whole.counter
    if expand_counter:
        counter.update(expand_counter)
    return ZmwWindows(
        name=zmw,
        window_pos=np.asarray(window_pos, np.int64),
        rows=np.stack(model_rows) if model_rows else None,
        skipped=skipped,
        counter=counter,
        ec=ccs.ec, np_num_passes=ccs.np_num_passes, rq=ccs.rq, rg=ccs.rg,
    )


def _plane_zmw_windows(zmw, planes, specs, ccs_ids, table_ok, name, ccs,
                       options: InferenceOptions, counter,
                       expand_counter) -> ZmwWindows:
    """ZmwWindows of a ZMW on the plane path, shared by spaced planes and
    unspaced ZMWs: skip triage over the window ``specs`` into the window
    table and the passthrough table of ``planes``.

    ``ccs_ids`` are the spaced CCS base ids. A skipped window becomes a
    passthrough table entry when ``table_ok`` (device passthrough and CCS
    qualities that fit the uint8 code), an object under ``name`` otherwise.
    ``counter`` holds the window counters; ``expand_counter`` joins it.
    """
    win_start: List[int] = []
    win_w: List[int] = []
    window_pos: List[int] = []
    skipped: List[stitch_utils.DCModelOutput] = []
    pt: List[Tuple[int, int, int, int]] = []
    for spec in specs:
        if _skip_window(spec.overflow, spec.bq, options):
            if table_ok:
                pt.append(
                    (spec.start, spec.w, spec.width, spec.window_pos)
                )
                continue
            ids = np.zeros(spec.width, np.uint8)
            ids[: spec.w] = ccs_ids[spec.start : spec.start + spec.w]
            skipped.append(_passthrough_output(
                ids, spec.bq, spec.window_pos, name,
                ccs.ec, ccs.np_num_passes, ccs.rq, ccs.rg, options,
            ))
            continue
        win_start.append(spec.start)
        win_w.append(spec.w)
        window_pos.append(spec.window_pos)
    planes.win_start = np.asarray(win_start, np.int32)
    planes.win_w = np.asarray(win_w, np.int32)
    if pt:
        cols = np.asarray(pt, np.int64).T
        planes.pt_start, planes.pt_w, planes.pt_width = (
            c.astype(np.int32) for c in cols[:3]
        )
        planes.pt_pos = cols[3]
    planes.need_q(bool(pt))  # only a passthrough table reads the ccs_q plane
    if not win_start:
        # Without model windows only the passthrough table needs the
        # planes, and of them only the CCS row.
        planes = planes.without_subreads() if pt else None
    if expand_counter:
        counter.update(expand_counter)
    return ZmwWindows(
        name=zmw,
        window_pos=np.asarray(window_pos, np.int64),
        rows=None,
        skipped=skipped,
        counter=counter,
        ec=ccs.ec, np_num_passes=ccs.np_num_passes, rq=ccs.rq, rg=ccs.rg,
        planes=planes,
    )


def _unspaced_zmw_windows(zmw, unspaced, ccs, options: InferenceOptions,
                          modes: Modes, expand_counter) -> ZmwWindows:
    """ZmwWindows of a ZMW that ships unspaced (spacing_mode "device"):
    windows, counters and triage from the CCS row, which follows from
    ``ins_max`` before any read is spaced."""
    ccs_ids, ccs_idx, ccs_bq, ccs_width = spacing_device.spaced_ccs_row(
        unspaced, ccs.ccs_idx
    )
    counter = collections.Counter()
    specs = windows_lib.window_specs(
        unspaced.max_length, unspaced.W, ccs_width, ccs_bq, ccs_idx,
        windows_lib.fixed_window_widths(ccs_width, unspaced.max_length),
        counter,
    )
    return _plane_zmw_windows(
        zmw, unspaced, specs, ccs_ids, modes.passthrough_mode == "device",
        zmw, ccs, options, counter, expand_counter,
    )


def _skip_window(overflow, ccs_bq, options: InferenceOptions) -> bool:
    """Skip triage: overflow windows and windows whose average CCS
    quality exceeds --skip_windows_above take the CCS passthrough."""
    skip = bool(overflow)
    if not skip and options.skip_windows_above:
        skip = phred.avg_phred(ccs_bq) > options.skip_windows_above
    return skip


def process_skipped_window(
    feature_dict: Dict[str, Any], options: InferenceOptions
) -> stitch_utils.DCModelOutput:
    """CCS passthrough for skipped windows (quick_inference.py:567-594)."""
    rows = feature_dict["subreads"]
    (_, _, _, _, ccs_index, _, _) = cfg.get_indices(
        options.max_passes, options.use_ccs_bq
    )
    return _passthrough_output(
        rows[ccs_index[0], :, 0],
        feature_dict["ccs_base_quality_scores"],
        feature_dict["window_pos"],
        feature_dict["name"],
        feature_dict["ec"], feature_dict["np_num_passes"],
        feature_dict["rq"], feature_dict["rg"],
        options,
    )


def passthrough_qualities(ccs_bq, options: InferenceOptions) -> np.ndarray:
    """Output QVs (int32) of a passthrough window from its CCS qualities:
    calibration when enabled, then the clamp to 0..max_base_quality.
    Elementwise, so it is also what passthrough_quality_lut tabulates."""
    ccs_quality_scores = np.asarray(ccs_bq, dtype=np.float64)
    if options.ccs_calibration_values.enabled:
        ccs_quality_scores = calibration_lib.calibrate_quality_scores(
            ccs_quality_scores, options.ccs_calibration_values
        )
    ccs_quality_scores = np.minimum(
        ccs_quality_scores, options.max_base_quality
    )
    ccs_quality_scores = np.maximum(ccs_quality_scores, 0)
    return ccs_quality_scores.astype(np.int32)


def passthrough_quality_lut(options: InferenceOptions) -> np.ndarray:
    """uint8 [256]: ZmwPlanes.ccs_q code (q + 1) -> output QV, by
    passthrough_qualities itself over q = -1..254. The device passthrough
    looks QVs up here, so no quality arithmetic runs on the GPU."""
    stitch_device.check_max_base_quality(options.max_base_quality)
    return passthrough_qualities(np.arange(-1, 255), options).astype(
        np.uint8
    )


def _runner_quality_lut(runner, options: InferenceOptions, native: bool):
    """passthrough_quality_lut, built (and on a native runner uploaded)
    once per runner and set of quality options instead of per ZMW batch."""
    c = options.ccs_calibration_values
    key = (options.max_base_quality, c.enabled, c.threshold, c.w, c.b)
    cache = getattr(runner, "_passthrough_luts", None)
    if cache is None:
        cache = {}
        try:
            runner._passthrough_luts = cache
        except AttributeError:  # a runner that takes no attributes
            pass
    lut = cache.get(key)
    if lut is None:
        lut = passthrough_quality_lut(options)
        if native:
            lut = torch.from_numpy(lut).to(runner.device)
        cache[key] = lut
    return lut


def _passthrough_output(
    ccs_ids: np.ndarray, ccs_bq, window_pos, name, ec, np_num_passes, rq,
    rg, options: InferenceOptions,
) -> stitch_utils.DCModelOutput:
    """The passthrough DCModelOutput from the window's padded CCS base
    ids and padded CCS qualities alone."""
    ccs_seq = phred.encoded_sequence_to_string(ccs_ids)
    ccs_quality_scores = passthrough_qualities(ccs_bq, options)
    return stitch_utils.DCModelOutput(
        window_pos=window_pos,
        molecule_name=name,
        sequence=ccs_seq,
        quality_string=phred.quality_scores_to_string(ccs_quality_scores),
        ec=ec,
        np_num_passes=np_num_passes,
        rq=rq,
        rg=rg,
    )


def _gap_tripwire(runner, rows_t, bases_np, gap_frac, n_chunk):
    """Audits a majority-gap chunk against the fp32 torch path.

    ``bases_np`` is the chunk's host base ids, or a callable returning
    them: a caller that keeps the chunk on the device then copies it back
    for suspect chunks only.
    """
    # Corruption tripwire: a healthy model rarely predicts majority
    # gap. A batch-size-dependent native-path regression produced
    # silent all-gap output (profiles/r01_perf_journal.md "GAP
    # REGRESSION") — surface it instead of writing garbage FASTQ.
    if gap_frac > 0.6 and n_chunk > 1 and getattr(
        runner, "native", False
    ):
        if callable(bases_np):
            bases_np = bases_np()
        # Corruption tripwire turned hard gate: audit a
        # sample of the suspect batch against the fp32 torch path
        # and refuse to write FASTQ from a disagreeing native pass.
        sample = min(32, n_chunk)
        with torch.no_grad():
            probs = runner.model(
                rows_t[:sample].to(runner.device).float(),
                training=False,
            )
        torch_bases = probs.argmax(-1).cpu().numpy()
        agree = float((bases_np[:sample] == torch_bases).mean())
        if agree < 0.99:
            raise RuntimeError(
                f"native inference path disagrees with the torch "
                f"reference on {100 * (1 - agree):.1f}% of base "
                f"calls in a {100 * gap_frac:.0f}%-gap batch of "
                f"{n_chunk} windows — refusing to write "
                f"corrupted FASTQ. This indicates a native-kernel "
                f"regression; re-run with DC_FUSED_FFN=0/"
                f"smaller --batch_size and file a bug."
            )
        log.info(
            "high gap fraction %.0f%% over %d windows, but the "
            "native path agrees with the torch reference "
            "(%.4f) — input is legitimately gappy",
            100.0 * gap_frac, n_chunk, agree,
        )


_SEQ_LUT = np.frombuffer(constants.SEQ_VOCAB.encode("ascii"), np.uint8)


# The model input of a ZMW batch and its chunk loop live in model_chunks.py.
_ModelChunks = model_chunks_lib.model_chunks


def run_model_on_zmws(
    zmws: List[ZmwWindows],
    runner: InferenceRunner,
    options: InferenceOptions,
) -> List[stitch_utils.DCModelOutput]:
    """Batched model execution emitting per-window DCModelOutput.

    Model-bound windows arrive pre-stacked per ZMW; this concatenates
    them across the ZMW batch, runs the device model in batch_size
    chunks, and converts bases/QVs to strings with batch-level numpy
    (one LUT pass + one +33 pass per chunk).
    """
    predictions: List[stitch_utils.DCModelOutput] = []
    for z in zmws:
        if featurize_device.n_table_passthrough(z):
            raise ValueError(
                "passthrough table entries need the device stitcher "
                "(run_model_and_stitch_on_zmws)"
            )
        predictions.extend(z.skipped)
    chunks = _ModelChunks(zmws, runner, options)
    if not chunks.n_model:
        return predictions
    # Per-window owner metadata, in concatenation order.
    owners: List[ZmwWindows] = []
    for z in chunks.model_zmws:
        owners.extend([z] * featurize_device.n_model_windows(z))
    all_pos = chunks.all_pos
    for i, rows_t, bases_t, quals_t, n_valid in chunks.forward():
        bases_np = bases_t.cpu().numpy()
        _gap_tripwire(
            runner, rows_t, bases_np, float((bases_np == 0).mean()),
            n_valid,
        )
        seq_mat = _SEQ_LUT[bases_np.astype(np.int64)]
        qual_mat = (quals_t.cpu().numpy() + 33).astype(np.uint8)
        for j in range(n_valid):
            z = owners[i + j]
            predictions.append(
                stitch_utils.DCModelOutput(
                    window_pos=int(all_pos[i + j]),
                    molecule_name=z.name,
                    sequence=seq_mat[j].tobytes().decode("ascii"),
                    quality_string=qual_mat[j].tobytes().decode("ascii"),
                    ec=z.ec,
                    np_num_passes=z.np_num_passes,
                    rq=z.rq,
                    rg=z.rg,
                )
            )
    return predictions


@dataclasses.dataclass
class StitchedBatch:
    """Output of run_model_and_stitch_on_zmws: the stitch plan plus the
    gap-free bytes of every read of the ZMW batch, on the host."""

    plan: stitch_device.StitchPlan
    seq_out: np.ndarray  # uint8 ASCII bases, reads back to back
    qual_out: np.ndarray  # uint8 Phred+33
    out_off: np.ndarray  # [S + 1] int32 segment offsets into the above
    n_model: int
    n_skipped: int

    def __len__(self) -> int:
        return self.n_model + self.n_skipped


def run_model_and_stitch_on_zmws(
    zmws: List[ZmwWindows],
    runner: InferenceRunner,
    options: InferenceOptions,
) -> StitchedBatch:
    """Batched model execution with the stitch done on the device.

    Same model loop as run_model_on_zmws, but each chunk's base ids and
    QVs are copied device-to-device into one flat accumulation buffer per
    ZMW batch; after the last chunk the stitch_compact kernel drops the
    gap positions and one D2H copy returns the finished read bytes. No
    per-window objects are built and gap bytes never leave the device.
    On a non-native runner the same plan runs on host buffers with the
    kernel's numpy twin.
    """
    stitch_device.check_max_base_quality(options.max_base_quality)
    n_skipped = sum(
        len(z.skipped) + featurize_device.n_table_passthrough(z)
        for z in zmws
    )
    chunks = _ModelChunks(zmws, runner, options)
    all_pos = chunks.all_pos
    row_length = chunks.row_length
    n_model = chunks.n_model
    plan = stitch_device.build_plan(
        zmws, all_pos, options.max_length, row_length=row_length
    )
    n_model_bytes = n_model * row_length
    n_table_bytes = plan.n_table_bytes
    n_total = plan.n_source_bytes
    if n_table_bytes != chunks.n_pt_bytes:
        raise ValueError(
            "stitch plan and packed passthrough table disagree on the "
            "size of the passthrough region"
        )
    # Object passthrough windows sit behind the table ones.
    extra_lo = n_model_bytes + n_table_bytes

    native = bool(getattr(runner, "native", False))
    # One [2, n_total] buffer: row 0 base ids, row 1 QVs; model windows
    # first, passthrough windows behind them (StitchPlan has the order).
    if native:
        acc = torch.empty((2, n_total), dtype=torch.uint8,
                          device=runner.device)
    else:
        acc_np = np.empty((2, n_total), np.uint8)
    # The per-chunk gap count below synchronises, so the staging buffer is
    # free again before the next chunk overwrites it.
    for i, rows_t, bases_t, quals_t, n_valid in chunks.forward():
        lo, hi = i * row_length, (i + n_valid) * row_length
        if native:
            # The graph's output buffer is rewritten by the next replay:
            # these copies are queued on the same stream ahead of it.
            acc[0, lo:hi].view(n_valid, row_length).copy_(bases_t)
            acc[1, lo:hi].view(n_valid, row_length).copy_(quals_t)
            n_gap = int((bases_t == 0).sum().item())
            bases_host = lambda b=bases_t: b.cpu().numpy()  # noqa: E731
        else:
            bases_host = bases_t.cpu().numpy()
            acc_np[0, lo:hi] = bases_host.reshape(-1)
            acc_np[1, lo:hi] = quals_t.cpu().numpy().reshape(-1)
            n_gap = int((bases_host == 0).sum())
        # Exact count / size: the same float64 as the host-side mean.
        _gap_tripwire(
            runner, rows_t, bases_host, n_gap / (n_valid * row_length),
            n_valid,
        )

    n_seg = len(plan.seg_off)
    if n_seg == 0:
        seq_out = qual_out = np.empty(0, np.uint8)
        out_off = np.zeros(1, np.int32)
    elif native:
        if n_table_bytes:
            chunks.fill_passthrough(
                _runner_quality_lut(runner, options, True),
                acc[0, n_model_bytes:extra_lo],
                acc[1, n_model_bytes:extra_lo],
            )
        if n_total > extra_lo:
            extra = torch.from_numpy(
                np.stack([plan.extra_bases, plan.extra_quals])
            )
            acc[:, extra_lo:].copy_(extra)
        segs = torch.from_numpy(
            np.stack([plan.seg_off, plan.seg_len])
        ).to(runner.device)
        seq_t, qual_t, _, off_t = runner.ext.stitch_compact(
            acc[0], acc[1], segs[0], segs[1]
        )
        # One D2H copy: [out_off bytes | seq_out | qual_out].
        packed = torch.cat(
            [off_t.view(torch.uint8), seq_t, qual_t]
        ).cpu().numpy()
        n_off = 4 * (n_seg + 1)
        out_off = packed[:n_off].view(np.int32)
        n_kept = int(out_off[-1])
        seq_out = packed[n_off : n_off + n_kept]
        qual_out = packed[n_off + n_kept :]
    else:
        if n_table_bytes:
            chunks.fill_passthrough(
                _runner_quality_lut(runner, options, False),
                acc_np[0, n_model_bytes:extra_lo],
                acc_np[1, n_model_bytes:extra_lo],
            )
        acc_np[0, extra_lo:] = plan.extra_bases
        acc_np[1, extra_lo:] = plan.extra_quals
        seq_out, qual_out, _, out_off = (
            stitch_device.compact_segments_numpy(
                acc_np[0], acc_np[1], plan.seg_off, plan.seg_len
            )
        )
    return StitchedBatch(
        plan=plan, seq_out=seq_out, qual_out=qual_out, out_off=out_off,
        n_model=n_model, n_skipped=n_skipped,
    )


class Timelog:
    """Stage wall-clock CSV (quick_inference.py:278-299,777-783)."""

    def __init__(self):
        self.rows: List[Dict[str, Any]] = []

    def add(self, stage, item, before, num_examples=None, num_subreads=None,
            num_zmws=None):
        self.rows.append(
            dict(
                item=item, stage=stage, runtime=time.time() - before,
                num_zmws=num_zmws, num_examples=num_examples,
                num_subreads=num_subreads,
            )
        )

    def save(self, output_prefix: str):
        cols = ["item", "stage", "runtime", "num_zmws", "num_examples",
                "num_subreads"]
        with open(f"{output_prefix}.csv", "w") as f:
            f.write(",".join(cols) + "\n")
            for r in self.rows:
                f.write(",".join(str(r[c]) for c in cols) + "\n")


def _stitch_batch_to_text(args):
    """Process-pool stitcher: sorts + stitches a batch of predictions
    into FASTQ text, returning (text, outcome_counts). Runs in the
    worker pool so the GIL-heavy stitching never blocks the serial
    model loop or the prefetch threads."""
    predictions, max_length, min_quality, min_length = args
    counter = stitch_utils.OutcomeCounter()
    parts = []
    predictions = sorted(
        predictions, key=lambda dc: (dc.molecule_name, dc.window_pos)
    )
    for zmw, preds in itertools.groupby(
        predictions, lambda p: p.molecule_name
    ):
        fastq_string = stitch_utils.stitch_to_fastq(
            molecule_name=zmw,
            predictions=list(preds),
            max_length=max_length,
            min_quality=min_quality,
            min_length=min_length,
            outcome_counter=counter,
        )
        if fastq_string:
            parts.append(fastq_string)
    return "".join(parts), dataclasses.asdict(counter)


def _write_outputs(
    predictions: List[stitch_utils.DCModelOutput],
    output_writer,
    bam_out,
    options: InferenceOptions,
    outcome_counter: stitch_utils.OutcomeCounter,
):
    """Sorts, stitches and writes per-ZMW outputs
    (quick_inference.py:718-760)."""
    from deepconsensus_amd.dcio import bam as bam_lib

    predictions = sorted(
        predictions, key=lambda dc: (dc.molecule_name, dc.window_pos)
    )
    for zmw, preds in itertools.groupby(
        predictions, lambda p: p.molecule_name
    ):
        preds = list(preds)
        fastq_string = stitch_utils.stitch_to_fastq(
            molecule_name=zmw,
            predictions=preds,
            max_length=options.max_length,
            min_quality=options.min_quality,
            min_length=options.min_length,
            outcome_counter=outcome_counter,
        )
        if not fastq_string:
            continue
        if bam_out is None:
            output_writer.write(fastq_string)
        else:
            name, seq, _, qual = fastq_string.splitlines()
            name = name[1:]
            record = bam_lib.BamRead(
                qname=name,
                flag=4,
                ref_id=-1,
                pos=-1,
                mapq=255,
                seq=seq,
                query_qualities=phred.quality_string_to_array(qual),
                tags={
                    "ec": preds[0].ec if preds[0].ec is not None else -1.0,
                    "np": preds[0].np_num_passes or 0,
                    "rq": preds[0].rq if preds[0].rq is not None else -1.0,
                    "RG": preds[0].rg or "",
                    "zm": int(name.split("/")[1]),
                },
            )
            bam_out.write(record)


def _write_stitched(
    stitched: StitchedBatch,
    output_writer,
    bam_out,
    options: InferenceOptions,
    outcome_counter: stitch_utils.OutcomeCounter,
):
    """_write_outputs for a device-stitched batch: filters and writes the
    already gap-free reads (same FASTQ text, same BAM tags)."""
    from deepconsensus_amd.dcio import bam as bam_lib

    for name, seq, qual, (ec, np_num_passes, rq, rg) in (
        stitch_device.finish_reads(
            stitched.plan, stitched.seq_out, stitched.qual_out,
            stitched.out_off, options, outcome_counter,
        )
    ):
        seq = seq.decode("ascii")
        if bam_out is None:
            output_writer.write(
                stitch_utils.format_as_fastq(name, seq, qual.decode("ascii"))
            )
        else:
            record = bam_lib.BamRead(
                qname=name,
                flag=4,
                ref_id=-1,
                pos=-1,
                mapq=255,
                seq=seq,
                query_qualities=(
                    np.frombuffer(qual, np.uint8).astype(np.int64) - 33
                ).tolist(),
                tags={
                    "ec": ec if ec is not None else -1.0,
                    "np": np_num_passes or 0,
                    "rq": rq if rq is not None else -1.0,
                    "RG": rg or "",
                    "zm": int(name.split("/")[1]),
                },
            )
            bam_out.write(record)


def run(
    subreads_to_ccs: str,
    ccs_bam: str,
    checkpoint: str,
    output: str,
    options: Optional[InferenceOptions] = None,
    limit: int = 0,
    dc_calibration: Optional[str] = None,
    ccs_calibration: Optional[str] = None,
    device: Optional[str] = None,
) -> stitch_utils.OutcomeCounter:
    """Performs an inference run (quick_inference.py:794-963)."""
    t_start = time.time()
    options = options or InferenceOptions()
    # A bad value or mode combination fails here, not in a worker.
    stitch_mode = resolve_modes(options).stitch_mode
    if stitch_mode == "device":
        stitch_device.check_max_base_quality(options.max_base_quality)

    # Load params + model. checkpoint == 'random' builds a random-init model
    # (testing only); otherwise a directory with params.json + weights.
    if checkpoint == "random":
        params = cfg.get_config("transformer_learn_values+custom")
        params.max_passes = options.max_passes
        cfg.modify_params(
            params, max_length=options.max_length, is_training=False
        )
        model = get_model(params)
    else:
        params = ckpt_lib.load_params(checkpoint)
        cfg.modify_params(
            params, max_length=options.max_length, is_training=False
        )
        model = get_model(params)
        ckpt_lib.load_checkpoint(checkpoint, model)
        options.max_passes = params.max_passes
        options.use_ccs_bq = bool(params.get("use_ccs_bq", False))
    options.example_height = cfg.get_total_rows(
        options.max_passes, options.use_ccs_bq
    )

    # Calibration: explicit flag > params.json dc_calibration > skip.
    if dc_calibration is None:
        dc_calibration = params.get("dc_calibration", "skip")
    options.dc_calibration_values = calibration_lib.parse_calibration_string(
        dc_calibration
    )
    if ccs_calibration is not None:
        options.ccs_calibration_values = (
            calibration_lib.parse_calibration_string(ccs_calibration)
        )

    calib_str = dc_calibration if dc_calibration else "skip"

    # Output writer.
    bam_out = None
    if output.endswith(".bam"):
        from deepconsensus_amd.dcio import bam as bam_lib

        header = bam_lib.BamHeader(
            text="@HD\tVN:1.6\tSO:unknown", references=[]
        )
        bam_out = bam_lib.BamWriter(output, header)
        output_writer = None
    else:
        output_writer = open(output, "w")

    outcome_counter = stitch_utils.OutcomeCounter()
    stats_counter = collections.Counter()
    timelog = Timelog()
    output_prefix = os.path.splitext(output)[0]

    dc_config = DcConfig(
        options.max_passes, options.max_length, options.use_ccs_bq
    )
    proc_feeder, main_counter = pre_feeder.create_proc_feeder(
        subreads_to_ccs=subreads_to_ccs,
        ccs_bam=ccs_bam,
        dc_config=dc_config,
        ins_trim=options.ins_trim,
        use_ccs_smart_windows=options.use_ccs_smart_windows,
        limit=limit,
        defer_expansion=True,
        shard_index=options.shard_index,
        shard_count=options.shard_count,
    )

    pool = None
    stitch_pool = None
    if options.cpus > 0:
        pool = concurrent.futures.ProcessPoolExecutor(options.cpus)
        # Dedicated small stitch pool: submitting stitch work to the
        # preprocess pool queued it AHEAD of later preprocess batches
        # (FIFO) and starved the prefetch pipeline (measured 209 -> 130
        # ZMW/s at 1000 ZMWs).
        stitch_pool = concurrent.futures.ProcessPoolExecutor(
            max(2, options.cpus // 4)
        )

    def zmw_batches():
        # ZMW sharding happens inside the feeder (byte-range seek when a
        # `deepconsensus index` sidecar exists, modulo streaming else).
        batch = []
        for input_data in proc_feeder():
            subreads, zmw, dcc, split, window_widths = input_data
            batch.append((zmw, subreads, dcc, window_widths, options))
            if len(batch) >= options.batch_zmws:
                yield batch
                batch = []
        if batch:
            yield batch

    def preprocess_batch(inputs):
        if pool is not None:
            return list(pool.map(preprocess_one_zmw, inputs))
        return [preprocess_one_zmw(z) for z in inputs]

    def infer_batch(inputs, outputs, batch_name):
        before = time.time()
        for z in outputs:
            stats_counter.update(z.counter)
        n_examples = sum(z.n_examples for z in outputs)
        n_subreads = sum(len(z[1]) for z in inputs)
        timelog.add("preprocess", batch_name, before, n_examples,
                    n_subreads, len(inputs))
        if options.end_after_stage in (DebugStage.DC_INPUT,
                                       DebugStage.TF_EXAMPLES):
            return

        before = time.time()
        n_model = sum(z.n_model for z in outputs)
        n_skipped = sum(z.n_skipped for z in outputs)
        if stitch_mode == "device":
            preds = run_model_and_stitch_on_zmws(outputs, runner, options)
        else:
            preds = run_model_on_zmws(outputs, runner, options)
        # Per-batch model/skip split (quick_inference.py:688-705).
        total = max(len(preds), 1)
        log.info(
            "Example summary: ran model=%d (%.2f%%) skip=%d (%.2f%%) "
            "total=%d.",
            n_model, 100.0 * n_model / total,
            n_skipped, 100.0 * n_skipped / total, len(preds),
        )
        timelog.add("run_model", batch_name, before, n_examples,
                    n_subreads, len(inputs))
        if options.end_after_stage == DebugStage.RUN_MODEL:
            return

        before = time.time()
        # Within-lease A/B at 800 ZMWs: serial 173 ZMW/s vs pool 162
        # (plus ~2 s stitch-pool spin-up on the first batch) — the
        # overlap does not pay at this scale; serial is the default
        # and DC_STITCH_MODE=pool keeps the experiment reachable.
        if stitch_mode == "device":
            _write_stitched(preds, output_writer, bam_out, options,
                            outcome_counter)
            timelog.add("stitch_and_write_fastq", batch_name, before,
                        n_examples, n_subreads, len(inputs))
        elif (stitch_mode == "pool" and stitch_pool is not None
                and bam_out is None):
            # Stitch in the PROCESS pool (no GIL contention with the
            # prefetch threads), write the returned text on the ordered
            # writer thread. BAM output keeps the in-process path (the
            # writer needs record objects).
            fut = stitch_pool.submit(
                _stitch_batch_to_text,
                (preds, options.max_length, options.min_quality,
                 options.min_length),
            )

            def write_task(fut=fut, batch_name=batch_name,
                           n_examples=n_examples,
                           n_subreads=n_subreads, n_inputs=len(inputs),
                           before=before):
                text, counts = fut.result()
                for k, v in counts.items():
                    setattr(outcome_counter, k,
                            getattr(outcome_counter, k) + v)
                if text:
                    output_writer.write(text)
                timelog.add("stitch_and_write_fastq", batch_name,
                            before, n_examples, n_subreads, n_inputs)

            writer_futs.append(writer_pool.submit(write_task))
        else:
            _write_outputs(preds, output_writer, bam_out, options,
                           outcome_counter)
            timelog.add("stitch_and_write_fastq", batch_name, before,
                        n_examples, n_subreads, len(inputs))

    # Pipelined loop: up to `prefetch_batches` ZMW batches preprocess in
    # the worker pool while the current batch runs the model.
    batch_iter = zmw_batches()
    lookahead = max(1, options.prefetch_batches)
    pending: "collections.deque" = collections.deque()
    n_fed = 0
    n_batches = 0
    writer_pool = concurrent.futures.ThreadPoolExecutor(1)
    writer_futs: List[concurrent.futures.Future] = []
    with concurrent.futures.ThreadPoolExecutor(lookahead) as prefetcher:

        def feed_one() -> bool:
            # Serial ZMW streaming is a real pipeline stage: account it
            # (the reference folded it into its preprocess rows).
            nonlocal n_fed
            before = time.time()
            inputs = next(batch_iter, None)
            timelog.add("feeder", f"batch {n_fed}", before,
                        num_zmws=len(inputs) if inputs else 0)
            if inputs is None:
                return False
            pending.append(
                (inputs, prefetcher.submit(preprocess_batch, inputs))
            )
            n_fed += 1
            return True

        # Prime the pipeline BEFORE device/model setup: the worker pool
        # preprocesses the first batches while InferenceRunner brings up
        # the device, loads the HIP extension and moves weights — on a
        # cold box that startup is ~20 s and fully overlapped.
        while len(pending) < lookahead and feed_one():
            pass
        before = time.time()
        runner = InferenceRunner(
            params, model, device=device, calibration=calib_str,
            max_qual=options.max_base_quality,
        )
        timelog.add("startup_runner", "startup", before)
        log.info("model on %s (native kernels: %s)", runner.device,
                 runner.native)

        while pending:
            prev_inputs, prev_fut = pending.popleft()
            name = f"batch {n_batches}"
            # Time blocked on the overlapped preprocessing (not a
            # reference stage; extends the CSV so wall is accounted).
            before = time.time()
            outputs = prev_fut.result()
            timelog.add("wait_preprocess", name, before, None, None,
                        len(prev_inputs))
            infer_batch(prev_inputs, outputs, name)
            n_batches += 1
            while len(pending) < lookahead and feed_one():
                pass

    writer_pool.shutdown(wait=True)
    for f in writer_futs:
        f.result()  # surface stitch/write errors instead of truncating
    if stitch_pool is not None:
        stitch_pool.shutdown()
    if pool is not None:
        pool.shutdown()
    if bam_out is not None:
        bam_out.close()
    if output_writer is not None:
        output_writer.close()

    stats_counter.update(main_counter)
    timelog.save(f"{output_prefix}.runtime")
    with open(f"{output_prefix}.inference.json", "w") as f:
        json.dump(dict(stats_counter), f, indent=True)

    log.info(
        "Processed %d ZMWs in %.3f seconds",
        main_counter["n_zmw_processed"], time.time() - t_start,
    )
    log.info("Outcome counts: %s", outcome_counter)
    return outcome_counter
