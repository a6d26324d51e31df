"""Device-side window stitching: plan on the host, compact on the device.

The serial stitcher (postprocess/stitch.py) builds one DCModelOutput per
window, sorts and joins them, and removes gaps in a per-character Python
loop. This module splits the same computation into three parts so that the
per-base work is a single stream compaction over ``uint8`` buffers:

* ``build_plan``   — host, per-window metadata only: reproduces the
  ``_write_outputs`` + ``get_full_sequence`` ordering (reads by name,
  windows by position, missing-window discard) and emits a *segment table*
  (source offset + length per window, in output order).
* compaction       — ``ops/hip/stitch_compact.hip`` on the device, or its
  numpy twin ``compact_segments_numpy`` (CPU backend and test oracle):
  drops gap positions, translates ids to ASCII and QVs to Phred+33.
* ``finish_reads`` — host, per read: the remaining ``stitch_to_fastq``
  taxonomy (only_gaps, quality filter, length filter, success).

``stitch.py`` stays the oracle; N-fill (``fill_n=True``) is not offered.
"""
from __future__ import annotations

import dataclasses
from typing import Any, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from deepconsensus_amd.postprocess import stitch as stitch_utils
from deepconsensus_amd.preprocess.featurize_device import (
    n_model_windows,
    n_table_passthrough,
)
from deepconsensus_amd.utils import constants, phred

# Largest QV whose +33 byte is still printable ASCII ('~').
MAX_DEVICE_QUAL = 93

# id -> ASCII. Ids outside the vocabulary surface as 'N', as in the kernel.
_ID_TO_ASCII = np.full(256, ord("N"), np.uint8)
_ID_TO_ASCII[: len(constants.SEQ_VOCAB)] = np.frombuffer(
    constants.SEQ_VOCAB.encode("ascii"), np.uint8
)
# ASCII -> id; 255 marks a character outside SEQ_VOCAB.
_ASCII_TO_ID = np.full(256, 255, np.uint8)
for _i, _c in enumerate(constants.SEQ_VOCAB):
    _ASCII_TO_ID[ord(_c)] = _i

# (ec, np_num_passes, rq, rg) of a read's first window.
ReadMetadata = Tuple[
    Optional[float], Optional[int], Optional[float], Optional[str]
]


def check_max_base_quality(max_base_quality: int) -> None:
    """Device mode keeps QVs as uint8 and emits QV+33 as one ASCII byte."""
    if max_base_quality > MAX_DEVICE_QUAL:
        raise ValueError(
            f"max_base_quality={max_base_quality} is not supported by the "
            f"device stitcher: QV+33 must stay printable ASCII "
            f"(max {MAX_DEVICE_QUAL})"
        )


def compact_segments_numpy(
    bases: np.ndarray,
    quals: np.ndarray,
    seg_off: np.ndarray,
    seg_len: np.ndarray,
) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Numpy twin of the ``stitch_compact`` kernel.

    Returns (seq_out u8, qual_out u8, seg_kept i32 [S], out_off i32 [S+1]).
    """
    bases = np.asarray(bases)
    quals = np.asarray(quals)
    if bases.dtype != np.uint8 or quals.dtype != np.uint8:
        raise ValueError("bases and quals must be uint8")
    if bases.ndim != 1 or bases.shape != quals.shape:
        raise ValueError("bases and quals must be flat and of equal length")
    seg_off = np.asarray(seg_off).astype(np.int64).ravel()
    seg_len = np.asarray(seg_len).astype(np.int64).ravel()
    if seg_off.shape != seg_len.shape:
        raise ValueError("seg_off and seg_len must have equal length")
    n_seg = len(seg_off)
    if n_seg and (
        (seg_len < 0).any()
        or (seg_off < 0).any()
        or (seg_off + seg_len > len(bases)).any()
    ):
        raise ValueError("segment outside the source buffer")
    # Gather index of every source byte, in output (segment) order.
    src_start = np.cumsum(seg_len) - seg_len
    n_src = int(seg_len.sum())
    idx = np.repeat(seg_off - src_start, seg_len) + np.arange(n_src)
    seg_id = np.repeat(np.arange(n_seg), seg_len)
    ids = bases[idx]
    keep = ids != 0
    seg_kept = np.bincount(seg_id[keep], minlength=n_seg).astype(np.int32)
    out_off = np.zeros(n_seg + 1, np.int32)
    np.cumsum(seg_kept, out=out_off[1:])
    seq_out = _ID_TO_ASCII[ids[keep]]
    qual_out = (quals[idx][keep] + np.uint8(33)).astype(np.uint8)
    return seq_out, qual_out, seg_kept, out_off


@dataclasses.dataclass
class StitchPlan:
    """Everything about one ZMW batch's stitching except the bytes.

    The flat source buffers are laid out as ``n_model * row_length`` model
    bytes (window i at ``[i * row_length, (i + 1) * row_length)``) followed
    by the passthrough windows: first the ``n_table_bytes`` of the windows
    that arrive as passthrough table entries of their ZMW's planes (ZMW
    order, then window order; filled from the CCS planes by
    ``passthrough_fill``), then ``extra_bases`` / ``extra_quals``, the
    windows that arrive as ``DCModelOutput`` objects.
    Read r owns segments ``read_seg_start[r] : read_seg_start[r + 1]``.
    """

    read_names: List[str]
    read_empty: np.ndarray  # [R] bool: empty_sequence reads (no segments)
    read_seg_start: np.ndarray  # [R + 1] int64
    read_metadata: List[ReadMetadata]
    seg_off: np.ndarray  # [S] int32
    seg_len: np.ndarray  # [S] int32
    extra_bases: np.ndarray  # uint8 ids of the object passthrough windows
    extra_quals: np.ndarray  # uint8 QVs of the object passthrough windows
    n_model: int
    row_length: int
    n_table_bytes: int = 0  # region of the table passthrough windows

    @property
    def n_source_bytes(self) -> int:
        return (self.n_model * self.row_length + self.n_table_bytes
                + len(self.extra_bases))


def _decode_passthrough(
    skipped: Sequence[stitch_utils.DCModelOutput],
) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Joined passthrough strings -> (ids u8, QVs u8, per-window length)."""
    seqs = [sk.sequence for sk in skipped]
    qual_strs = [sk.quality_string for sk in skipped]
    lengths = np.fromiter((len(s) for s in seqs), np.int64, len(seqs))
    qual_lengths = np.fromiter(
        (len(q) for q in qual_strs), np.int64, len(qual_strs)
    )
    if (lengths != qual_lengths).any():
        raise ValueError(
            "passthrough window with sequence and quality_string of "
            "different lengths"
        )
    seq_bytes = np.frombuffer("".join(seqs).encode("ascii"), np.uint8)
    qual_bytes = np.frombuffer("".join(qual_strs).encode("ascii"), np.uint8)
    ids = _ASCII_TO_ID[seq_bytes]
    if (ids == 255).any():
        raise ValueError(
            f"passthrough sequence has characters outside "
            f"{constants.SEQ_VOCAB!r}"
        )
    if (qual_bytes < 33).any():
        raise ValueError("passthrough quality_string below Phred+33 '!'")
    return ids, qual_bytes - np.uint8(33), lengths


def build_plan(
    zmws: Sequence[Any],
    all_pos: Optional[np.ndarray],
    max_length: int,
    row_length: Optional[int] = None,
) -> StitchPlan:
    """Builds the segment table for one ZMW batch.

    ``zmws`` are ZmwWindows-like objects (``name``, ``window_pos``,
    ``rows`` or ``planes``, ``skipped``, ``ec``, ``np_num_passes``, ``rq``,
    ``rg``).
    Model windows are numbered in concatenation order (ZMW by ZMW, the
    order ``run_model_on_zmws`` stacks them); ``all_pos`` is their
    concatenated ``window_pos`` (derived from ``zmws`` when None).

    Ordering parity with ``_write_outputs``: its prediction list holds
    every skipped window first, then every model window; it is sorted
    (stably) by (molecule_name, window_pos) and grouped by name. A read
    whose k-th window sits at ``window_pos > k * max_length`` — or whose
    windows are all empty — is ``empty_sequence`` and contributes no
    segments. A ZMW without any window never reaches the stitcher there
    and is not a read here either.

    A skipped window is either a ``DCModelOutput`` in ``z.skipped`` or an
    entry of the passthrough table of ``z.planes`` (``pt_pos``,
    ``pt_width``); both take the same place in the prediction list, and a
    table entry carries its ZMW's name and tags.
    """
    row_length = max_length if row_length is None else row_length
    names: List[str] = []
    name_id: dict = {}

    def intern(name: str) -> int:
        i = name_id.get(name)
        if i is None:
            i = name_id[name] = len(names)
            names.append(name)
        return i

    skipped = [sk for z in zmws for sk in z.skipped]
    model_zmws = [z for z in zmws if n_model_windows(z)]
    model_counts = np.fromiter(
        (n_model_windows(z) for z in model_zmws), np.int64, len(model_zmws)
    )
    n_model = int(model_counts.sum())
    if all_pos is None:
        all_pos = (
            np.concatenate([z.window_pos for z in model_zmws])
            if model_zmws else np.empty(0, np.int64)
        )
    all_pos = np.asarray(all_pos, np.int64)
    if len(all_pos) != n_model:
        raise ValueError("all_pos does not match the model window count")

    extra_bases, extra_quals, sk_len = _decode_passthrough(skipped)

    # Skipped windows in prediction-list order: ZMW by ZMW, a ZMW's either
    # as objects or as passthrough table entries of its planes. Objects
    # are walked one by one; table entries are whole arrays per ZMW.
    # s_owner indexes ``skipped`` for an object, ``zmws`` for an entry.
    s_name: List[np.ndarray] = []
    s_pos: List[np.ndarray] = []
    s_tab: List[np.ndarray] = []
    s_owner: List[np.ndarray] = []
    tab_len: List[np.ndarray] = []
    n_objects = 0
    for zi, z in enumerate(zmws):
        n_obj, n_tab = len(z.skipped), n_table_passthrough(z)
        if n_obj:
            s_name.append(np.fromiter(
                (intern(sk.molecule_name) for sk in z.skipped), np.int64,
                n_obj,
            ))
            s_pos.append(np.fromiter(
                (int(sk.window_pos) for sk in z.skipped), np.int64, n_obj
            ))
            s_tab.append(np.zeros(n_obj, bool))
            s_owner.append(np.arange(n_objects, n_objects + n_obj))
            n_objects += n_obj
        if n_tab:
            p = z.planes
            pos = np.asarray(p.pt_pos, np.int64)
            width = np.asarray(p.pt_width, np.int64)
            if pos.shape != (n_tab,) or width.shape != (n_tab,):
                raise ValueError(
                    "passthrough table columns of different lengths"
                )
            if (width < 0).any():
                raise ValueError("passthrough window of negative width")
            s_name.append(np.full(n_tab, intern(z.name), np.int64))
            s_pos.append(pos)
            s_tab.append(np.ones(n_tab, bool))
            s_owner.append(np.full(n_tab, zi, np.int64))
            tab_len.append(width)

    def cat(parts: List[np.ndarray], dtype) -> np.ndarray:
        return np.concatenate(parts) if parts else np.empty(0, dtype)

    is_tab = cat(s_tab, bool)
    skip_owner = cat(s_owner, np.int64)
    tab_len_all = cat(tab_len, np.int64)
    n_skipped = len(is_tab)
    n_table_bytes = int(tab_len_all.sum())
    table_lo = n_model * row_length
    if table_lo + n_table_bytes + len(extra_bases) >= 2**31:
        raise ValueError("ZMW batch too large for int32 segment offsets")
    s_len = np.empty(n_skipped, np.int64)
    s_len[is_tab] = tab_len_all
    s_len[~is_tab] = sk_len
    s_off = np.empty(n_skipped, np.int64)
    s_off[is_tab] = table_lo + np.cumsum(tab_len_all) - tab_len_all
    s_off[~is_tab] = table_lo + n_table_bytes + np.cumsum(sk_len) - sk_len

    # Per-window columns in prediction-list order: skipped, then model.
    w_name = np.concatenate([
        cat(s_name, np.int64),
        np.repeat(
            np.fromiter(
                (intern(z.name) for z in model_zmws), np.int64,
                len(model_zmws),
            ),
            model_counts,
        ),
    ])
    w_pos = np.concatenate([cat(s_pos, np.int64), all_pos])
    w_off = np.concatenate([
        s_off, np.arange(n_model, dtype=np.int64) * row_length,
    ])
    w_len = np.concatenate([s_len, np.full(n_model, row_length, np.int64)])
    n_windows = len(w_name)

    # Python string order of the names, as sorted() on the tuples gives.
    rank = np.empty(len(names), np.int64)
    rank[sorted(range(len(names)), key=names.__getitem__)] = np.arange(
        len(names)
    )
    w_rank = rank[w_name]
    # lexsort is stable: ties keep prediction-list order.
    order = np.lexsort((w_pos, w_rank))
    w_rank, w_pos = w_rank[order], w_pos[order]
    w_off, w_len = w_off[order], w_len[order]

    if n_windows:
        first = np.flatnonzero(np.r_[True, w_rank[1:] != w_rank[:-1]])
    else:
        first = np.empty(0, np.int64)
    counts = np.diff(np.r_[first, n_windows])
    k = np.arange(n_windows) - np.repeat(first, counts)
    if n_windows:
        missing = np.logical_or.reduceat(w_pos > k * max_length, first)
        empty = missing | (np.add.reduceat(w_len, first) == 0)
    else:
        empty = np.empty(0, bool)
    keep = ~np.repeat(empty, counts)
    read_seg_start = np.zeros(len(first) + 1, np.int64)
    np.cumsum(np.where(empty, 0, counts), out=read_seg_start[1:])

    # preds[0] of each read: a skipped window carries its own tags, a
    # model window its ZMW's.
    sorted_names = sorted(names)
    model_owner = np.repeat(np.arange(len(model_zmws)), model_counts)
    read_names: List[str] = []
    read_metadata: List[ReadMetadata] = []
    for w in first:
        read_names.append(sorted_names[w_rank[w]])
        src = int(order[w])
        if src >= n_skipped:
            o = model_zmws[model_owner[src - n_skipped]]
        elif is_tab[src]:
            # What a skipped object of this ZMW would carry.
            o = zmws[skip_owner[src]]
        else:
            o = skipped[skip_owner[src]]
        read_metadata.append((o.ec, o.np_num_passes, o.rq, o.rg))

    return StitchPlan(
        read_names=read_names,
        read_empty=empty,
        read_seg_start=read_seg_start,
        read_metadata=read_metadata,
        seg_off=w_off[keep].astype(np.int32),
        seg_len=w_len[keep].astype(np.int32),
        extra_bases=extra_bases,
        extra_quals=extra_quals,
        n_model=n_model,
        row_length=row_length,
        n_table_bytes=n_table_bytes,
    )


def finish_reads(
    plan: StitchPlan,
    seq_out: np.ndarray,
    qual_out: np.ndarray,
    out_off: np.ndarray,
    options: Any,
    outcome_counter: stitch_utils.OutcomeCounter,
) -> Iterator[Tuple[str, bytes, bytes, ReadMetadata]]:
    """Applies the ``stitch_to_fastq`` outcome taxonomy to compacted bytes.

    ``options`` provides ``min_quality`` and ``min_length``. Yields
    ``(name, seq_bytes, qual_bytes, first_window_metadata)`` per successful
    read, in output order; ``outcome_counter`` advances as reads are
    consumed.
    """
    for r, name in enumerate(plan.read_names):
        if plan.read_empty[r]:
            outcome_counter.empty_sequence += 1
            continue
        lo = int(out_off[plan.read_seg_start[r]])
        hi = int(out_off[plan.read_seg_start[r + 1]])
        if hi == lo:
            outcome_counter.only_gaps += 1
            continue
        qual = qual_out[lo:hi]
        # Same function on the same int64 values in the same order as
        # stitch.is_quality_above_threshold: parity is bit-exact.
        avg = phred.avg_phred(qual.astype(np.int64) - 33)
        if not round(avg, 5) >= options.min_quality:
            outcome_counter.failed_quality_filter += 1
            continue
        if hi - lo < options.min_length:
            outcome_counter.failed_length_filter += 1
            continue
        outcome_counter.success += 1
        yield (
            name, seq_out[lo:hi].tobytes(), qual.tobytes(),
            plan.read_metadata[r],
        )
