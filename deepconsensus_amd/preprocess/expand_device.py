"""Device-side alignment expansion: raw BAM records on the host, the
unspaced element streams of spacing_device.py built on the device.

With spacing_mode "device" a worker still decodes every subread record
(bam.decode_record), expands it (expand.expand_clip_indent) and re-encodes it
(spacing_device.build_unspaced) before three bytes per expanded element
cross the pool pipe. All of that is a function of the cigar ops, and the
record already holds the operands in their densest form. This module ships
the record's operands and a normalized op table instead:

* ``build_raw``          — worker, per ZMW: ``ZmwRaw`` from the undecoded
  records of a feeder.RawZmwJob, or None (the ZMW is then materialized and
  takes the spacing path); O(n_ops) work per read, no per-base array.
* ``pack_expand``        — main thread, called by spacing_device.pack_spacing:
  operands back to back, one op table and one read table (``ExpandBatch``),
  validated by ``validate_expand_tables``.
* expansion              — ``ops/hip/cigar_expand.hip`` on the device, or its
  numpy twin ``expand_reads_numpy`` (CPU backend and test oracle). It writes
  ``codes[n] | pw[n] | ip[n]`` per read into the ``src`` buffer of the
  spacing batch, the bytes build_unspaced would have shipped.

expand.py (trim_insertions, expand_clip_indent) and the C++ ``expand_read``
are the semantics. Element ``e`` of a read belongs to the last op row with
``out_start <= e``; with ``q = q_start + (e - out_start)`` an EMIT or
EMIT_INS row gives (LUT[nibble q] | INS_FLAG on an insertion, pw[t], ip[t]),
``t = q`` forward and ``l_seq - 1 - q`` reverse; a GAP row gives (0, 0, 0).
"""
from __future__ import annotations

import collections
import dataclasses
import functools
import struct
from typing import Any, Callable, List, Optional, Sequence, Tuple

import numpy as np

from deepconsensus_amd.dcio import bam
from deepconsensus_amd.preprocess import blob as blob_lib
from deepconsensus_amd.preprocess import featurize_device, spacing_device
from deepconsensus_amd.preprocess.spacing_device import INS_FLAG, MAX_RUN
from deepconsensus_amd.utils import constants

# Kinds of an op row.
EMIT, EMIT_INS, GAP, DROP, END = range(5)
OP_KIND, OP_OUT, OP_Q = range(3)
OP_COLS = 3
# Columns of an xr_tab row.
(XR_DST, XR_N, XR_OP0, XR_NOPS, XR_SEQ, XR_LSEQ, XR_TAG,
 XR_REVERSE) = range(8)
XR_COLS = 8

# Why a ZMW leaves this path; each cause has a counter. The last six are
# build_unspaced's, under its names.
FALLBACK_CAUSES = (
    "decoded_records", "smart_windows", "missing_tag", "pw_ip_type",
    "tag_length", "unknown_op", "cigar_length", "trim_odd_op", "inner_clip",
    "empty_read", "sn_shape", "ccs_quality", "past_ccs", "long_run",
)


fallback_counter = functools.partial(blob_lib.fallback_counter, "expand")


# 4-bit sequence code -> base id, from the two tables the host path goes
# through (decode_record's letters, then encode_bases).
NT16_LUT = spacing_device.encode_bases(
    np.array(list(bam._SEQ_NT16), dtype="<U1"))

# Per cigar op code M I D N S H P = X: kind, query consumed, CCS consumed.
_N_OPS = 9
_KIND_OF = np.array([EMIT, EMIT_INS, GAP, GAP, DROP, DROP, DROP, EMIT, EMIT],
                    np.int64)
_USES_Q = np.array([1, 1, 0, 0, 1, 0, 0, 1, 1], np.int64)
_USES_REF = np.array([1, 0, 1, 1, 0, 0, 0, 1, 1], np.int64)


@dataclasses.dataclass(kw_only=True)
class ZmwRaw(spacing_device.ZmwBeforeSpacing):
    """One ZMW before expansion: the operands and op tables of its
    records. Packs like a spacing_device.ZmwUnspaced whose reads are born
    on the device."""

    raw_records = True

    raw: np.ndarray  # uint8: per read packed_seq | pw[l_seq] | ip[l_seq]
    ops: np.ndarray  # int32 [sum(n_ops), 3]: (kind, out_start, q_start)
    n_ops: np.ndarray  # int32 [n_sub], sentinel row included
    l_seq: np.ndarray  # int32 [n_sub]
    # The decoded CCS read, for the worker's window triage only: cleared
    # before the ZMW crosses the pool pipe.
    ccs_read: Any = None

    def _no_subreads(self) -> dict:
        return dict(
            super()._no_subreads(), raw=np.empty(0, np.uint8),
            ops=np.empty((0, OP_COLS), np.int32),
            n_ops=np.empty(0, np.int32), l_seq=np.empty(0, np.int32))


class _Fallback(Exception):
    """Carries the cause out of the per-read parse."""


def _parse_read(buf: bytes, ins_trim: int, counter: collections.Counter):
    """Operands, op table and CCS footprint of one subread record by
    fixed-offset peeks: (packed seq view, pw view, ip view, sn, reverse,
    l_seq, op table int64 [n_ops + 1, 3], n_elem, n_ref, insertion ref
    positions, insertion lengths). Counts trim_insertions' counters."""
    (_ref_id, pos, l_read_name, _mapq, _bin, n_cigar, flag,
     l_seq) = struct.unpack_from("<llBBHHHl", buf, 0)
    cig_off = 32 + l_read_name
    seq_off = cig_off + 4 * n_cigar
    n_seq_bytes = (l_seq + 1) // 2
    tags = bam.raw_tag_views(buf, ("pw", "ip", "sn"),
                             off=seq_off + n_seq_bytes + l_seq)
    if len(tags) != 3:
        raise _Fallback("missing_tag")
    (pw_type, pw), (ip_type, ip) = tags["pw"], tags["ip"]
    if pw_type != "C" or ip_type != "C" or not (
            isinstance(pw, np.ndarray) and isinstance(ip, np.ndarray)):
        raise _Fallback("pw_ip_type")
    if len(pw) != l_seq or len(ip) != l_seq:
        raise _Fallback("tag_length")

    cig = np.frombuffer(buf, "<u4", n_cigar, cig_off)
    op = (cig & 0xF).astype(np.int64)
    ln = (cig >> 4).astype(np.int64)
    if (op >= _N_OPS).any():
        raise _Fallback("unknown_op")
    trimmed = np.zeros(n_cigar, bool)
    if ins_trim > 0:
        if np.isin(op, (constants.CREF_SKIP, constants.CHARD_CLIP,
                        constants.CPAD)).any():
            raise _Fallback("trim_odd_op")
        trimmed = (op == constants.CINS) & (ln > ins_trim)
    kind = _KIND_OF[op]
    kind[trimmed] = DROP
    uses_q = _USES_Q[op] * ln
    if int(uses_q.sum()) != l_seq:
        raise _Fallback("cigar_length")
    # Hard clips and pads are no part of the alignment; a soft clip and a
    # trimmed insertion consume query without being body ops.
    body = np.flatnonzero(kind != DROP)
    if len(body):
        inner = op[body[0] : body[-1] + 1] == constants.CSOFT_CLIP
        if inner.any():
            raise _Fallback("inner_clip")
    if ins_trim > 0 and n_cigar:
        n_trimmed = int(trimmed.sum())
        if n_trimmed:
            counter["zmw_trimmed_insertions"] += n_trimmed
            counter["zmw_trimmed_insertions_bp"] += int(ln[trimmed].sum())
        counter["zmw_total_bp"] += int(ln.sum())

    pos = max(int(pos), 0)
    keep = (op != constants.CHARD_CLIP) & (op != constants.CPAD)
    kind, ln, op, uses_q = kind[keep], ln[keep], op[keep], uses_q[keep]
    out_len = np.where(kind == DROP, 0, ln)
    table = np.empty((len(kind) + 2, OP_COLS), np.int64)
    table[0] = (GAP, 0, 0)  # the indent
    table[1:-1, OP_KIND] = kind
    table[1:-1, OP_OUT] = pos + np.cumsum(out_len) - out_len
    table[1:-1, OP_Q] = np.cumsum(uses_q) - uses_q
    n_elem = pos + int(out_len.sum())
    table[-1] = (END, n_elem, l_seq)

    uses_ref = np.where(kind == DROP, 0, _USES_REF[op] * ln)
    ref_end = pos + np.cumsum(uses_ref)
    ins = kind == EMIT_INS
    return (
        np.frombuffer(buf, np.uint8, n_seq_bytes, seq_off), pw, ip,
        tags["sn"][1], bool(flag & bam.FREVERSE), l_seq, table, n_elem,
        int(ref_end[-1]) if len(ref_end) else pos, ref_end[ins], ln[ins],
    )


def build_raw(
    job: Any,
    config: Any,
    window_widths: Optional[np.ndarray] = None,
    ins_trim: int = 0,
    counter: Optional[collections.Counter] = None,
) -> Optional[ZmwRaw]:
    """ZmwRaw of the undecoded records of ``job`` (a feeder.RawZmwJob), with
    empty tables; replaces RawZmwJob.materialize and build_unspaced. The
    trim_insertions counters of ``ins_trim`` go to ``counter``.

    Returns None, after counting the cause in ``counter`` and nothing
    else, when the ZMW needs the host expansion: decoded records, CCS smart
    windows, a read (kept or beyond max_passes) without a pw, ip or sn tag,
    with pw or ip not a ``B:C`` array or not l_seq long, with a cigar op
    code above 8, a cigar that does not consume l_seq bases, an N, H or P op
    under ins_trim, or a soft clip between body ops; and build_unspaced's
    own empty_read, sn_shape, ccs_quality, past_ccs and long_run.
    """
    from deepconsensus_amd.preprocess import feeder

    def fallback(cause: str) -> None:
        if counter is not None:
            counter[fallback_counter(cause)] += 1
        return None

    if not isinstance(job, feeder.RawZmwJob):
        return fallback("decoded_records")
    if window_widths is not None:
        return fallback("smart_windows")
    trim_counter: collections.Counter = collections.Counter()
    try:
        reads = [_parse_read(buf, ins_trim, trim_counter)
                 for buf in job.read_set]
    except _Fallback as e:
        return fallback(e.args[0])
    ccs = feeder.construct_ccs_read(
        bam.decode_record(job.ccs_bam_read, job.header))
    Lc = len(ccs.bases)
    if Lc == 0 or any(r[7] == 0 for r in reads):
        return fallback("empty_read")
    kept = reads[: config.max_passes]
    sn = np.zeros(4, np.int16)
    if kept:
        sn_raw = np.asarray(kept[0][3])
        if sn_raw.shape != (4,):
            return fallback("sn_shape")
        sn = np.clip(sn_raw, 0, featurize_device.SN_MAX).astype(np.int16)
    q = np.asarray(ccs.base_quality_scores)
    codes = featurize_device.encode_ccs_qualities(q)
    if codes is None or codes.shape != (Lc,) or not q.any():
        return fallback("ccs_quality")

    ins_max = np.zeros(Lc + 1, np.int64)
    for r in reads:
        n_ref, ins_ref, ins_len = r[8:11]
        if n_ref > Lc:
            return fallback("past_ccs")
        if len(ins_ref):
            # One run per slot: insertion ops of one slot add up (exactly,
            # in float64, far below 2^53).
            runs = np.bincount(ins_ref, weights=ins_len, minlength=Lc + 1)
            np.maximum(ins_max, runs.astype(np.int64), out=ins_max)
    # The second bound keeps every table entry inside int32.
    if ins_max.max() > MAX_RUN or max(r[7] for r in reads) >= 2**31:
        return fallback("long_run")

    parts: List[np.ndarray] = []
    for seq, pw, ip, *_ in kept:
        parts += [seq, pw, ip]
    if counter is not None:
        counter.update(trim_counter)
    reverse = np.array([r[4] for r in kept], bool)
    return ZmwRaw(
        raw=np.concatenate(parts) if parts else np.empty(0, np.uint8),
        ops=(np.concatenate([r[6] for r in kept]).astype(np.int32)
             if kept else np.empty((0, OP_COLS), np.int32)),
        n_ops=np.array([len(r[6]) for r in kept], np.int32),
        l_seq=np.array([r[5] for r in kept], np.int32),
        n_elem=np.array([r[7] for r in kept], np.int32),
        strand=np.where(reverse, int(constants.Strand.REVERSE),
                        int(constants.Strand.FORWARD)).astype(np.uint8),
        sn=sn,
        ccs=spacing_device.encode_bases(ccs.bases),
        ccs_q=codes,
        ins_max=ins_max.astype(np.uint16),
        W=Lc + int(ins_max.sum()),
        use_ccs_bq=bool(config.use_ccs_bq),
        max_passes=config.max_passes,
        max_length=config.max_length,
        ccs_read=ccs,
    )


@dataclasses.dataclass
class ExpandBatch:
    """Raw ZMWs of one batch, packed for the cigar_expand kernel.

    ``blob`` is one ``uint8`` buffer holding, at ``offsets[name]``: xr_tab
    int64 [Rn, 8] = (offset of the read in the spacing ``src``, n elements,
    first row in op_tab, n op rows with the sentinel, offset of the packed
    sequence in raw, l_seq, offset of pw in raw (ip follows it), reverse);
    op_tab int32 [n, 3] = (kind, out_start, q_start); raw uint8.
    """

    blob: np.ndarray
    offsets: dict
    xr_tab: np.ndarray
    op_tab: np.ndarray
    raw: np.ndarray


_check = functools.partial(blob_lib.check, "pack_expand")


def validate_expand_tables(
    op_tab: np.ndarray,
    xr_tab: np.ndarray,
    n_raw: int,
    n_src: int,
    n_src_host: int,
    read_tab: np.ndarray,
) -> None:
    """Host validator of the expand tables against the buffer sizes and the
    read table of the spacing batch.

    Raises ValueError unless every read has its op rows inside op_tab, its
    operands inside ``raw`` (pw behind the packed sequence, ip behind pw)
    and its ``3 * n_elem`` bytes inside the device-born part [n_src_host,
    n_src) of ``src``; out_start and q_start start at 0 and do not
    decrease; the last row is (END, n_elem, l_seq) and no other row is END;
    every EMIT / EMIT_INS / DROP row's query range lies inside [0, l_seq];
    destinations are disjoint and each is the (offset, n) of a read_tab
    row.
    """
    op_tab, xr_tab = np.asarray(op_tab), np.asarray(xr_tab)
    _check(op_tab.ndim == 2 and op_tab.shape[1] == OP_COLS
           and op_tab.dtype == np.int32, "op_tab must be int32 [n, 3]")
    _check(xr_tab.ndim == 2 and xr_tab.shape[1] == XR_COLS
           and xr_tab.dtype == np.int64, "xr_tab must be int64 [Rn, 8]")
    _check(max(n_raw, n_src, len(op_tab)) < 2**31,
           "expand batch too large for int32 columns")
    _check(0 <= n_src_host <= n_src, "host part of src outside src")
    read_tab = np.asarray(read_tab)
    if not len(xr_tab):
        return
    dst, n, op0, n_ops, seq_off, l_seq, tag_off, reverse = xr_tab.T
    _check(bool((n >= 1).all()), "read with a length below 1")
    _check(bool(((dst >= n_src_host) & (dst + 3 * n <= n_src)).all()),
           "destination outside the device-born part of src")
    # Offsets and lengths are below 2^31: one int64 key per (offset, n).
    _check(bool(np.isin(dst << 31 | n, read_tab[:, spacing_device.RD_SRC]
                        << 31 | read_tab[:, spacing_device.RD_N]).all()),
           "destination that is no read_tab row")
    order = np.argsort(dst, kind="stable")
    _check(bool((dst[order][:-1] + 3 * n[order][:-1]
                 <= dst[order][1:]).all()), "destinations overlap")
    _check(bool(((n_ops >= 2) & (op0 >= 0)
                 & (op0 + n_ops <= len(op_tab))).all()),
           "op rows past the end of op_tab")
    _check(bool(((l_seq >= 0) & (l_seq < 2**31) & (seq_off >= 0)
                 & (tag_off == seq_off + (l_seq + 1) // 2)
                 & (tag_off + 2 * l_seq <= n_raw)).all()),
           "operands past the end of raw")
    _check(bool(((reverse == 0) | (reverse == 1)).all()),
           "reverse must be 0 or 1")
    # The op rows of all reads, read after read.
    start = np.cumsum(n_ops) - n_ops
    total = int(n_ops.sum())
    rows = op_tab[np.repeat(op0 - start, n_ops) + np.arange(total)].astype(
        np.int64)
    kind, out, q = rows.T
    last = start + n_ops - 1
    _check(bool((out[start] == 0).all() and (q[start] == 0).all()),
           "out_start and q_start must start at 0")
    _check(bool((kind[last] == END).all() and (out[last] == n).all()
                and (q[last] == l_seq).all()),
           "sentinel is not (END, n_elem, l_seq)")
    inner = np.ones(total, bool)
    inner[last] = False  # a row and its successor in the same read
    kind = kind[inner]
    d_out, d_q = (np.append(np.diff(c), 0)[inner] for c in (out, q))
    _check(bool(((kind >= EMIT) & (kind <= DROP)).all()), "unknown op kind")
    _check(bool((d_out >= 0).all() and (d_q >= 0).all()),
           "out_start or q_start decreases")
    # With these three every query range lies inside [0, l_seq] and no
    # element of an EMIT row reads past it.
    _check(bool((d_q[kind == GAP] == 0).all()),
           "GAP row that consumes query")
    _check(bool((d_out[kind <= EMIT_INS] == d_q[kind <= EMIT_INS]).all()),
           "EMIT row whose output and query lengths differ")
    _check(bool((d_out[kind == DROP] == 0).all()), "DROP row with output")


def pack_expand(
    items: Sequence[Tuple[ZmwRaw, np.ndarray]],
    n_src: int,
    n_src_host: int,
    read_tab: np.ndarray,
    alloc: Optional[Callable[[int], np.ndarray]] = None,
) -> ExpandBatch:
    """Packs ``items`` = (ZmwRaw, offsets of its reads in the spacing
    ``src``) back to back and validates the tables. ``alloc`` as in
    pack_batch."""
    n_reads = sum(u.n_sub for u, _ in items)
    sizes = [
        ("xr_tab", np.int64, n_reads * XR_COLS),
        ("op_tab", np.int32, sum(len(u.ops) for u, _ in items) * OP_COLS),
        ("raw", np.uint8, sum(len(u.raw) for u, _ in items)),
    ]
    blob, offsets, views = blob_lib.pack_views(sizes, alloc, "pack_expand")
    xr_tab = views["xr_tab"].reshape(n_reads, XR_COLS)
    op_tab = views["op_tab"].reshape(-1, OP_COLS)
    raw = views["raw"]
    read0 = op0 = raw_off = 0
    for u, dst in items:
        n = u.n_sub
        _check(u.raw.dtype == np.uint8 and u.ops.dtype == np.int32
               and u.ops.ndim == 2 and u.ops.shape[1] == OP_COLS,
               "raw must be uint8 and ops int32 [n, 3]")
        l_seq = np.asarray(u.l_seq, np.int64)
        n_ops = np.asarray(u.n_ops, np.int64)
        _check(l_seq.shape == n_ops.shape == np.shape(dst) == (n,),
               "l_seq, n_ops and the destinations must be [n_sub]")
        _check(bool((l_seq >= 0).all() and (n_ops >= 0).all()),
               "negative l_seq or n_ops")
        size = (l_seq + 1) // 2 + 2 * l_seq
        _check(len(u.raw) == int(size.sum())
               and len(u.ops) == int(n_ops.sum()),
               "raw or ops do not add up to l_seq and n_ops")
        rows = xr_tab[read0 : read0 + n]
        rows[:, XR_DST] = dst
        rows[:, XR_N] = u.n_elem
        rows[:, XR_OP0] = op0 + np.cumsum(n_ops) - n_ops
        rows[:, XR_NOPS] = n_ops
        rows[:, XR_SEQ] = raw_off + np.cumsum(size) - size
        rows[:, XR_LSEQ] = l_seq
        rows[:, XR_TAG] = rows[:, XR_SEQ] + (l_seq + 1) // 2
        rows[:, XR_REVERSE] = u.strand == int(constants.Strand.REVERSE)
        op_tab[op0 : op0 + len(u.ops)] = u.ops
        raw[raw_off : raw_off + len(u.raw)] = u.raw
        read0 += n
        op0 += len(u.ops)
        raw_off += len(u.raw)
    validate_expand_tables(op_tab, xr_tab, len(raw), n_src, n_src_host,
                           read_tab)
    return ExpandBatch(blob=blob, offsets=offsets, xr_tab=xr_tab,
                       op_tab=op_tab, raw=raw)


def expand_reads_numpy(
    raw: np.ndarray,
    op_tab: np.ndarray,
    xr_tab: np.ndarray,
    src: np.ndarray,
) -> None:
    """Numpy twin of the ``cigar_expand`` kernel: writes ``codes[n] | pw[n]
    | ip[n]`` of every read of ``xr_tab`` into ``src``.

    Like the kernel it never trusts the tables: a read whose op rows,
    operands or destination do not lie inside op_tab / raw / src is skipped
    whole; the op index is clamped to the read's rows, q to [0, l_seq) and
    with it t; an element of a row that is neither EMIT nor EMIT_INS, or of
    a read without bases, is (0, 0, 0).
    """
    for name, a in (("raw", raw), ("src", src)):
        if a.dtype != np.uint8 or a.ndim != 1:
            raise ValueError(f"{name} must be flat uint8")
    if op_tab.ndim != 2 or op_tab.shape[1] != OP_COLS or (
            op_tab.dtype != np.int32):
        raise ValueError("op_tab must be int32 [n, 3]")
    if xr_tab.ndim != 2 or xr_tab.shape[1] != XR_COLS:
        raise ValueError("xr_tab must be [Rn, 8]")
    n_raw, n_src, n_rows = len(raw), len(src), len(op_tab)
    for dst, n, op0, n_ops, seq_off, l_seq, tag_off, reverse in (
            xr_tab.astype(np.int64).tolist()):
        if n < 0 or not 0 <= dst <= n_src or n > (n_src - dst) // 3:
            continue
        if n_ops < 1 or not 0 <= op0 <= n_rows or n_ops > n_rows - op0:
            continue
        if not (0 <= l_seq < 2**31 and 0 <= seq_off <= n_raw
                and (l_seq + 1) // 2 <= n_raw - seq_off
                and 0 <= tag_off <= n_raw
                and l_seq <= (n_raw - tag_off) // 2):
            continue
        rows = op_tab[op0 : op0 + n_ops].astype(np.int64)
        e = np.arange(n)
        j = np.searchsorted(rows[:, OP_OUT], e, side="right") - 1
        j = np.clip(j, 0, n_ops - 1)
        kind = rows[j, OP_KIND]
        emit = ((kind == EMIT) | (kind == EMIT_INS)) & (l_seq > 0)
        q = np.clip(rows[j, OP_Q] + e - rows[j, OP_OUT], 0,
                    max(l_seq - 1, 0))
        t = l_seq - 1 - q if reverse else q
        if l_seq:
            byte = raw[seq_off + (q >> 1)]
            nibble = np.where(q & 1, byte & 0xF, byte >> 4)
            code = NT16_LUT[nibble] | np.where(kind == EMIT_INS, INS_FLAG,
                                               0).astype(np.uint8)
            pw = raw[tag_off + t]
            ip = raw[tag_off + l_seq + t]
        else:
            code = pw = ip = np.zeros(n, np.uint8)
        src[dst : dst + n] = np.where(emit, code, 0)
        src[dst + n : dst + 2 * n] = np.where(emit, pw, 0)
        src[dst + 2 * n : dst + 3 * n] = np.where(emit, ip, 0)


def expand_batch_numpy(batch: Any) -> None:
    """CPU backend: the twin on the host ``src`` of a FeaturizeBatch, ahead
    of spacing_device.space_batch_numpy."""
    sp = batch.spacing
    if sp is None or sp.expand is None:
        return
    ex = sp.expand
    expand_reads_numpy(ex.raw, ex.op_tab, ex.xr_tab, sp.src)
