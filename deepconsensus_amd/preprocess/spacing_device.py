"""Device-side subread spacing: unspaced reads on the host, the spaced
``uint8`` planes of featurize_device.py built on the device.

The host path spaces every read of a ZMW (read.py: space_out_subreads ->
Read.put_spacing), wraps them in a DcExample and re-encodes them into planes
(featurize_device.build_planes) before anything crosses the pool pipe. Spacing
has a closed form: with ``Lc`` CCS positions, an element of an expanded read
is an insertion (cigar op I) or consumes one CCS position;

* ``ref(e)``  non-insertion elements before ``e`` in its read,
* ``k(e)``    index of an insertion inside its run,
* ``ins_max[c]``, c in 0..Lc: the longest insertion run with ``ref == c``
  over ALL reads of the ZMW (also those beyond max_passes, and the CCS),
* ``col_ref[c] = c + sum(ins_max[0..c])``, ``slot0[c] = col_ref[c] -
  ins_max[c]``,
* a non-insertion element goes to column ``col_ref[ref]``, an insertion to
  ``slot0[ref] + k``, and ``W = Lc + sum(ins_max)``.

So the worker only needs ``ins_max``: the CCS row (and with it the window
table, the skip triage, the passthrough table and the counters) follows from
it, and the reads ship unspaced, three bytes per element:

* ``build_unspaced``     — worker, per ZMW: ``ZmwUnspaced`` or None (the ZMW
  then takes the host path); ``spaced_ccs_row`` gives the CCS row.
* ``pack_spacing``       — main thread, called by featurize_device.pack_batch:
  reads back to back in one buffer, a ZMW table and a read table
  (``SpacingBatch``), validated by ``validate_spacing_tables``.
* spacing                — ``ops/hip/subread_space.hip`` on the device, or its
  numpy twin ``space_planes_numpy`` (CPU backend and test oracle).
"""
from __future__ import annotations

import collections
import dataclasses
import functools
from typing import Any, Callable, List, Optional, Sequence, Tuple

import numpy as np

from deepconsensus_amd.preprocess import blob as blob_lib
from deepconsensus_amd.preprocess import featurize_device
from deepconsensus_amd.preprocess.featurize_device import (
    TAB_CCS_OFF, TAB_FIXED, TAB_N_SUB, TAB_SUB_OFF, TAB_W,
)
from deepconsensus_amd.utils import constants

INS_FLAG = 0x80  # on the code byte of an insertion
MAX_RUN = 65535  # ins_max is uint16

# Columns of an sp_tab row and of a read_tab row.
(SP_ZMW, SP_READ0, SP_NREAD, SP_LC, SP_INS_OFF, SP_CCS_SRC,
 SP_FLAGS) = range(7)
SP_COLS = 7
SP_WANT_Q = 1  # SP_FLAGS bit: the ZMW's ccs_q plane is written
RD_SP, RD_SRC, RD_N = range(3)
RD_COLS = 3

# Why a ZMW keeps the host path; each cause has a counter.
FALLBACK_CAUSES = (
    "smart_windows", "label", "empty_read", "pw_ip_dtype", "sn_shape",
    "ccs_quality", "past_ccs", "long_run",
)


fallback_counter = functools.partial(blob_lib.fallback_counter, "spacing")
encode_bases = featurize_device.encode_bases


@dataclasses.dataclass(kw_only=True)
class ZmwBeforeSpacing(featurize_device.ZmwTables):
    """One ZMW whose planes are built on the device: the CCS, ``ins_max``
    and the element count of each of its ``n_sub = min(n_subreads,
    max_passes)`` reads. ZmwUnspaced adds the expanded reads,
    expand_device.ZmwRaw the records they expand from."""

    unspaced = True

    n_elem: np.ndarray  # int32 [n_sub]
    ccs: np.ndarray  # uint8 [Lc] CCS base ids, unspaced
    ccs_q: np.ndarray  # uint8 [Lc] CCS quality codes q + 1, unspaced
    ins_max: np.ndarray  # uint16 [Lc + 1]
    W: int
    use_ccs_bq: bool
    want_q: bool = False  # a passthrough table reads the ccs_q plane

    @property
    def n_sub(self) -> int:
        return len(self.n_elem)

    @property
    def width(self) -> int:
        return self.W

    @property
    def Lc(self) -> int:
        return len(self.ccs)

    @property
    def has_bq(self) -> bool:
        return bool(self.use_ccs_bq)

    @property
    def wants_q(self) -> bool:
        return bool(self.want_q)

    def need_q(self, needed: bool) -> None:
        self.want_q = needed

    def _no_subreads(self) -> dict:
        return dict(n_elem=np.empty(0, np.int32))


@dataclasses.dataclass(kw_only=True)
class ZmwUnspaced(ZmwBeforeSpacing):
    """One ZMW before spacing: its expanded reads, three bytes per
    element."""

    src: np.ndarray  # uint8: per read codes[n] | pw[n] | ip[n]

    def _no_subreads(self) -> dict:
        return dict(super()._no_subreads(), src=np.empty(0, np.uint8))


def insertion_runs(cigar: np.ndarray, Lc: int) -> Optional[np.ndarray]:
    """Insertion run length per CCS slot 0..Lc of one read (int64), or
    None when the read consumes more than Lc CCS positions."""
    nonins = cigar != constants.CINS
    n_ref = int(np.count_nonzero(nonins))
    if n_ref > Lc:
        return None
    if n_ref == len(cigar):
        return np.zeros(Lc + 1, np.int64)
    # A read has one run per slot, so the count of insertions with a given
    # ref is that run's length.
    ref = np.cumsum(nonins)[~nonins]
    return np.bincount(ref, minlength=Lc + 1)


def column_of_elements(cigar: np.ndarray,
                       ins_max: np.ndarray) -> np.ndarray:
    """Spaced column of every element of a read (the closed form above):
    what space_out_subreads leaves in ``Read._seq_indices``."""
    nonins = cigar != constants.CINS
    ins = np.asarray(ins_max, np.int64)
    col_ref = np.arange(len(ins)) + np.cumsum(ins)
    idx = np.arange(len(cigar))
    ref = np.cumsum(nonins) - nonins
    last = np.maximum.accumulate(np.where(nonins, idx, -1))
    k = idx - 1 - last
    return np.where(nonins, col_ref[ref], col_ref[ref] - ins[ref] + k)


def build_unspaced(
    reads: Sequence[Any],
    ccs: Any,
    config: Any,
    window_widths: Optional[np.ndarray] = None,
    counter: Optional[collections.Counter] = None,
) -> Optional[ZmwUnspaced]:
    """ZmwUnspaced of the expanded subreads ``reads`` and the ``ccs`` read
    (both as expand_clip_indent / construct_ccs_read leave them), with
    empty tables; replaces space_out_subreads, DcExample and build_planes.

    Returns None, after counting the cause in ``counter``, when the ZMW
    needs the host path: CCS smart windows, a label, an empty read, pw/ip
    not ``uint8``, ``sn`` not [4], CCS qualities that put_spacing would
    not space (all zero) or that do not fit the uint8 code, a read that
    runs past the CCS, or an insertion run longer than 65,535.
    """

    def fallback(cause: str) -> None:
        if counter is not None:
            counter[fallback_counter(cause)] += 1
        return None

    if window_widths is not None:
        return fallback("smart_windows")
    if any(r.truth_range is not None for r in list(reads) + [ccs]):
        return fallback("label")
    Lc = len(ccs.bases)
    if Lc == 0 or any(len(r.bases) == 0 for r in reads):
        return fallback("empty_read")
    kept = list(reads[: config.max_passes])
    if any(r.pw.dtype != np.uint8 or r.ip.dtype != np.uint8 for r in kept):
        return fallback("pw_ip_dtype")
    sn = np.zeros(4, np.int16)
    if kept:
        sn_raw = np.asarray(kept[0].sn)
        if sn_raw.shape != (4,):
            return fallback("sn_shape")
        sn = np.clip(sn_raw, 0, featurize_device.SN_MAX).astype(np.int16)
    q = np.asarray(ccs.base_quality_scores)
    codes = featurize_device.encode_ccs_qualities(q)
    if codes is None or codes.shape != (Lc,) or not q.any():
        return fallback("ccs_quality")

    ins_max = np.zeros(Lc + 1, np.int64)
    for r in list(reads) + [ccs]:
        runs = insertion_runs(r.cigar, Lc)
        if runs is None:
            return fallback("past_ccs")
        np.maximum(ins_max, runs, out=ins_max)
    if ins_max.max() > MAX_RUN:
        return fallback("long_run")

    parts: List[np.ndarray] = []
    for r in kept:
        code = encode_bases(r.bases)
        code[r.cigar == constants.CINS] |= INS_FLAG
        parts += [code, r.pw, r.ip]
    return ZmwUnspaced(
        src=np.concatenate(parts) if parts else np.empty(0, np.uint8),
        n_elem=np.array([len(r.bases) for r in kept], np.int32),
        strand=np.array([int(r.strand) for r in kept], np.uint8),
        sn=sn,
        ccs=encode_bases(ccs.bases),
        ccs_q=codes,
        ins_max=ins_max.astype(np.uint16),
        W=Lc + int(ins_max.sum()),
        use_ccs_bq=bool(config.use_ccs_bq),
        max_passes=config.max_passes,
        max_length=config.max_length,
    )


def spaced_ccs_row(
    u: ZmwUnspaced, ccs_idx: np.ndarray
) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """The spaced CCS row from ``ins_max`` alone: (base ids uint8 [W],
    ccs_idx [W], qualities int64 [W], ccs_width), gap columns 0 / -1 / -1
    as put_spacing leaves them; ccs_width is DcExample.ccs_width."""
    Lc = u.Lc
    cols = np.arange(Lc) + np.cumsum(u.ins_max[:Lc], dtype=np.int64)
    ids = np.zeros(u.W, np.uint8)
    ids[cols] = u.ccs
    idx = np.full(u.W, -1)
    idx[cols] = ccs_idx
    bq = np.full(u.W, -1)
    bq[cols] = u.ccs_q.astype(np.int64) - 1
    return ids, idx, bq, int(cols[-1]) + 1


@dataclasses.dataclass
class SpacingBatch:
    """Unspaced ZMWs of one batch, packed for the subread_space kernel.

    ``blob`` is one ``uint8`` buffer holding, at ``offsets[name]``:
    sp_tab int64 [S, 7] = (row of the ZMW in zmw_tab, first row in
    read_tab, n_reads, Lc, offset of its Lc + 1 entries in ins_max, offset
    of its CCS ids in src, flags); read_tab int64 [Rn, 3] = (sp_tab row,
    offset in src, n elements); ins_max uint16; src uint8. A read is
    codes[n] | pw[n] | ip[n]; a ZMW's CCS is ids[Lc] | quality codes[Lc].
    """

    blob: np.ndarray
    offsets: dict
    sp_tab: np.ndarray
    read_tab: np.ndarray
    ins_max: np.ndarray
    src: np.ndarray
    # expand_mode "device": the reads of expand_device.ZmwRaw items are not
    # packed; their 3 * n_elem bytes are reserved behind the ``n_src_host``
    # bytes the host wrote, and ``expand`` (expand_device.ExpandBatch) holds
    # what the cigar_expand kernel or its twin fills them from. ``n_src`` is
    # the whole length; with ``device_src`` the host ``src`` ends at
    # n_src_host and the caller allocates the rest on the device.
    n_src: int = 0
    n_src_host: int = 0
    expand: Any = None


_check = functools.partial(blob_lib.check, "pack_spacing")


def validate_spacing_tables(
    sp_tab: np.ndarray,
    read_tab: np.ndarray,
    ins_max: np.ndarray,
    n_src: int,
    zmw_tab: np.ndarray,
    n_sub_bytes: int,
    n_ccs: int,
) -> None:
    """Host validator of the spacing tables against the buffer sizes and
    the plane layout in ``zmw_tab``.

    Raises ValueError unless every ZMW entry names a row of zmw_tab, has
    Lc >= 1 and n_reads == n_sub, its ins_max and CCS source ranges lie
    inside their buffers, Lc + sum(ins_max) equals the W of its planes and
    its planes lie inside the plane arrays; and every read belongs to the
    ZMW whose read range holds it, has 1 <= n <= W and a source range
    inside ``src``.
    """
    sp_tab, read_tab = np.asarray(sp_tab), np.asarray(read_tab)
    _check(sp_tab.ndim == 2 and sp_tab.shape[1] == SP_COLS
           and sp_tab.dtype == np.int64, "sp_tab must be int64 [S, 7]")
    _check(read_tab.ndim == 2 and read_tab.shape[1] == RD_COLS
           and read_tab.dtype == np.int64, "read_tab must be int64 [Rn, 3]")
    ins_max = np.asarray(ins_max)
    _check(ins_max.dtype == np.uint16 and ins_max.ndim == 1,
           "ins_max must be flat uint16")
    _check(max(n_src, len(ins_max), n_sub_bytes, n_ccs) < 2**31,
           "spacing batch too large for int32 columns")
    n_read_rows = len(read_tab)
    csum = np.concatenate([[0], np.cumsum(ins_max, dtype=np.int64)])
    for s, (zi, read0, n_reads, Lc, ins_off, ccs_src, flags) in enumerate(
            sp_tab.tolist()):
        _check(0 <= zi < len(zmw_tab), "ZMW that is not packed")
        row = zmw_tab[zi]
        W, n_sub = int(row[TAB_W]), int(row[TAB_N_SUB])
        _check(Lc >= 1, "CCS length below 1 (negative length)")
        _check(0 <= ins_off and ins_off + Lc + 1 <= len(ins_max),
               "ins_max offset past the end")
        _check(0 <= ccs_src and ccs_src + 2 * Lc <= n_src,
               "CCS source offset past the end")
        total = int(csum[ins_off + Lc + 1] - csum[ins_off])
        _check(Lc + total == W,
               f"Lc + sum(ins_max) = {Lc + total} is not the ZMW width {W}")
        _check(n_reads == n_sub and 0 <= read0
               and read0 + n_reads <= n_read_rows,
               "read range does not match n_sub or the read table")
        _check(0 <= row[TAB_CCS_OFF] and row[TAB_CCS_OFF] + W <= n_ccs,
               "CCS plane past the end")
        _check(0 <= row[TAB_SUB_OFF]
               and row[TAB_SUB_OFF] + 3 * n_sub * W <= n_sub_bytes,
               "subread planes past the end")
        _check(flags in (0, SP_WANT_Q), "unknown flags")
    if n_read_rows:
        sp, off, n = read_tab.T
        _check(bool(((sp >= 0) & (sp < len(sp_tab))).all()),
               "read of a ZMW that is not packed")
        r = np.arange(n_read_rows)
        _check(bool(((r >= sp_tab[sp, SP_READ0])
                     & (r < sp_tab[sp, SP_READ0] + sp_tab[sp, SP_NREAD])
                     ).all()),
               "read outside the read range of its ZMW")
        _check(bool((n >= 1).all()), "read with a length below 1 "
               "(negative length)")
        _check(bool((n <= zmw_tab[sp_tab[sp, SP_ZMW], TAB_W]).all()),
               "read longer than the ZMW width")
        _check(bool(((off >= 0) & (off + 3 * n <= n_src)).all()),
               "read source offset past the end")


def pack_spacing(
    items: Sequence[Tuple[int, Any]],
    zmw_tab: np.ndarray,
    n_sub_bytes: int,
    n_ccs: int,
    alloc: Optional[Callable[[int], np.ndarray]] = None,
    device_src: bool = False,
) -> SpacingBatch:
    """Packs ``items`` = (row in zmw_tab, ZmwUnspaced or
    expand_device.ZmwRaw) back to back and validates the tables. ``alloc``
    as in pack_batch. The reads of a ZmwRaw get their place in ``src``
    behind everything the host writes (see SpacingBatch); ``device_src``
    leaves that part out of the host buffer."""
    n_reads = sum(u.n_sub for _, u in items)
    n_src_host = sum((0 if u.raw_records else len(u.src)) + 2 * u.Lc
                     for _, u in items)
    n_src = n_src_host + sum(
        3 * int(np.sum(u.n_elem, dtype=np.int64))
        for _, u in items if u.raw_records)
    sizes = [
        ("sp_tab", np.int64, len(items) * SP_COLS),
        ("read_tab", np.int64, n_reads * RD_COLS),
        ("ins_max", np.uint16, sum(u.Lc + 1 for _, u in items)),
        ("src", np.uint8, n_src_host if device_src else n_src),
    ]
    blob, offsets, views = blob_lib.pack_views(sizes, alloc, "pack_spacing")
    sp_tab = views["sp_tab"].reshape(len(items), SP_COLS)
    read_tab = views["read_tab"].reshape(n_reads, RD_COLS)
    ins_all, src = views["ins_max"], views["src"]
    src[n_src_host:] = 0  # until the expand twin fills it
    read0 = ins_off = src_off = 0
    born_off = n_src_host
    raw_items = []
    for s, (zi, u) in enumerate(items):
        Lc = u.Lc
        _check(u.ccs.dtype == np.uint8 and u.ccs_q.dtype == np.uint8
               and (u.raw_records or u.src.dtype == np.uint8),
               "sources must be uint8")
        _check(u.ccs_q.shape == (Lc,), "ccs_q must be [Lc]")
        _check(u.ins_max.dtype == np.uint16
               and u.ins_max.shape == (Lc + 1,),
               "ins_max must be uint16 [Lc + 1]")
        n_elem = np.asarray(u.n_elem, np.int64)
        n_bytes = 3 * int(n_elem.sum())
        read_tab[read0 : read0 + u.n_sub, RD_SP] = s
        read_tab[read0 : read0 + u.n_sub, RD_N] = n_elem
        read_off = 3 * (np.cumsum(n_elem) - n_elem)
        if u.raw_records:
            read_tab[read0 : read0 + u.n_sub, RD_SRC] = born_off + read_off
            raw_items.append((u, born_off + read_off))
            born_off += n_bytes
        else:
            _check(len(u.src) == n_bytes,
                   "src is not three bytes per element")
            read_tab[read0 : read0 + u.n_sub, RD_SRC] = src_off + read_off
            src[src_off : src_off + n_bytes] = u.src
            src_off += n_bytes
        sp_tab[s] = (zi, read0, u.n_sub, Lc, ins_off, src_off,
                     SP_WANT_Q if u.want_q else 0)
        src[src_off : src_off + Lc] = u.ccs
        src[src_off + Lc : src_off + 2 * Lc] = u.ccs_q
        src_off += 2 * Lc
        ins_all[ins_off : ins_off + Lc + 1] = u.ins_max
        ins_off += Lc + 1
        read0 += u.n_sub
    validate_spacing_tables(sp_tab, read_tab, ins_all, n_src, zmw_tab,
                            n_sub_bytes, n_ccs)
    expand = None
    if raw_items:
        from deepconsensus_amd.preprocess import expand_device

        expand = expand_device.pack_expand(
            raw_items, n_src, n_src_host, read_tab, alloc=alloc)
    return SpacingBatch(blob=blob, offsets=offsets, sp_tab=sp_tab,
                        read_tab=read_tab, ins_max=ins_all, src=src,
                        n_src=n_src, n_src_host=n_src_host, expand=expand)


def _load_zmw(sp_tab, zmw_tab, s, n_src, n_ins, n_sub_bytes, n_ccs):
    """The kernel's load_zmw: the decoded entry, or None when it is
    skipped."""
    if not 0 <= s < len(sp_tab):
        return None
    zi, read0, n_reads, Lc, ins_off, ccs_src, flags = (
        int(v) for v in sp_tab[s])
    if not 0 <= zi < len(zmw_tab):
        return None
    sub_off, ccs_off, bq_off, n_sub, W = (
        int(v) for v in zmw_tab[zi, :TAB_FIXED])
    ok = (0 <= Lc < n_ins and 0 <= ins_off <= n_ins - (Lc + 1)
          and 0 <= ccs_src <= n_src and 2 * Lc <= n_src - ccs_src
          and W >= 1 and 0 <= ccs_off <= n_ccs and W <= n_ccs - ccs_off
          and 0 <= n_sub <= n_sub_bytes and 0 <= sub_off <= n_sub_bytes
          and n_sub * W <= (n_sub_bytes - sub_off) // 3)
    if not ok:
        return None
    return dict(read0=read0, n_reads=n_reads, Lc=Lc, ins_off=ins_off,
                ccs_src=ccs_src, want_q=bool(flags & SP_WANT_Q),
                sub_off=sub_off, ccs_off=ccs_off, bq_off=bq_off,
                n_sub=n_sub, W=W)


def space_planes_numpy(
    src: np.ndarray,
    ins_max: np.ndarray,
    sp_tab: np.ndarray,
    read_tab: np.ndarray,
    zmw_tab: np.ndarray,
    sub: np.ndarray,
    ccs: np.ndarray,
    ccs_q: np.ndarray,
    ccs_bq: np.ndarray,
    use_ccs_bq: bool,
) -> None:
    """Numpy twin of the ``subread_space`` kernel: scatters the unspaced
    reads and CCS rows into the zero-filled planes ``sub`` / ``ccs`` /
    ``ccs_q`` (uint8) and ``ccs_bq`` (int16, gap columns -1).

    Like the kernel it never trusts the tables: an entry or read whose
    ranges do not lie inside ``src`` / ``ins_max``, whose ZMW is outside
    zmw_tab or whose planes do not lie inside the outputs is skipped whole;
    every ref is clamped to [0, Lc], every column to [0, W), and a read's
    row must be below n_sub.
    """
    for name, a, dtype in (("src", src, np.uint8), ("sub", sub, np.uint8),
                           ("ccs", ccs, np.uint8), ("ccs_q", ccs_q, np.uint8),
                           ("ins_max", ins_max, np.uint16),
                           ("ccs_bq", ccs_bq, np.int16)):
        if a.dtype != dtype or a.ndim != 1:
            raise ValueError(f"{name} must be flat {np.dtype(dtype).name}")
    if sp_tab.ndim != 2 or sp_tab.shape[1] != SP_COLS:
        raise ValueError("sp_tab must be [S, 7]")
    if read_tab.ndim != 2 or read_tab.shape[1] != RD_COLS:
        raise ValueError("read_tab must be [Rn, 3]")
    if zmw_tab.ndim != 2 or (len(zmw_tab) and zmw_tab.shape[1] < TAB_FIXED):
        raise ValueError("zmw_tab must be [Z, >= 5]")
    sizes = (len(src), len(ins_max), len(sub), len(ccs))
    col_refs = {}
    for s in range(len(sp_tab)):
        z = _load_zmw(sp_tab, zmw_tab, s, *sizes)
        if z is None:
            continue
        Lc, W = z["Lc"], z["W"]
        ins = ins_max[z["ins_off"] : z["ins_off"] + Lc + 1].astype(np.int64)
        col_ref = np.minimum(np.arange(Lc + 1) + np.cumsum(ins), W)
        col_refs[s] = (z, ins, col_ref)
        cols = np.minimum(col_ref[:Lc], W - 1) + z["ccs_off"]
        q = src[z["ccs_src"] + Lc : z["ccs_src"] + 2 * Lc]
        ccs[cols] = src[z["ccs_src"] : z["ccs_src"] + Lc]
        if z["want_q"] and W <= len(ccs_q) - z["ccs_off"]:
            ccs_q[cols] = q
        bq_off = z["bq_off"]
        if use_ccs_bq and 0 <= bq_off <= len(ccs_bq) and (
                W <= len(ccs_bq) - bq_off):
            # Columns [max(col_ref - ins, 0), col_ref) of every slot.
            lo = np.maximum(col_ref - ins, 0)
            covered = np.zeros(W + 1, np.int64)
            np.add.at(covered, lo, 1)
            np.add.at(covered, col_ref, -1)
            gap = np.cumsum(covered)[:W] > 0
            plane = ccs_bq[bq_off : bq_off + W]
            plane[gap] = -1
            plane[cols - z["ccs_off"]] = q.astype(np.int16) - 1
    for r in range(len(read_tab)):
        s, src_off, n = (int(v) for v in read_tab[r])
        if s not in col_refs:
            continue
        z, ins, col_ref = col_refs[s]
        row = r - z["read0"]
        if not (0 <= row < z["n_reads"] and row < z["n_sub"]):
            continue
        if n < 0 or not 0 <= src_off <= len(src) or (
                n > (len(src) - src_off) // 3):
            continue
        Lc, W = z["Lc"], z["W"]
        code = src[src_off : src_off + n]
        nonins = (code & INS_FLAG) == 0
        idx = np.arange(n)
        ref = np.minimum(np.cumsum(nonins) - nonins, Lc)
        last = np.maximum.accumulate(np.where(nonins, idx, -1)) if n else idx
        col = np.where(nonins, col_ref[ref],
                       col_ref[ref] - ins[ref] + idx - 1 - last)
        col = np.clip(col, 0, W - 1)
        plane = z["n_sub"] * W
        dst = z["sub_off"] + row * W + col
        sub[dst] = code & 0x7F
        sub[dst + plane] = src[src_off + n : src_off + 2 * n]
        sub[dst + 2 * plane] = src[src_off + 2 * n : src_off + 3 * n]


def space_batch_numpy(batch: Any) -> None:
    """CPU backend: the twin on the host planes of a FeaturizeBatch."""
    sp = batch.spacing
    if sp is None:
        return
    space_planes_numpy(
        sp.src, sp.ins_max, sp.sp_tab, sp.read_tab, batch.zmw_tab,
        batch.sub, batch.ccs, batch.ccs_q, batch.ccs_bq, batch.use_ccs_bq,
    )
