"""Device-side window featurization: compact planes on the host, the
``int16 [B, R, L]`` model input expanded on the device.

The host featurizer (windows.py: iter_feature_dicts) expands every window
into an 85 x 100 int16 matrix in the worker; the matrix is then pickled,
concatenated, staged and copied to the device. Nearly all of it is
redundant: column slices of per-ZMW planes the worker already holds, one
strand value per row, four SN values, and zero padding. This module ships
the planes instead:

* ``build_planes``  — worker, per ZMW: the ``uint8`` planes of the spaced
  ZMW (``ZmwPlanes``), or None when the ZMW needs the per-window path.
* ``pack_batch``    — main thread, per ZMW batch: planes back to back in
  one buffer, a per-ZMW table and a per-window table (``FeaturizeBatch``),
  validated on the host.
* expansion         — ``ops/hip/window_featurize.hip`` on the device, or
  its numpy twin ``featurize_windows_numpy`` (CPU backend and test oracle).

Window enumeration, counters and the skip triage stay in windows.py /
quick_inference.py and are shared with the host path.

With passthrough_mode "device" the planes also carry the skipped windows:
a passthrough table (``ZmwPlanes.pt_*``) and the CCS qualities as ``uint8``
codes (``ccs_q``). ``pack_batch`` turns them into ``pt_tab`` and
``ops/hip/passthrough_fill.hip`` (numpy twin: ``passthrough_fill_numpy``)
writes their base ids and QVs into the stitch buffer.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Any, Callable, List, Optional, Sequence, Tuple

import numpy as np

from deepconsensus_amd.preprocess import blob as blob_lib
from deepconsensus_amd.preprocess.windows import DcExample
from deepconsensus_amd.utils import constants

# format_rows' clipping (models/config.py PW_MAX / IP_MAX / SN_MAX).
PW_MAX = 255
IP_MAX = 255
SN_MAX = 500

# Leading columns of a zmw_tab row; strand[max_passes] and sn[4] follow.
TAB_SUB_OFF, TAB_CCS_OFF, TAB_BQ_OFF, TAB_N_SUB, TAB_W = range(5)
TAB_FIXED = 5


def tensor_height(max_passes: int, use_ccs_bq: bool) -> int:
    return 4 * max_passes + 1 + int(bool(use_ccs_bq)) + 4


@dataclasses.dataclass(kw_only=True)
class ZmwTables:
    """What ZmwWindows.planes holds for one ZMW on the plane path, whichever
    stage its reads are in: the window table, the passthrough table and the
    per-read constants. ZmwPlanes (spaced planes), spacing_device.ZmwUnspaced
    (reads before spacing) and expand_device.ZmwRaw (records before
    expansion) add the reads; each says how many it keeps (``n_sub``), how
    wide its planes are (``width``), whether it carries the ccs_bq and ccs_q
    planes (``has_bq``, ``wants_q``; ``need_q`` drops the latter) and what
    remains of it without model windows (``without_subreads``)."""

    unspaced = False  # the planes are built on the device (spacing_device)
    raw_records = False  # ... from reads born on the device (expand_device)

    strand: np.ndarray  # uint8 [n_sub]
    sn: np.ndarray  # int16 [4], clipped to 0..SN_MAX
    max_passes: int
    max_length: int
    win_start: np.ndarray = blob_lib.empty_column(np.int32)  # model-bound
    win_w: np.ndarray = blob_lib.empty_column(np.int32)  # windows only
    # Passthrough table (passthrough_mode "device"): one entry per skipped
    # window, columns [start, start + w) padded to ``width`` (above
    # max_length for an overflow window). Empty when the ZMW keeps host
    # ``skipped`` objects.
    pt_start: np.ndarray = blob_lib.empty_column(np.int32)
    pt_w: np.ndarray = blob_lib.empty_column(np.int32)
    pt_width: np.ndarray = blob_lib.empty_column(np.int32)
    pt_pos: np.ndarray = blob_lib.empty_column(np.int64)  # window_pos

    @property
    def n_windows(self) -> int:
        return len(self.win_start)

    @property
    def n_passthrough(self) -> int:
        return len(self.pt_start)

    def _no_subreads(self) -> dict:
        """The read fields of the subclass, emptied."""
        raise NotImplementedError

    def without_subreads(self):
        """What a ZMW without model windows still needs: the CCS row."""
        return dataclasses.replace(
            self, strand=np.empty(0, np.uint8), sn=np.zeros(4, np.int16),
            **self._no_subreads())


@dataclasses.dataclass(kw_only=True)
class ZmwPlanes(ZmwTables):
    """Compact model input of one ZMW: ``n_sub = min(n_subreads,
    max_passes)`` subreads over the spaced width W."""

    sub: np.ndarray  # uint8 [3, n_sub, W]: base ids, pw, ip
    ccs: np.ndarray  # uint8 [W] CCS base ids
    ccs_bq: Optional[np.ndarray]  # int16 [W], only with use_ccs_bq
    # CCS quality of every column coded q + 1 (0 = the -1 padding value);
    # None means the passthrough table is empty.
    ccs_q: Optional[np.ndarray] = None  # uint8 [W]

    @property
    def n_sub(self) -> int:
        return self.sub.shape[1]

    @property
    def width(self) -> int:
        return self.ccs.shape[0]

    @property
    def has_bq(self) -> bool:
        return self.ccs_bq is not None

    @property
    def wants_q(self) -> bool:
        return self.ccs_q is not None

    def need_q(self, needed: bool) -> None:
        if not needed:
            self.ccs_q = None

    def _no_subreads(self) -> dict:
        return dict(sub=np.empty((3, 0, self.width), np.uint8))


def encode_ccs_qualities(qualities: Any) -> Optional[np.ndarray]:
    """CCS qualities as ``uint8`` codes q + 1, or None when a value is not
    an integer in -1..254 (the ZMW then keeps the host passthrough)."""
    q = np.asarray(qualities)
    if q.ndim != 1:
        return None
    if q.dtype.kind not in "iu":
        if q.dtype.kind != "f" or not np.array_equal(q, np.floor(q)):
            return None
    if q.size and (q.min() < -1 or q.max() > 254):
        return None
    return (q.astype(np.int64) + 1).astype(np.uint8)


# Code point -> base id; anything outside the vocabulary is id 0.
_BASE_LUT = np.zeros(128, np.uint8)
for _k, _base in enumerate(constants.SEQ_VOCAB):
    if _k:
        _BASE_LUT[ord(_base)] = _k


def encode_bases(bases: np.ndarray) -> np.ndarray:
    """Base ids of a ``<U1`` array in one table lookup."""
    cp = np.ascontiguousarray(bases).view(np.uint32)
    return _BASE_LUT[np.minimum(cp, 127)]


def build_planes(dc: DcExample) -> Optional[ZmwPlanes]:
    """Planes of a spaced ZMW, with an empty window table.

    Returns None when the ZMW does not meet the fast-path precondition
    (training ZMW, irregular read widths, pw/ip not already ``uint8``,
    qualities not spaced to W): the caller then featurizes that ZMW on
    the host. Values equal what iter_feature_dicts(pw_max=255,
    ip_max=255, sn_max=500, out_dtype=int16) puts into its matrices.
    """
    if not dc.is_evenly_spaced_inference:
        return None
    config = dc.config
    subs = dc.subreads[: config.max_passes]
    n, W = len(subs), dc.width
    if any(r.pw.dtype != np.uint8 or r.ip.dtype != np.uint8 for r in subs):
        return None
    sub = np.zeros((3, n, W), np.uint8)
    sn = np.zeros(4, np.int16)
    if n:
        sub[0] = encode_bases(np.stack([r.bases for r in subs]))
        # uint8 is 0..255 already; the clip documents format_rows' bound.
        np.clip(np.stack([r.pw for r in subs]), 0, PW_MAX, out=sub[1])
        np.clip(np.stack([r.ip for r in subs]), 0, IP_MAX, out=sub[2])
        sn_raw = np.asarray(subs[0].sn)
        if sn_raw.shape != (4,):
            return None
        sn = np.clip(sn_raw, 0, SN_MAX).astype(np.int16)
    ccs_bq = None
    if config.use_ccs_bq:
        bq = np.asarray(dc.ccs.base_quality_scores)
        if bq.shape != (W,):
            return None
        ccs_bq = bq.astype(np.int16)
    return ZmwPlanes(
        sub=sub,
        strand=np.array([int(r.strand) for r in subs], np.uint8),
        sn=sn,
        ccs=encode_bases(dc.ccs.bases),
        ccs_bq=ccs_bq,
        max_passes=config.max_passes,
        max_length=config.max_length,
    )


def n_model_windows(z: Any) -> int:
    """Model-bound windows of a ZmwWindows-like object, whichever form
    (``rows`` or ``planes``) it carries them in."""
    if z.rows is not None:
        return len(z.rows)
    planes = getattr(z, "planes", None)
    return 0 if planes is None else planes.n_windows


def n_table_passthrough(z: Any) -> int:
    """Skipped windows a ZmwWindows-like object carries as passthrough
    table entries of its planes (not as ``skipped`` objects)."""
    planes = getattr(z, "planes", None)
    return 0 if planes is None else planes.n_passthrough


# Columns of a pt_tab row.
PT_ZMW, PT_START, PT_W, PT_WIDTH, PT_DST = range(5)


def validate_passthrough_table(
    pt_tab: np.ndarray, zmw_widths: Sequence[int]
) -> int:
    """Host validator of a passthrough table against the widths W of the
    packed ZMWs; returns the byte count of the passthrough region.

    Raises ValueError unless, for every entry, zmw_index names a packed
    ZMW, start >= 0, 1 <= w <= width, start + w <= W, dst_off is the
    running sum of the widths before it, and the total stays below 2^31.
    """
    pt_tab = np.asarray(pt_tab)
    _check(pt_tab.ndim == 2 and pt_tab.shape[1] == 5
           and pt_tab.dtype in (np.int32, np.int64),
           "pt_tab must be an integer [P, 5] table")
    if not len(pt_tab):
        return 0
    tab = pt_tab.astype(np.int64)
    zi, start, w, width, dst = tab.T
    widths = np.asarray(zmw_widths, np.int64)
    _check(bool(((zi >= 0) & (zi < len(widths))).all()),
           "passthrough window of a ZMW that is not packed")
    _check(bool((start >= 0).all()), "passthrough window with start < 0")
    _check(bool(((w >= 1) & (w <= width)).all()),
           "passthrough window with w outside 1..width")
    _check(bool((start + w <= widths[zi]).all()),
           "passthrough window ends past the ZMW width")
    _check(bool((dst == np.cumsum(width) - width).all()),
           "passthrough dst_off is not the running sum of the widths")
    total = int(width.sum())
    _check(total < 2**31, "passthrough region too large for int32 offsets")
    return total


@dataclasses.dataclass
class FeaturizeBatch:
    """Planes and tables of one ZMW batch.

    ``blob`` is one ``uint8`` buffer; ``zmw_tab``, ``win_tab``, ``ccs_bq``,
    ``sub`` and ``ccs`` are views into it at ``offsets[name]`` (bytes), so
    one copy moves everything to the device.

    zmw_tab int64 [Z, 5 + max_passes + 4]: element offsets of the ZMW's
    planes in ``sub`` / ``ccs`` / ``ccs_bq``, n_sub, W, strand[max_passes],
    sn[4]. A ZMW's ``sub`` block is its [3, n_sub, W] array, row-major.

    win_tab int32 [n_padded, 3]: (zmw_index, start, w) per model window,
    in concatenation order. zmw_index -1 means the kernel writes zeros:
    tail padding, or a window of a fallback ZMW whose host ``rows`` the
    caller copies in (``fallback_idx`` / ``fallback_rows``).

    With passthrough tables (passthrough_mode "device") the blob also
    holds ``ccs_q`` uint8, laid out like ``ccs`` at the same offsets (zero
    for a ZMW without one), and pt_tab int32 [P, 5]: (zmw_index, start, w,
    width, dst_off) per skipped window, in ZMW order then window order;
    dst_off is the running sum of ``width``, the window's offset inside
    the ``n_pt_bytes`` passthrough region of the stitch buffer. Both are
    empty otherwise.
    """

    blob: np.ndarray
    offsets: dict
    zmw_tab: np.ndarray
    win_tab: np.ndarray
    ccs_bq: np.ndarray  # int16, empty without use_ccs_bq
    sub: np.ndarray
    ccs: np.ndarray
    n_windows: int  # without the tail padding
    n_rows: int
    max_length: int
    max_passes: int
    use_ccs_bq: bool
    fallback_idx: np.ndarray  # int64, ascending window indices
    fallback_rows: Optional[np.ndarray]  # int16 [len(fallback_idx), R, L]
    ccs_q: np.ndarray = blob_lib.empty_column(np.uint8)
    pt_tab: np.ndarray = dataclasses.field(
        default_factory=lambda: np.empty((0, 5), np.int32))
    n_pt_bytes: int = 0
    # spacing_mode "device": the unspaced ZMWs of the batch
    # (spacing_device.SpacingBatch); their planes are zero until the
    # subread_space kernel or its twin has run. ``plane_layout`` maps
    # ccs_bq / sub / ccs / ccs_q to (byte offset, dtype, element count)
    # inside the plane region. With ``device_planes`` the region is not part
    # of ``blob`` (the four host views are empty): the caller allocates it
    # zero-filled on the device and copies in ``host_planes``, the (name,
    # element offset, array) pieces of the ZMWs that were spaced on the
    # host.
    spacing: Any = None
    plane_layout: dict = dataclasses.field(default_factory=dict)
    device_planes: bool = False
    host_planes: list = dataclasses.field(default_factory=list)

    @property
    def plane_nbytes(self) -> int:
        return sum(np.dtype(dtype).itemsize * count
                   for _, dtype, count in self.plane_layout.values())

    def fallback_range(self, lo: int, hi: int) -> Tuple[int, int]:
        """Slice of fallback_idx / fallback_rows inside windows [lo, hi)."""
        k0, k1 = np.searchsorted(self.fallback_idx, [lo, hi])
        return int(k0), int(k1)


_check = functools.partial(blob_lib.check, "pack_batch")


def pack_batch(
    zmws: Sequence[Any],
    pad_multiple: int = 1,
    alloc: Optional[Callable[[int], np.ndarray]] = None,
    device_planes: bool = False,
) -> FeaturizeBatch:
    """Packs the model windows of a ZMW batch for the featurize kernel.

    ``zmws`` are ZmwWindows-like objects carrying either ``planes`` or
    host ``rows``; window order is ZMW order. ``pad_multiple`` pads the
    window table with -1 entries to a multiple of it (fixed-shape graph
    replays). ``alloc(nbytes)`` returns the ``uint8`` buffer to pack
    into (pinned memory, say); numpy allocates otherwise.

    ``planes`` may also be a spacing_device.ZmwUnspaced: the ZMW gets the
    same table rows and the same, zero-filled, slices of the plane arrays,
    and its reads are packed into ``FeaturizeBatch.spacing`` (a second
    ``alloc`` call). ``device_planes`` then leaves the plane arrays out of
    the host buffer (see FeaturizeBatch). An expand_device.ZmwRaw packs
    like a ZmwUnspaced; its records go to ``FeaturizeBatch.spacing.expand``
    (a third ``alloc`` call) and with ``device_planes`` its reads have no
    host bytes at all.

    Raises ValueError when a table entry would make the kernel read
    outside a plane or when the ZMWs disagree on the layout.
    """
    _check(pad_multiple >= 1, "pad_multiple must be positive")
    plane_zmws: List[ZmwTables] = []
    win_parts: List[np.ndarray] = []
    fb_idx: List[np.ndarray] = []
    fb_rows: List[np.ndarray] = []
    n_windows = 0
    layout = None  # (max_passes, max_length, use_ccs_bq)
    rows_shape = None
    pt_parts: List[np.ndarray] = []
    for z in zmws:
        n = n_model_windows(z)
        n_pt = n_table_passthrough(z)
        if not n and not n_pt:
            continue
        if z.rows is not None:
            rows = np.asarray(z.rows)
            _check(rows.ndim == 3 and rows.dtype == np.int16,
                   "fallback rows must be int16 [n, R, L]")
            _check(rows_shape in (None, rows.shape[1:]),
                   "fallback rows of different shapes")
            rows_shape = rows.shape[1:]
            fb_idx.append(np.arange(n_windows, n_windows + n))
            fb_rows.append(rows)
            win_parts.append(np.full((n, 3), -1, np.int32))
            win_parts[-1][:, 1:] = 0
        else:
            p = z.planes
            unspaced = p.unspaced
            this = (int(p.max_passes), int(p.max_length), p.has_bq)
            _check(layout in (None, this),
                   f"ZMWs disagree on (max_passes, max_length, "
                   f"use_ccs_bq): {layout} and {this}")
            layout = this
            n_sub, W = p.n_sub, p.width
            if not unspaced:
                _check(p.sub.dtype == np.uint8
                       and p.sub.shape == (3, n_sub, W),
                       "sub must be uint8 [3, n_sub, W]")
                _check(p.ccs.dtype == np.uint8, "ccs must be uint8")
            _check(n_sub <= p.max_passes,
                   f"n_sub={n_sub} exceeds max_passes={p.max_passes}")
            _check(p.strand.shape == (n_sub,), "strand must be [n_sub]")
            _check(np.shape(p.sn) == (4,), "sn must be [4]")
            if not unspaced and p.ccs_bq is not None:
                _check(p.ccs_bq.dtype == np.int16
                       and p.ccs_bq.shape == (W,),
                       "ccs_bq must be int16 [W]")
            start = np.asarray(p.win_start, np.int64)
            w = np.asarray(p.win_w, np.int64)
            _check(start.shape == w.shape == (n,),
                   "win_start and win_w must be [n_model]")
            _check(bool((start >= 0).all()), "window with start < 0")
            _check(bool(((w >= 1) & (w <= p.max_length)).all()),
                   f"window width outside 1..{p.max_length}")
            _check(bool((start + w <= W).all()),
                   f"window ends past the ZMW width {W}")
            tab = np.empty((n, 3), np.int32)
            tab[:, 0] = len(plane_zmws)
            tab[:, 1] = start
            tab[:, 2] = w
            win_parts.append(tab)
            if not unspaced and p.ccs_q is not None:
                _check(p.ccs_q.dtype == np.uint8 and p.ccs_q.shape == (W,),
                       "ccs_q must be uint8 [W]")
            if n_pt:
                _check(p.wants_q,
                       "passthrough table on a ZMW without ccs_q")
                _check(np.shape(p.pt_w) == np.shape(p.pt_width) == (n_pt,),
                       "pt_start, pt_w and pt_width must be [n_passthrough]")
                pt = np.zeros((n_pt, 5), np.int64)
                pt[:, PT_ZMW] = len(plane_zmws)
                pt[:, PT_START] = p.pt_start
                pt[:, PT_W] = p.pt_w
                pt[:, PT_WIDTH] = p.pt_width
                pt_parts.append(pt)
            plane_zmws.append(p)
        n_windows += n

    if pt_parts:
        pt_all = np.concatenate(pt_parts)
        # The validator rejects width < 1 below, before dst_off is used.
        pt_all[:, PT_DST] = np.cumsum(pt_all[:, PT_WIDTH]) - pt_all[
            :, PT_WIDTH]
    else:
        pt_all = np.empty((0, 5), np.int64)
    n_pt_bytes = validate_passthrough_table(
        pt_all, [p.width for p in plane_zmws])
    with_q = any(p.wants_q for p in plane_zmws)
    unspaced_zmws = [(i, p) for i, p in enumerate(plane_zmws)
                     if p.unspaced]
    device_planes = bool(device_planes and unspaced_zmws)

    if layout is None:
        _check(rows_shape is not None or n_windows == 0, "no layout")
        if rows_shape is not None:
            R, L = rows_shape
            use_ccs_bq = (R - 5) % 4 != 0
            layout = ((R - 5 - int(use_ccs_bq)) // 4, L, use_ccs_bq)
        else:
            layout = (0, 0, False)
    max_passes, max_length, use_ccs_bq = layout
    n_rows = tensor_height(max_passes, use_ccs_bq)
    if rows_shape is not None:
        _check(tuple(rows_shape) == (n_rows, max_length),
               f"fallback rows are {tuple(rows_shape)}, planes expand to "
               f"{(n_rows, max_length)}")

    n_zmw = len(plane_zmws)
    n_padded = -(-n_windows // pad_multiple) * pad_multiple
    n_col = TAB_FIXED + max_passes + 4
    plane_sizes = [
        ("ccs_bq", np.int16,
         sum(p.width for p in plane_zmws) if use_ccs_bq else 0),
        ("sub", np.uint8, sum(3 * p.n_sub * p.width for p in plane_zmws)),
        ("ccs", np.uint8, sum(p.width for p in plane_zmws)),
        ("ccs_q", np.uint8,
         sum(p.width for p in plane_zmws) if with_q else 0),
    ]
    plane_offsets, _ = blob_lib.region_offsets(plane_sizes)
    plane_layout = {name: (plane_offsets[name], dtype, count)
                    for name, dtype, count in plane_sizes}
    sizes = [
        ("zmw_tab", np.int64, n_zmw * n_col),
        ("win_tab", np.int32, n_padded * 3),
        ("pt_tab", np.int32, len(pt_all) * 5),
    ] + [(name, dtype, 0 if device_planes else count)
         for name, dtype, count in plane_sizes]
    blob, offsets, views = blob_lib.pack_views(sizes, alloc, "pack_batch")
    zmw_tab = views["zmw_tab"].reshape(n_zmw, n_col)
    win_tab = views["win_tab"].reshape(n_padded, 3)
    zmw_tab[:] = 0
    sub_off = ccs_off = 0
    host_planes: List[Tuple[str, int, np.ndarray]] = []
    for i, p in enumerate(plane_zmws):
        n_sub, W = p.n_sub, p.width
        sub_size = 3 * n_sub * W
        zmw_tab[i, TAB_SUB_OFF] = sub_off
        zmw_tab[i, TAB_CCS_OFF] = ccs_off
        zmw_tab[i, TAB_BQ_OFF] = ccs_off if use_ccs_bq else 0
        zmw_tab[i, TAB_N_SUB] = n_sub
        zmw_tab[i, TAB_W] = W
        zmw_tab[i, TAB_FIXED : TAB_FIXED + n_sub] = p.strand
        zmw_tab[i, TAB_FIXED + max_passes :] = p.sn
        if p.unspaced:
            # Zero until the spacing kernel (or its twin) fills them.
            pieces = [("sub", sub_off, sub_size, 0), ("ccs", ccs_off, W, 0)]
            if use_ccs_bq:
                pieces.append(("ccs_bq", ccs_off, W, 0))
            if with_q:
                pieces.append(("ccs_q", ccs_off, W, 0))
        else:
            pieces = [("sub", sub_off, sub_size, p.sub.reshape(-1)),
                      ("ccs", ccs_off, W, p.ccs)]
            if use_ccs_bq:
                pieces.append(("ccs_bq", ccs_off, W, p.ccs_bq))
            if with_q and p.ccs_q is not None:
                pieces.append(("ccs_q", ccs_off, W, p.ccs_q))
            elif with_q:
                pieces.append(("ccs_q", ccs_off, W, 0))
        for name, off, count, value in pieces:
            if not device_planes:
                views[name][off : off + count] = value
            elif isinstance(value, np.ndarray) and count:
                host_planes.append((name, off, np.ascontiguousarray(value)))
        sub_off += sub_size
        ccs_off += W
    # Offsets inside the arrays: true by construction, checked anyway.
    _check(sub_off == plane_layout["sub"][2]
           and ccs_off == plane_layout["ccs"][2],
           "plane offsets do not add up to the packed arrays")
    spacing = None
    if unspaced_zmws:
        from deepconsensus_amd.preprocess import spacing_device

        spacing = spacing_device.pack_spacing(
            unspaced_zmws, zmw_tab, sub_off, ccs_off, alloc=alloc,
            device_src=device_planes)
    if n_windows:
        win_tab[:n_windows] = np.concatenate(win_parts)
    win_tab[n_windows:, 0] = -1
    win_tab[n_windows:, 1:] = 0
    pt_tab = views["pt_tab"].reshape(len(pt_all), 5)
    pt_tab[:] = pt_all
    return FeaturizeBatch(
        spacing=spacing, plane_layout=plane_layout,
        device_planes=device_planes, host_planes=host_planes,
        ccs_q=views["ccs_q"], pt_tab=pt_tab, n_pt_bytes=n_pt_bytes,
        blob=blob, offsets=offsets, zmw_tab=zmw_tab, win_tab=win_tab,
        ccs_bq=views["ccs_bq"], sub=views["sub"], ccs=views["ccs"],
        n_windows=n_windows, n_rows=n_rows, max_length=max_length,
        max_passes=max_passes, use_ccs_bq=use_ccs_bq,
        fallback_idx=(np.concatenate(fb_idx) if fb_idx
                      else np.empty(0, np.int64)),
        fallback_rows=np.concatenate(fb_rows) if fb_rows else None,
    )


def featurize_windows_numpy(
    batch: FeaturizeBatch,
    lo: int,
    hi: int,
    R: int,
    L: int,
    max_passes: int,
    use_ccs_bq: bool,
) -> np.ndarray:
    """Numpy twin of the ``window_featurize`` kernel: windows [lo, hi) of
    ``batch.win_tab`` as ``int16 [hi - lo, R, L]``.

    Like the kernel it never trusts the tables: a window whose zmw_index
    is outside the ZMW table, or whose ZMW's planes do not lie inside the
    packed arrays, comes out as zeros; n_sub is clamped to max_passes,
    start to [0, W] and w to [0, min(L, W - start)]. Fallback windows
    (zmw_index -1) are zeros here; the caller copies their rows in.
    """
    if R != tensor_height(max_passes, use_ccs_bq):
        raise ValueError(
            f"R={R} does not match max_passes={max_passes}, "
            f"use_ccs_bq={use_ccs_bq}"
        )
    zmw_tab, win_tab = batch.zmw_tab, batch.win_tab
    if zmw_tab.ndim != 2 or zmw_tab.shape[1] != TAB_FIXED + max_passes + 4:
        raise ValueError("zmw_tab does not have 5 + max_passes + 4 columns")
    if not 0 <= lo <= hi <= len(win_tab):
        raise ValueError("window range outside win_tab")
    sub, ccs, bq_all = batch.sub, batch.ccs, batch.ccs_bq
    mp = max_passes
    out = np.zeros((hi - lo, R, L), np.int16)
    for j in range(hi - lo):
        zi, start, w = (int(v) for v in win_tab[lo + j])
        if not 0 <= zi < len(zmw_tab):
            continue
        row = zmw_tab[zi]
        sub_off, ccs_off, bq_off, n_raw, W = (
            int(v) for v in row[:TAB_FIXED]
        )
        if (
            n_raw < 0 or W < 0 or sub_off < 0 or ccs_off < 0
            or sub_off + 3 * n_raw * W > len(sub)
            or ccs_off + W > len(ccs)
            or (use_ccs_bq and (bq_off < 0 or bq_off + W > len(bq_all)))
        ):
            continue
        n_sub = min(n_raw, mp)
        start = min(max(start, 0), W)
        w = min(max(w, 0), L, W - start)
        x = out[j]
        if n_sub:
            planes = sub[sub_off : sub_off + 3 * n_raw * W].reshape(
                3, n_raw, W
            )
            for f in range(3):
                x[f * mp : f * mp + n_sub, :w] = planes[
                    f, :n_sub, start : start + w
                ]
            x[3 * mp : 3 * mp + n_sub] = row[
                TAB_FIXED : TAB_FIXED + n_sub, None
            ]
            x[R - 4 :] = row[TAB_FIXED + mp :, None]
        x[4 * mp, :w] = ccs[ccs_off + start : ccs_off + start + w]
        if use_ccs_bq:
            x[4 * mp + 1, :w] = bq_all[bq_off + start : bq_off + start + w]
            x[4 * mp + 1, w:] = -1
    return out


def featurize_chunk_numpy(
    batch: FeaturizeBatch, lo: int, hi: int
) -> np.ndarray:
    """CPU backend: the twin plus the host rows of fallback ZMWs."""
    out = featurize_windows_numpy(
        batch, lo, hi, batch.n_rows, batch.max_length, batch.max_passes,
        batch.use_ccs_bq,
    )
    k0, k1 = batch.fallback_range(lo, hi)
    if k1 > k0:
        out[batch.fallback_idx[k0:k1] - lo] = batch.fallback_rows[k0:k1]
    return out


def passthrough_fill_numpy(
    ccs: np.ndarray,
    ccs_q: np.ndarray,
    zmw_tab: np.ndarray,
    pt_tab: np.ndarray,
    qual_lut: np.ndarray,
    bases_out: np.ndarray,
    quals_out: np.ndarray,
) -> None:
    """Numpy twin of the ``passthrough_fill`` kernel: fills the
    passthrough region (``bases_out`` / ``quals_out``, uint8 [n]) from the
    packed ``ccs`` / ``ccs_q`` planes and the passthrough table.

    Entry (zmw_index, start, w, width, dst_off) writes ``width`` bytes at
    ``dst_off``: the CCS ids / ``qual_lut[ccs_q]`` of columns [start,
    start + w), then id 0 / ``qual_lut[0]``. Like the kernel it never
    trusts the tables: an entry whose zmw_index is outside the ZMW table,
    or whose ZMW's planes do not lie inside ``ccs`` / ``ccs_q``, is id 0
    and quality 0 throughout; start is clamped to [0, W], w to [0,
    min(width, W - start)]; only bytes inside [0, n) are written.
    """
    for name, a in (("ccs", ccs), ("ccs_q", ccs_q), ("qual_lut", qual_lut),
                    ("bases_out", bases_out), ("quals_out", quals_out)):
        if a.dtype != np.uint8 or a.ndim != 1:
            raise ValueError(f"{name} must be flat uint8")
    if qual_lut.shape != (256,):
        raise ValueError("qual_lut must have 256 entries")
    if bases_out.shape != quals_out.shape:
        raise ValueError("bases_out and quals_out must be of equal length")
    if zmw_tab.ndim != 2 or (len(zmw_tab) and zmw_tab.shape[1] < TAB_FIXED):
        raise ValueError("zmw_tab must be [Z, >= 5]")
    if pt_tab.ndim != 2 or pt_tab.shape[1] != 5:
        raise ValueError("pt_tab must be [P, 5]")
    n = len(bases_out)
    n_src = min(len(ccs), len(ccs_q))
    for zi, start, w, width, dst in pt_tab.astype(np.int64).tolist():
        width = max(width, 0)
        lo, hi = max(dst, 0), min(dst + width, n)
        if hi <= lo:
            continue
        ids = np.zeros(width, np.uint8)
        qvs = np.zeros(width, np.uint8)
        if 0 <= zi < len(zmw_tab):
            ccs_off = int(zmw_tab[zi, TAB_CCS_OFF])
            W = int(zmw_tab[zi, TAB_W])
            if ccs_off >= 0 and W >= 0 and ccs_off + W <= n_src:
                start = min(max(start, 0), W)
                w = min(max(w, 0), width, W - start)
                src = slice(ccs_off + start, ccs_off + start + w)
                ids[:w] = ccs[src]
                qvs[:w] = qual_lut[ccs_q[src]]
                qvs[w:] = qual_lut[0]
        bases_out[lo:hi] = ids[lo - dst : hi - dst]
        quals_out[lo:hi] = qvs[lo - dst : hi - dst]
