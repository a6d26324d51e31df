"""Span scanner for serialized tf.train.Example training records.

The device input mode (models/data_device.py) moves the two tensor payloads
of a record as raw bytes and never needs the other features, so instead of
example_codec.decode_example (which materialises every value list,
`ccs_base_quality_scores` included) this walks the wire format once and
returns only where `subreads/encoded` and `label/encoded` lie inside the
buffer, plus the two shape lists. Every other feature is skipped by its
length. The order features were written in does not matter.
decode_example stays the oracle (tests/test_input_device.py).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

_LEN = 2  # wire type of a length-delimited field

SUBREADS = b"subreads/encoded"
SUBREADS_SHAPE = b"subreads/shape"
LABEL = b"label/encoded"
LABEL_SHAPE = b"label/shape"
_WANTED = (SUBREADS, SUBREADS_SHAPE, LABEL, LABEL_SHAPE)


class ExampleSpans(NamedTuple):
    """(offset, length) byte spans into the scanned buffer; label fields are
    None for a record without a label."""

    subreads: Tuple[int, int]
    subreads_shape: List[int]
    label: Optional[Tuple[int, int]]
    label_shape: Optional[List[int]]


def _fail(what: str, where) -> ValueError:
    if isinstance(where, bytes):
        where = where.decode(errors="replace")
    return ValueError(f"malformed tf.Example: {what} in feature {where!r}")


def _varint(buf, off: int, end: int, where) -> Tuple[int, int]:
    shift = 0
    result = 0
    while True:
        if off >= end or shift > 63:
            raise _fail("truncated varint", where)
        b = buf[off]
        off += 1
        result |= (b & 0x7F) << shift
        if not (b & 0x80):
            return result, off
        shift += 7


def _field(buf, off: int, end: int, where) -> Tuple[int, int, int, int]:
    """Reads one field header; returns (field number, wire type, start of
    the value, offset after the value). Checks the value lies inside end."""
    tag, off = _varint(buf, off, end, where)
    wt = tag & 7
    if wt == _LEN:
        ln, off = _varint(buf, off, end, where)
        nxt = off + ln
    elif wt == 0:
        _, nxt = _varint(buf, off, end, where)
    elif wt == 1:
        nxt = off + 8
    elif wt == 5:
        nxt = off + 4
    else:
        raise _fail(f"unsupported wire type {wt}", where)
    if nxt > end:
        raise _fail("truncated value", where)
    return tag >> 3, wt, off, nxt


def _bytes_span(buf, off: int, end: int, name) -> Tuple[int, int]:
    """First value of a Feature holding a BytesList."""
    while off < end:
        kind, wt, v0, v1 = _field(buf, off, end, name)
        if kind == 1 and wt == _LEN:
            p = v0
            while p < v1:
                fno, wt2, b0, b1 = _field(buf, p, v1, name)
                if fno == 1 and wt2 == _LEN:
                    return b0, b1 - b0
                p = b1
        off = v1
    raise _fail("no bytes value", name)


def _int64_list(buf, off: int, end: int, name) -> List[int]:
    """All values of a Feature holding an Int64List (packed or not)."""
    out: List[int] = []
    while off < end:
        kind, wt, v0, v1 = _field(buf, off, end, name)
        if kind == 3 and wt == _LEN:
            p = v0
            while p < v1:
                fno, wt2, b0, b1 = _field(buf, p, v1, name)
                if fno == 1 and wt2 == _LEN:
                    q = b0
                    while q < b1:
                        v, q = _varint(buf, q, b1, name)
                        out.append(v - (1 << 64) if v >= 1 << 63 else v)
                elif fno == 1 and wt2 == 0:
                    v, _ = _varint(buf, b0, b1, name)
                    out.append(v - (1 << 64) if v >= 1 << 63 else v)
                p = b1
        elif kind in (1, 2):
            raise _fail("expected an int64 list", name)
        off = v1
    return out


def scan_example(buf, start: int = 0, end: Optional[int] = None
                 ) -> ExampleSpans:
    """Locates the subreads / label payloads of the record buf[start:end].

    buf is anything indexable to ints (bytes, bytearray, memoryview); the
    returned spans are offsets into buf itself, so a whole un-gzipped file
    can be scanned in place. Raises ValueError naming the feature on a
    truncated or malformed record.
    """
    if end is None:
        end = len(buf)
    if not 0 <= start <= end <= len(buf):
        raise _fail("record bounds outside the buffer", "Example")
    found = {}
    off = start
    while off < end:
        fno, wt, f0, f1 = _field(buf, off, end, "Example.features")
        off = f1
        if fno != 1 or wt != _LEN:
            continue
        p = f0
        while p < f1:  # Features.feature map entries
            eno, ewt, e0, e1 = _field(buf, p, f1, "Features.feature")
            p = e1
            if eno != 1 or ewt != _LEN:
                continue
            name = None
            value = None
            q = e0
            while q < e1:
                kno, kwt, k0, k1 = _field(
                    buf, q, e1, name if name is not None else "map entry")
                q = k1
                if kwt != _LEN:
                    continue
                if kno == 1:
                    name = bytes(buf[k0:k1])
                elif kno == 2:
                    value = (k0, k1)
            if name in _WANTED:
                if value is None:
                    raise _fail("no value", name)
                if name == SUBREADS or name == LABEL:
                    found[name] = _bytes_span(buf, value[0], value[1], name)
                else:
                    found[name] = _int64_list(buf, value[0], value[1], name)
    for need in (SUBREADS, SUBREADS_SHAPE):
        if need not in found:
            raise _fail("missing", need)
    if (LABEL in found) != (LABEL_SHAPE in found):
        raise _fail("missing", LABEL_SHAPE if LABEL in found else LABEL)
    return ExampleSpans(found[SUBREADS], found[SUBREADS_SHAPE],
                        found.get(LABEL), found.get(LABEL_SHAPE))
