"""One buffer per packer: typed regions back to back in a ``uint8`` blob,
so one copy moves everything to the device. Shared by pack_batch,
pack_spacing and pack_expand, and by whoever uploads what they packed."""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np

Region = Tuple[str, type, int]  # (name, dtype, element count)


def check(label: str, cond: bool, message: str) -> None:
    if not cond:
        raise ValueError(f"{label}: {message}")


def empty_column(dtype):
    """Dataclass field of a table column that starts out empty."""
    return dataclasses.field(default_factory=lambda: np.empty(0, dtype))


def fallback_counter(stage: str, cause: str) -> str:
    """Counter of the ZMWs that left device stage ``stage`` for ``cause``."""
    return f"n_zmw_{stage}_fallback_{cause}"


def region_offsets(regions: Sequence[Region]) -> Tuple[Dict[str, int], int]:
    """Byte offset of every region, and the total. No padding: regions in
    descending item size are each aligned to their own type."""
    offsets, total = {}, 0
    for name, dtype, count in regions:
        offsets[name] = total
        total += count * np.dtype(dtype).itemsize
    return offsets, total


def pack_views(
    regions: Sequence[Region],
    alloc: Optional[Callable[[int], np.ndarray]] = None,
    label: str = "pack",
) -> Tuple[np.ndarray, Dict[str, int], Dict[str, np.ndarray]]:
    """(blob, byte offsets, typed flat views) for ``regions``.
    ``alloc(nbytes)`` returns the ``uint8`` buffer to pack into (pinned
    memory, say); numpy allocates otherwise."""
    offsets, total = region_offsets(regions)
    blob = np.empty(total, np.uint8) if alloc is None else alloc(total)
    check(label, isinstance(blob, np.ndarray) and blob.dtype == np.uint8
          and blob.shape == (total,) and blob.flags.c_contiguous,
          "alloc must return a contiguous uint8 array of nbytes")
    views = {}
    for name, dtype, count in regions:
        lo = offsets[name]
        views[name] = blob[lo : lo + count * np.dtype(dtype).itemsize].view(
            dtype)
    return blob, offsets, views


def typed_region(blob, lo: int, dtype, shape):
    """``shape`` elements of ``dtype`` at byte ``lo`` of a flat uint8 torch
    tensor, as a view."""
    import torch

    dtype = np.dtype(dtype)
    flat = blob[lo : lo + int(np.prod(shape)) * dtype.itemsize]
    return flat.view(getattr(torch, dtype.name)).view(tuple(shape))


def device_view(blob, packed, name: str, dtype=None):
    """Region ``name`` of ``packed`` (a batch with ``offsets`` and the host
    view as attribute ``name``) inside its uploaded ``blob``, with the host
    view's shape and dtype; ``dtype`` names a same-size type to reinterpret
    the elements as."""
    like = getattr(packed, name)
    return typed_region(blob, packed.offsets[name], dtype or like.dtype,
                        like.shape)
