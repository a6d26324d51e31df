"""The model input of one ZMW batch, batch_size windows at a time, and the
loop that takes each chunk through the model.

``model_chunks`` picks the form the batch arrived in:

* ``RowChunks`` (featurize_mode "host"): the pre-stacked per-ZMW matrices
  are concatenated once and each chunk is staged through a pinned buffer.
* ``PlaneChunks`` (featurize_mode "device"): the batch's planes and tables
  cross to the device in one copy per packer and each chunk is expanded
  there by the window_featurize kernel; ZMWs that kept host rows have theirs
  copied into their slots. On a non-native runner the kernels' numpy twins
  do the same on the host.

Both offer ``n_model``, ``row_length``, ``all_pos``, ``model_zmws``,
``n_pt_bytes``, ``chunk(i)`` and ``forward()``.
"""
from __future__ import annotations

import os
from typing import Any, Dict, Iterator, List, Tuple

import numpy as np
import torch

from deepconsensus_amd.preprocess import blob as blob_lib
from deepconsensus_amd.preprocess import expand_device
from deepconsensus_amd.preprocess import featurize_device
from deepconsensus_amd.preprocess import spacing_device


class ModelChunks:
    """What the two forms share."""

    n_pt_bytes = 0  # size of the packed passthrough region

    def __init__(self, zmws: List[Any], runner, options):
        self.runner = runner
        self.batch_size = options.batch_size
        self.model_zmws = [
            z for z in zmws if featurize_device.n_model_windows(z)
        ]
        self.all_pos = (
            np.concatenate([z.window_pos for z in self.model_zmws])
            if self.model_zmws else np.empty(0, np.int64)
        )
        # Native path: features are non-negative and <= SN_MAX (500)
        # after clipping, and the embed kernel casts to int anyway, so
        # int16 staging halves H2D traffic with bit-identical results
        # (numpy's truncation toward zero == the kernel's (int)v == the
        # torch model's .long()).
        self.native = bool(getattr(runner, "native", False))
        self.use_graph = (
            self.native and os.environ.get("DC_SERVE_GRAPH", "1") != "0"
        )

    def chunk(self, i: int) -> Tuple[torch.Tensor, int]:
        """(rows_t, n_valid) for windows [i, i + batch_size): the model
        input (padded to batch_size when the graph is in use) and the
        number of real windows in it."""
        raise NotImplementedError

    def forward(self) -> Iterator[Tuple[int, torch.Tensor, torch.Tensor,
                                        torch.Tensor, int]]:
        """(i, rows_t, bases_t, quals_t, n_valid) per chunk: the model step
        on the chunk at window i, its outputs cut to the real windows. The
        next replay of the graph rewrites them: the consumer reads them, or
        queues its copies on the same stream, before it asks for more."""
        for i in range(0, self.n_model, self.batch_size):
            rows_t, n_valid = self.chunk(i)
            if self.use_graph:
                bases_t, quals_t = self.runner.forward_windows_graphed(rows_t)
                bases_t = bases_t[:n_valid]
                quals_t = quals_t[:n_valid]
            else:
                bases_t, quals_t = self.runner.forward_windows(rows_t)
            yield i, rows_t, bases_t, quals_t, n_valid


class RowChunks(ModelChunks):
    """Host rows, staged through one pinned buffer per shape."""

    def __init__(self, zmws: List[Any], runner, options):
        super().__init__(zmws, runner, options)
        self.row_length = options.max_length
        self.n_model = 0
        if self.model_zmws:
            all_rows = np.concatenate([z.rows for z in self.model_zmws])
            self.row_length = all_rows.shape[2]
            if not self.native:
                all_rows = all_rows.astype(np.float32)
            self.all_rows = all_rows
            self.n_model = len(all_rows)
            self.pinned: Dict[Tuple[int, ...], torch.Tensor] = {}

    def chunk(self, i: int) -> Tuple[torch.Tensor, int]:
        chunk = np.ascontiguousarray(self.all_rows[i : i + self.batch_size])
        n_valid = len(chunk)
        rows_t = torch.from_numpy(chunk)
        if self.native:
            # Fixed-shape pinned buffer: partial tails are zero-padded
            # so the hipGraph-captured step replays at one shape (pad
            # windows cost compute on the final chunk only; their
            # outputs are sliced away).
            shape = (
                (self.batch_size,) + rows_t.shape[1:]
                if self.use_graph
                else tuple(rows_t.shape)
            )
            buf = self.pinned.get(shape)
            if buf is None:
                buf = torch.zeros(shape, dtype=rows_t.dtype).pin_memory()
                self.pinned[shape] = buf
            buf[:n_valid].copy_(rows_t)
            if self.use_graph and n_valid < shape[0]:
                buf[n_valid:].zero_()
            rows_t = buf
        return rows_t, n_valid


class PlaneChunks(ModelChunks):
    """Planes and tables, expanded per chunk. ``packed_zmws`` are the ZMWs
    with something to pack: model windows, or (passthrough_mode "device")
    passthrough table entries. A batch of the latter alone still crosses to
    the device: its CCS planes are the source of the passthrough fill."""

    def __init__(self, zmws: List[Any], runner, options,
                 packed_zmws: List[Any]):
        super().__init__(zmws, runner, options)
        if not self.native:
            self.batch = featurize_device.pack_batch(packed_zmws)
            expand_device.expand_batch_numpy(self.batch)
            spacing_device.space_batch_numpy(self.batch)
        else:
            self._upload(packed_zmws)
        self.n_model = self.batch.n_windows
        self.row_length = self.batch.max_length

    @property
    def n_pt_bytes(self) -> int:
        return self.batch.n_pt_bytes

    def _upload(self, packed_zmws: List[Any]) -> None:
        device = self.runner.device
        staging: List[torch.Tensor] = []

        def alloc(nbytes: int) -> np.ndarray:
            staging.append(
                torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            )
            return staging[-1].numpy()

        # With the graph every chunk is batch_size table entries:
        # the tail is padded with -1 (zero) windows once, here.
        self.batch = batch = featurize_device.pack_batch(
            packed_zmws,
            pad_multiple=self.batch_size if self.use_graph else 1,
            alloc=alloc, device_planes=True,
        )
        blob = staging[0].to(device, non_blocking=True)
        if batch.device_planes:
            # Unspaced ZMWs: the plane region is born on the device,
            # zero-filled, in pack_batch's layout.
            planes = torch.zeros(batch.plane_nbytes, dtype=torch.uint8,
                                 device=device)
            sub, ccs, ccs_bq, ccs_q = (
                blob_lib.typed_region(planes, lo, dtype, (count,))
                for lo, dtype, count in (
                    batch.plane_layout[name]
                    for name in ("sub", "ccs", "ccs_bq", "ccs_q"))
            )
        else:
            sub, ccs, ccs_bq, ccs_q = (
                blob_lib.device_view(blob, batch, name)
                for name in ("sub", "ccs", "ccs_bq", "ccs_q")
            )
        zmw_tab = blob_lib.device_view(blob, batch, "zmw_tab")
        self.dev = (sub, ccs, ccs_bq, zmw_tab)
        self.win_tab = blob_lib.device_view(blob, batch, "win_tab")
        # Inputs of passthrough_fill_into, ahead of the LUT.
        self.pt_dev = (
            ccs, ccs_q, zmw_tab, blob_lib.device_view(blob, batch, "pt_tab"),
        )
        if batch.spacing is not None:
            self._space_on_device(staging[1:])
        if batch.fallback_rows is not None:
            self.fallback_rows = torch.from_numpy(
                batch.fallback_rows
            ).to(device)
            self.fallback_idx = torch.from_numpy(
                batch.fallback_idx
            ).to(device)

    def _space_on_device(self, staged: List[torch.Tensor]) -> None:
        """Fills the device planes of the unspaced ZMWs: one copy of the
        packed reads, then the subread_space kernel, on the stream of the
        kernels that read the planes. ZMWs spaced on the host have their
        planes copied into their slices. With raw ZMWs (expand_mode
        "device") ``src`` is allocated on the device, the host-written part
        copied in, and the cigar_expand kernel fills the rest from the
        expand blob ahead of subread_space."""
        batch, sp = self.batch, self.batch.spacing
        device = self.runner.device
        sp_blob = staged[0].to(device, non_blocking=True)
        src = blob_lib.device_view(sp_blob, sp, "src")
        if sp.expand is not None:
            ex = sp.expand
            ex_blob = staged[1].to(device, non_blocking=True)
            host_src = src
            src = torch.empty(sp.n_src, dtype=torch.uint8, device=device)
            src[: sp.n_src_host].copy_(host_src)
            self.runner.ext.cigar_expand_into(
                blob_lib.device_view(ex_blob, ex, "raw"),
                blob_lib.device_view(ex_blob, ex, "op_tab"),
                blob_lib.device_view(ex_blob, ex, "xr_tab"),
                src, torch.from_numpy(expand_device.NT16_LUT),
            )

        sub, ccs, ccs_bq, zmw_tab = self.dev
        ccs_q = self.pt_dev[1]
        targets = dict(sub=sub, ccs=ccs, ccs_bq=ccs_bq, ccs_q=ccs_q)
        for name, off, array in batch.host_planes:
            targets[name][off : off + array.size].copy_(
                torch.from_numpy(array))
        # The kernel takes the uint16 run lengths as an int16 tensor.
        ins_max = blob_lib.device_view(sp_blob, sp, "ins_max", np.int16)
        self.runner.ext.subread_space_into(
            src, ins_max,
            blob_lib.device_view(sp_blob, sp, "sp_tab"),
            blob_lib.device_view(sp_blob, sp, "read_tab"),
            zmw_tab, torch.empty(ins_max.numel(), dtype=torch.int32,
                                 device=device),
            sub, ccs, ccs_q, ccs_bq, batch.use_ccs_bq,
        )

    def chunk(self, i: int) -> Tuple[torch.Tensor, int]:
        batch = self.batch
        n_valid = min(self.batch_size, self.n_model - i)
        if not self.native:
            rows = featurize_device.featurize_chunk_numpy(
                batch, i, i + n_valid
            )
            return torch.from_numpy(rows.astype(np.float32)), n_valid
        hi = i + (self.batch_size if self.use_graph else n_valid)
        rows_t = self.runner.ext.window_featurize(
            *self.dev, self.win_tab[i:hi], batch.n_rows, batch.max_length,
            batch.max_passes, batch.use_ccs_bq,
        )
        k0, k1 = batch.fallback_range(i, i + n_valid)
        if k1 > k0:
            rows_t.index_copy_(
                0, self.fallback_idx[k0:k1] - i, self.fallback_rows[k0:k1]
            )
        return rows_t, n_valid

    def fill_passthrough(self, qual_lut, bases_out, quals_out) -> None:
        """Base ids and QVs of the table passthrough windows, from the CCS
        planes: one launch per ZMW batch on the stream of the model loop
        and of stitch_compact, which reads what it writes."""
        if self.native:
            self.runner.ext.passthrough_fill_into(
                *self.pt_dev, qual_lut, bases_out, quals_out)
        else:
            batch = self.batch
            featurize_device.passthrough_fill_numpy(
                batch.ccs, batch.ccs_q, batch.zmw_tab, batch.pt_tab,
                qual_lut, bases_out, quals_out)


def model_chunks(zmws: List[Any], runner, options) -> ModelChunks:
    """RowChunks, or PlaneChunks when a ZMW with something to pack carries
    planes."""
    packed_zmws = [
        z for z in zmws
        if featurize_device.n_model_windows(z)
        or featurize_device.n_table_passthrough(z)
    ]
    if any(getattr(z, "planes", None) is not None for z in packed_zmws):
        return PlaneChunks(zmws, runner, options, packed_zmws)
    return RowChunks(zmws, runner, options)
