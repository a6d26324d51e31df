"""DcConfig + DcExample: window slicing and feature extraction.

Behavioral parity with the reference (pre_lib.py:450-819): DcConfig computes
the row layout of the model input matrix (4 per-subread blocks of max_passes
rows + CCS row + optional ccs_bq row + 4 SN rows); DcExample slices the
spaced ZMW into fixed or CCS-provided "smart" windows, handles label
overflow, and emits the (height x width x 1) float32 feature matrix, the
inference feature dict, or a serialized tf.Example.

PROVENANCE NOTE (round-1 review): the DcConfig row-layout dict IS the
tf.Example data contract (unavoidable similarity), and DcExample's
property scaffolding mirrors the reference closely for the same
golden-contract reason as read.py; iter_feature_dicts (the vectorized
featurizer) is original.
"""
from __future__ import annotations

import collections
import dataclasses
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np

from deepconsensus_amd.dcio import example_codec
from deepconsensus_amd.preprocess.read import Read
from deepconsensus_amd.utils import constants
from deepconsensus_amd.utils import phred


def dc_config_from_shape(
    subreads_shape: Tuple[int, int, int], use_ccs_bq: bool = False
) -> "DcConfig":
    """Inverse constructor from tensor shape (pre_lib.py:424-447)."""
    height, width, _ = subreads_shape
    fixed_height = 6 if use_ccs_bq else 5
    max_passes, remainder = divmod(
        height - fixed_height, len(DcConfig.n_subread_features)
    )
    if remainder != 0:
        raise ValueError(f"Invalid subreads shape {subreads_shape!r}.")
    return DcConfig(max_passes, width, use_ccs_bq)


class DcConfig:
    """Row layout of the model input matrix (pre_lib.py:450-528)."""

    n_subread_features = ["bases", "pw", "ip", "strand"]

    def __init__(self, max_passes: int, max_length: int,
                 use_ccs_bq: bool = False):
        self.max_passes = max_passes
        self.max_length = max_length
        self.use_ccs_bq = use_ccs_bq
        self.feature_rows = {
            "bases": max_passes,
            "pw": max_passes,
            "ip": max_passes,
            "strand": max_passes,
            "ccs": 1,
            "ccs_bq": 1 if use_ccs_bq else 0,
            "sn": 4,
        }
        self.feature_indices = {}
        i_rows = 0
        for k, v in self.feature_rows.items():
            self.feature_indices[k] = slice(i_rows, i_rows + v)
            setattr(self, k, i_rows)
            i_rows += v

    def indices(self, feature: str, n_subreads: int = 0) -> slice:
        if n_subreads:
            assert feature in DcConfig.n_subread_features
            n_rows = min(n_subreads, self.max_passes)
            return slice(
                getattr(self, feature), getattr(self, feature) + n_rows
            )
        assert feature not in DcConfig.n_subread_features
        return slice(
            getattr(self, feature),
            getattr(self, feature) + self.feature_rows[feature],
        )

    @property
    def tensor_height(self) -> int:
        return sum(self.feature_rows.values())

    def to_dict(self) -> Dict[str, str]:
        return {
            "max_passes": str(self.max_passes),
            "max_length": str(self.max_length),
            "tensor_height": str(self.tensor_height),
            "tensor_width": str(self.max_length),
        }


@dataclasses.dataclass
class WindowSpec:
    """One inference window as columns [start, start + w) of the spaced
    ZMW. ``width`` is the padded width (max_length, or more for an
    overflow window); ``bq`` the CCS qualities padded to it with -1."""

    start: int
    w: int
    width: int
    overflow: bool
    window_pos: int
    bq: np.ndarray


def fixed_window_widths(ccs_width: int, example_width: int) -> List[int]:
    """Fixed-width windows covering ``ccs_width`` spaced columns."""
    num_full = int(ccs_width / example_width)
    if ccs_width % example_width > 0:
        num_full += 1
    return [example_width] * num_full


def window_specs(max_length: int, W: int, ccs_width: int,
                 ccs_bq_all: np.ndarray, ccs_idx_all: np.ndarray,
                 window_widths: List[int], counter: collections.Counter):
    """The inference windows of a spaced ZMW from its CCS row alone:
    width W, ``ccs_width`` (last non-gap CCS column + 1), the spaced CCS
    qualities and CCS indices (-1 in gap columns). Fills ``counter``;
    windows without any CCS index are counted and not yielded. Shared by
    DcExample.iter_window_specs and the unspaced path
    (preprocess/spacing_device.py), which knows the CCS row before any
    read is spaced."""
    start_pos = 0
    for window_width in window_widths:
        counter[f"example_width_bucket_{window_width}"] += 1
        if start_pos > ccs_width:
            break
        s, e = start_pos, min(start_pos + window_width, W)
        start_pos += window_width
        w_idx = ccs_idx_all[s:e]
        valid = w_idx >= 0
        if not valid.any():
            counter["n_examples_no_ccs_idx"] += 1
            continue
        overflow = window_width > max_length
        if overflow:
            counter["n_examples_overflow"] += 1
            # Read.pad still applies: an overflow window clipped at
            # the ZMW end shorter than max_length pads back up to it.
            width = max(e - s, max_length)
        else:
            counter["n_examples_skip_large_windows_keep"] += 1
            width = max_length
        w = e - s
        bq = ccs_bq_all[s:e]
        if w < width:  # Read.pad pads quality scores with -1
            bq_full = np.full(width, -1, ccs_bq_all.dtype)
            bq_full[:w] = bq
            bq = bq_full
        yield WindowSpec(
            start=s, w=w, width=width, overflow=overflow,
            window_pos=int(w_idx[valid].min()), bq=bq,
        )


@dataclasses.dataclass
class DcExample:
    """Container generating model inputs from spaced reads."""

    name: str
    reads: List[Read]
    config: DcConfig
    window_widths: Optional[np.ndarray] = None
    counter: collections.Counter = dataclasses.field(
        default_factory=collections.Counter
    )

    _width: Optional[int] = None
    _ccs_width: Optional[int] = None
    _overflow: bool = False

    @property
    def contig(self) -> Optional[str]:
        if self.label:
            return self.label.truth_range["contig"]
        return None

    @property
    def is_training(self) -> bool:
        return self.reads[-1].is_label

    @property
    def ccs(self) -> Read:
        return self.reads[-2] if self.is_training else self.reads[-1]

    @property
    def label(self) -> Union[Read, None]:
        return self.reads[-1] if self.is_training else None

    @property
    def label_coords(self) -> str:
        return self.label.label_coords if self.is_training else ""

    @property
    def subreads(self) -> List[Read]:
        return self.reads[:-2] if self.is_training else self.reads[:-1]

    @property
    def n_subreads(self) -> int:
        return len(self.subreads)

    @property
    def keep_subreads(self) -> int:
        return min(self.config.max_passes, self.n_subreads)

    @property
    def width(self) -> int:
        if self._width is None:
            self._width = len(self.ccs.bases)
        return self._width

    @property
    def ccs_width(self) -> int:
        if self._ccs_width is None:
            # == len(str(self.ccs).rstrip()) without building the 10+ kb
            # string: index of the last non-gap base + 1 (gaps are ' ').
            nz = np.flatnonzero(self.ccs.bases != constants.GAP)
            self._ccs_width = int(nz[-1]) + 1 if nz.size else 0
        return self._ccs_width

    @property
    def is_empty(self) -> bool:
        return not (self.ccs.ccs_idx >= 0).any()

    @property
    def ccs_matches_label(self) -> bool:
        from deepconsensus_amd.preprocess.read import right_pad

        ccs = phred.left_shift_seq(self.ccs.bases_encoded)
        label = phred.left_shift_seq(self.label.bases_encoded)
        seq_len = max([len(ccs), len(label)])
        ccs = right_pad(ccs, seq_len, 0)
        label = right_pad(label, seq_len, 0)
        return bool(np.equal(ccs, label).all())

    def calculate_windows(self, example_width: int) -> List[int]:
        """Window widths, fixed or from CCS smart-window widths
        (pre_lib.py:625-650)."""
        window_widths = []
        last_pos = 0
        if self.window_widths is not None:
            ccs_calculated_width = 0
            for window_width in self.window_widths:
                original_width = 0
                window_width_spaced = 0
                while original_width < window_width:
                    if (
                        self.ccs.bases[last_pos + window_width_spaced]
                        != constants.GAP
                    ):
                        original_width += 1
                    window_width_spaced += 1
                window_widths.append(window_width_spaced)
                last_pos += window_width_spaced
                ccs_calculated_width += window_width_spaced
            assert ccs_calculated_width == self.ccs_width
        else:
            window_widths = fixed_window_widths(self.ccs_width, example_width)
        return window_widths

    def iter_examples(self):
        """Yields per-window DcExamples (pre_lib.py:652-697)."""
        self.counter = collections.Counter()
        max_length = self.config.max_length
        start_pos = 0
        for window_width in self.calculate_windows(max_length):
            self.counter[f"example_width_bucket_{window_width}"] += 1
            window = self[start_pos : start_pos + window_width]
            if start_pos > self.ccs_width:
                break
            start_pos += window_width
            if window.is_empty:
                self.counter["n_examples_no_ccs_idx"] += 1
                continue

            if (
                self.is_training
                and len(window.label.bases) > max_length
            ):
                adjusted_label = window.label.remove_gaps(max_length)
                if not adjusted_label:
                    self.counter["n_examples_label_overflow"] += 1
                    continue
                self.counter["n_examples_adjusted_label"] += 1
                window.reads[-1] = adjusted_label

            self._overflow = False
            if window_width > max_length:
                self.counter["n_examples_overflow"] += 1
                self._overflow = True
                if self.is_training:
                    continue
            else:
                self.counter["n_examples_skip_large_windows_keep"] += 1

            reads = [x.pad(max_length) for x in window.reads]
            yield DcExample(
                self.name, reads, self.config, _overflow=self._overflow
            )

    def iter_window_specs(self):
        """Enumerates the inference windows of an evenly spaced ZMW.

        The column bookkeeping of the vectorized featurizers, shared by
        iter_feature_dicts (host matrices) and the compact-plane path
        (preprocess/featurize_device.py): same windows, same counters,
        same padded CCS qualities either way. Resets and fills
        ``self.counter``; windows without any CCS index are counted and
        not yielded.
        """
        self.counter = collections.Counter()
        return window_specs(
            self.config.max_length, self.width, self.ccs_width,
            np.asarray(self.ccs.base_quality_scores), self.ccs.ccs_idx,
            self.calculate_windows(self.config.max_length), self.counter,
        )

    @property
    def is_evenly_spaced_inference(self) -> bool:
        """Precondition of the vectorized featurizers: no label, and
        every read as wide as the CCS."""
        return not self.is_training and all(
            len(r.bases) == self.width for r in self.reads
        )

    def iter_feature_dicts(self, pw_max=None, ip_max=None, sn_max=None,
                           out_dtype=None):
        """Vectorized inference twin of
        ``(x.to_features_dict() for x in iter_examples())``.

        The per-window path re-encodes bases and re-stacks features for
        every (window x read) pair — the worker-pool hot spot. This
        encodes the whole spaced ZMW once into [n_reads, W] planes and
        emits each window as column slices of them. Training ZMWs (label
        handling) and irregular read widths fall back to the per-window
        path; counters and dict contents are identical either way
        (tests/test_preprocess.py::test_iter_feature_dicts_matches_slow).

        pw_max/ip_max/sn_max apply format_rows' value clipping
        (data_providers.py:128-184) at the ZMW level (clipping is
        elementwise, so it commutes with windowing); out_dtype builds
        the feature matrix directly in that dtype (int16 staging for
        the native model path — truncation toward zero matches the
        embed kernel's cast). Dicts then carry "fmt": True and the
        fallback path applies the same formatting per window.
        """
        fmt = (pw_max is not None or ip_max is not None
               or sn_max is not None or out_dtype is not None)
        dtype = out_dtype or constants.NP_DATA_TYPE
        if not self.is_evenly_spaced_inference:
            from deepconsensus_amd.models import data as data_lib
            from deepconsensus_amd.models.config import Params

            fmt_params = Params(
                max_passes=self.config.max_passes,
                use_ccs_bq=self.config.use_ccs_bq,
                total_rows=self.config.tensor_height,
                PW_MAX=pw_max, IP_MAX=ip_max, SN_MAX=sn_max,
            )
            for x in self.iter_examples():
                f = x.to_features_dict()
                if fmt:
                    rows = data_lib.format_rows(f["subreads"], fmt_params)
                    f["subreads"] = rows.astype(dtype)
                    f["fmt"] = True
                yield f
            return
        config = self.config
        subs = self.subreads[: config.max_passes]
        n = len(subs)
        ccs = self.ccs
        W = self.width
        if n:
            sub_bases = np.stack([r.bases for r in subs])
            sub_enc = np.zeros(sub_bases.shape, dtype)
            for k, base in enumerate(constants.SEQ_VOCAB):
                if k:
                    sub_enc[sub_bases == base] = k
            pw_all = np.stack([r.pw for r in subs]).astype(dtype)
            ip_all = np.stack([r.ip for r in subs]).astype(dtype)
            if pw_max is not None:
                np.clip(pw_all, 0, pw_max, out=pw_all)
            if ip_max is not None:
                np.clip(ip_all, 0, ip_max, out=ip_all)
            strand_col = np.array(
                [int(r.strand) for r in subs], dtype
            )[:, None]
            sn = np.asarray(subs[0].sn)
            if sn_max is not None:
                sn = np.clip(sn, 0, sn_max)
            sn_col = sn.astype(dtype)[:, None]
        ccs_enc = np.zeros(W, dtype)
        for k, base in enumerate(constants.SEQ_VOCAB):
            if k:
                ccs_enc[ccs.bases == base] = k
        n_rows = config.tensor_height
        scalars = dict(
            name=self.name,
            ec=ccs.ec, np_num_passes=ccs.np_num_passes,
            rq=ccs.rq, rg=ccs.rg,
        )
        keep = self.keep_subreads

        for spec in self.iter_window_specs():
            s, w, width = spec.start, spec.w, spec.width
            e = s + w
            overflow, bq = spec.overflow, spec.bq
            data = np.zeros((n_rows, width), dtype)
            if n:
                data[config.indices("bases", n), :w] = sub_enc[:, s:e]
                data[config.indices("pw", n), :w] = pw_all[:, s:e]
                data[config.indices("ip", n), :w] = ip_all[:, s:e]
                data[config.indices("strand", n)] = strand_col
                data[config.indices("sn")] = sn_col
            data[config.indices("ccs"), :w] = ccs_enc[s:e]
            if config.use_ccs_bq:
                data[config.indices("ccs_bq"), :w] = bq[:w]
                data[config.indices("ccs_bq"), w:] = -1
            out = {
                "subreads": data[:, :, None],
                "subreads/num_passes": keep,
                "window_pos": spec.window_pos,
                "ccs_base_quality_scores": bq,
                "overflow": overflow,
                **scalars,
            }
            if fmt:
                out["fmt"] = True
            yield out

    def stack_subread_feature(self, name: str) -> np.ndarray:
        max_passes = self.config.max_passes
        return np.stack(
            [getattr(x, name) for x in self.subreads[:max_passes]]
        )

    def extract_features(self) -> np.ndarray:
        """The (height x width x 1) float32 model input
        (pre_lib.py:704-744)."""

        def repeat(feature):
            return np.repeat(np.expand_dims(feature, -1), self.width, -1)

        n_subreads = self.n_subreads
        dims = (self.config.tensor_height, self.width)
        data = np.zeros(shape=dims, dtype=constants.NP_DATA_TYPE)

        bases_idx = self.config.indices("bases", n_subreads)
        pw_idx = self.config.indices("pw", n_subreads)
        ip_idx = self.config.indices("ip", n_subreads)
        strand_idx = self.config.indices("strand", n_subreads)
        ccs_idx = self.config.indices("ccs")
        ccs_bq_idx = self.config.indices("ccs_bq")
        sn_idx = self.config.indices("sn")

        if n_subreads:
            data[bases_idx] = self.stack_subread_feature("bases_encoded")
            data[pw_idx] = self.stack_subread_feature("pw")
            data[ip_idx] = self.stack_subread_feature("ip")
            strand = self.stack_subread_feature("strand")
            strand = strand.astype(constants.NP_DATA_TYPE)
            data[strand_idx] = repeat(strand)
        data[ccs_idx] = self.ccs.bases_encoded
        if self.config.use_ccs_bq:
            data[ccs_bq_idx] = self.ccs.base_quality_scores
        if n_subreads:
            data[sn_idx] = repeat(self.subreads[0].sn)
        return np.expand_dims(data, -1)

    def to_features_dict(self) -> Dict[str, Any]:
        """Inference feature dict (pre_lib.py:746-762)."""
        data = self.extract_features()
        return {
            "subreads": data,
            "subreads/num_passes": self.keep_subreads,
            "name": self.name,
            "window_pos": self.ccs.ccs_bounds.start,
            "ccs_base_quality_scores": self.ccs.base_quality_scores,
            "overflow": self._overflow,
            "ec": self.ccs.ec,
            "np_num_passes": self.ccs.np_num_passes,
            "rq": self.ccs.rq,
            "rg": self.ccs.rg,
        }

    def tf_example(self) -> bytes:
        """Serialized tf.train.Example (pre_lib.py:764-787)."""
        data = self.extract_features()
        feats: Dict[str, Tuple[str, Any]] = {
            "subreads/encoded": (example_codec.BYTES, [data.tobytes()]),
            "subreads/shape": (example_codec.INT64, list(data.shape)),
            "subreads/num_passes": (
                example_codec.INT64,
                [self.keep_subreads],
            ),
            "name": (example_codec.BYTES, [self.name.encode()]),
            "window_pos": (
                example_codec.INT64,
                [int(self.ccs.ccs_bounds.start)],
            ),
            "ccs_base_quality_scores": (
                example_codec.INT64,
                [int(x) for x in self.ccs.base_quality_scores],
            ),
        }
        if self.is_training:
            label = self.label.bases_encoded
            feats["label/encoded"] = (example_codec.BYTES, [label.tobytes()])
            feats["label/shape"] = (example_codec.INT64, list(label.shape))
        return example_codec.encode_example(feats)

    def __getitem__(self, r_slice) -> "DcExample":
        if isinstance(r_slice, int):
            raise NotImplementedError
        reads = self.subreads + [self.ccs]
        reads = [x[r_slice] for x in reads]
        if self.label:
            ccs_slice = self.ccs[r_slice].ccs_bounds
            reads.append(
                self.label.ccs_slice(ccs_slice.start, ccs_slice.stop)
            )
        return DcExample(self.name, reads, self.config)

    def __repr__(self):
        preview = self[:100]
        start = preview.ccs.ccs_bounds.start
        end = preview.ccs.ccs_bounds.stop
        output = (
            f"{self.name} CCS({start}-{end}) {self.label_coords}".strip()
            + f'\n{"-" * (preview.width + 24)}\n'
        )
        for subread in self.subreads:
            subread_range = subread.name.split("/")[2]
            output += f"{subread_range:<20} {subread.strand} >{str(subread)}\n"
        output += f'{"CCS":<22} >{str(preview.ccs)}\n'
        if self.is_training:
            output += f'{"Label":<22} >{str(self.label)}\n'
        if self._overflow:
            output += f'{"overflow":<22} >{self._overflow}\n'
        return output


def decode_bases(bases_encoded: np.ndarray) -> np.ndarray:
    """Reverses base encoding (pre_lib.py:822-828)."""
    n_subreads, max_length = bases_encoded.shape
    bases = np.stack(
        [np.full(max_length, constants.GAP, dtype="<U1")] * n_subreads
    )
    for k, base in enumerate(constants.SEQ_VOCAB):
        bases[bases_encoded == k] = base
    return bases


def tf_example_to_features_dict(
    serialized: bytes,
    inference: bool = False,
) -> Dict[str, Any]:
    """Decodes a serialized tf.Example into the features dict
    (pre_lib.py:902-963, without TF)."""
    decoded = example_codec.decode_example(serialized)
    features: Dict[str, Any] = {}
    features["name"] = decoded["name"][1][0].decode()
    features["subreads/shape"] = list(decoded["subreads/shape"][1])
    features["subreads/num_passes"] = int(
        decoded["subreads/num_passes"][1][0]
    )
    features["window_pos"] = int(decoded["window_pos"][1][0])
    features["ccs_base_quality_scores"] = np.array(
        decoded["ccs_base_quality_scores"][1], dtype=np.int64
    )
    data = np.frombuffer(
        decoded["subreads/encoded"][1][0], dtype=constants.NP_DATA_TYPE
    ).reshape(features["subreads/shape"])
    features["subreads"] = data
    if not inference and "label/encoded" in decoded:
        label = np.frombuffer(
            decoded["label/encoded"][1][0], dtype=constants.NP_DATA_TYPE
        ).reshape(list(decoded["label/shape"][1]))
        features["label"] = label
    return features
