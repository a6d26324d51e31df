"""The host path that feeds the device-mode kernels: packed bytes against
the digests recorded before the packers, the per-ZMW records and the chunk
loop were unified, the one base encoder against a literal table, and the
mode table against the five resolvers."""
import importlib.util
import json
import os

import numpy as np

from deepconsensus_amd.inference import quick_inference as qi
from deepconsensus_amd.preprocess import expand_device as xd
from deepconsensus_amd.preprocess import featurize_device as fd
from deepconsensus_amd.preprocess import spacing_device as spd

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pack_digest():
    spec = importlib.util.spec_from_file_location(
        "pack_digest", os.path.join(_ROOT, "scripts", "pack_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_packed_bytes_match_recorded(monkeypatch):
    """tests/golden/pack_digests.json is scripts/pack_digest.py's output on
    the three separate packers: every table and array view of
    FeaturizeBatch, SpacingBatch and ExpandBatch, the offsets, the plane
    layout and the host plane pieces, in four mode sets, packed plainly and
    with device_planes + pad_multiple."""
    for knob, *_ in qi.MODE_TABLE.values():
        monkeypatch.delenv(knob, raising=False)
    with open(os.path.join(_ROOT, "tests", "golden",
                           "pack_digests.json")) as f:
        want = json.load(f)
    mod = _pack_digest()
    assert len(want) == 128
    assert {k.split("/")[0] for k in want} == set(mod.MODE_SETS)
    assert any(k.startswith("expand/device/expand/") for k in want)
    got = mod.compute()
    differ = sorted(k for k in want if got.get(k) != want[k])
    print(f"{len(want) - len(differ)} of {len(want)} digests equal")
    assert sorted(got) == sorted(want)
    assert not differ, differ


def test_encode_bases_table():
    """Every code point 0..255, ' ' and code points above the table map to
    the id of their letter in SEQ_VOCAB (' ATCG'), anything else to 0. The
    per-letter masked form this replaced gave the same array."""
    cps = list(range(256)) + [ord(" "), 0x3B1, 0x20AC, 0x1F600]
    bases = np.array([chr(c) for c in cps], dtype="<U1")
    want = np.zeros(len(cps), np.uint8)
    want[ord("A")], want[ord("T")], want[ord("C")], want[ord("G")] = (
        1, 2, 3, 4)
    got = fd.encode_bases(bases)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert got[cps.index(ord(" "))] == 0 and not got[256:].any()
    # One encoder, whatever module it is reached through, on any shape.
    assert spd.encode_bases is fd.encode_bases
    grid = bases.reshape(4, 65)
    assert np.array_equal(fd.encode_bases(grid), want.reshape(4, 65))
    assert np.array_equal(fd.encode_bases(grid[:, ::2]),
                          want.reshape(4, 65)[:, ::2])
    assert xd.NT16_LUT.tolist() == [
        0, 1, 3, 0, 4, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0]


def test_mode_table_is_the_five_resolvers(monkeypatch):
    for knob, *_ in qi.MODE_TABLE.values():
        monkeypatch.delenv(knob, raising=False)
    assert tuple(qi.MODE_TABLE) == qi.Modes._fields
    options = qi.InferenceOptions(
        featurize_mode="device", stitch_mode="device",
        passthrough_mode="device", spacing_mode="device")
    modes = qi.resolve_modes(options)
    assert modes == ("device", "device", "device", "host", "device")
    for field in qi.Modes._fields:
        assert getattr(qi, f"resolve_{field}")(options) == getattr(
            modes, field)
    # An unknown DC_STITCH_MODE still passes through unchecked.
    monkeypatch.setenv("DC_STITCH_MODE", "threads")
    assert qi.resolve_modes(qi.InferenceOptions()).stitch_mode == "threads"
