"""GPU tests: fused_embed_condense (K2+K3+K4) against the two-kernel path.

The op must return the bits of
    fused_condense(embed_gather(rows, ...).reshape(B*L, K), w_img, pos, N, L)
from the same extension, so every comparison is torch.equal on the int16
view: no tolerance. Layouts come from models built from the project's
config (max_passes 20 / 32, without / with ccs_bq: K = 560, 568, 872, 880,
i.e. the 8-wave and 4-wave tiles and both half-granule widths).
"""
import numpy as np
import pytest
import torch

from deepconsensus_amd import ops as dc_ops
from deepconsensus_amd.models import config as cfg
from deepconsensus_amd.models.model import get_model
from deepconsensus_amd.models.runner import (
    InferenceRunner,
    build_condense_image,
    build_gather_tables,
)

pytestmark = pytest.mark.gpu

N_OUT = 280
LAYOUTS = [(20, False, 560), (20, True, 568), (32, False, 872),
           (32, True, 880)]
# single lane / partial 32-row group / M = 300: a row group crosses a
# window boundary and the 256 and 128 tile edges / M = 259: L a multiple of
# nothing, one row past a 256 tile.
SHAPES = [(1, 1), (1, 31), (3, 100), (7, 37)]


@pytest.fixture(scope="module")
def ext():
    return dc_ops.get_ext(required=True)


def _params(max_passes, use_ccs_bq):
    params = cfg.get_config("transformer_learn_values+custom")
    params.use_ccs_bq = use_ccs_bq
    params.max_passes = max_passes
    cfg.modify_params(params, is_training=False)
    return params


@pytest.fixture(scope="module")
def layouts():
    """Per layout: device gather tables + map, CPU shift / vocab, weight
    image. Built once, never modified."""
    made = {}
    for max_passes, bq, k in LAYOUTS:
        torch.manual_seed(100 + k)
        model = get_model(_params(max_passes, bq))
        tabs = build_gather_tables(model)
        assert tabs[3].numel() * 8 == k
        g = torch.Generator().manual_seed(k)
        w = torch.randn(N_OUT, k, generator=g) * 0.05
        made[k] = dict(
            tabs=tuple(t.cuda() for t in tabs),
            shift=tabs[1].numpy(), vocab=tabs[2].numpy(),
            img=build_condense_image(w).cuda(),
        )
    return made


def _ids(lay, b, l, seed):
    """int16 [b, R, l]: ids over each row's full vocabulary (after the
    row's shift), a few below 0 and above vocab - 1 per row, and -1 on the
    shifted (ccs_bq) row."""
    rng = np.random.default_rng(seed)
    shift, vocab = lay["shift"], lay["vocab"]
    nrow = len(vocab)
    ids = np.zeros((b, nrow, l), dtype=np.int64)
    for r in range(nrow):
        ids[:, r] = rng.integers(0, vocab[r], size=(b, l)) - shift[r]
        flat = ids[:, r].reshape(-1)
        n_bad = min(3, flat.size)
        where = rng.choice(flat.size, size=n_bad, replace=False)
        flat[where] = rng.choice(
            [-3 - shift[r], vocab[r] + 5, -200, vocab[r] - shift[r]],
            size=n_bad)
        if shift[r] == 1:
            flat[rng.integers(0, flat.size)] = -1
        ids[:, r] = flat.reshape(b, l)
    assert ids.min() >= -32768 and ids.max() <= 32767
    return torch.from_numpy(ids.astype(np.int16))


def _pos(l, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(l, N_OUT, generator=g) * 0.3).cuda()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _two_kernel(ext, lay, rows, pos):
    b, _, l = rows.shape
    emb = ext.embed_gather(rows, *lay["tabs"])
    return ext.fused_condense(emb.reshape(b * l, -1), lay["img"], pos,
                              N_OUT, l)


def _assert_same_bits(ext, lay, rows, pos):
    b, _, l = rows.shape
    want = _two_kernel(ext, lay, rows, pos)
    got = ext.fused_embed_condense(rows, *lay["tabs"], lay["img"], pos, N_OUT)
    assert got.shape == (b * l, N_OUT) and got.dtype == torch.bfloat16
    n_diff = int((_bits(got) != _bits(want)).sum())
    print(f"B={b} L={l} differing elements: {n_diff}")
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("b,l", SHAPES)
@pytest.mark.parametrize("k", [k for _, _, k in LAYOUTS])
def test_matches_two_kernel_path(ext, layouts, k, b, l):
    lay = layouts[k]
    rows = _ids(lay, b, l, seed=1000 * k + 10 * b + l).cuda()
    _assert_same_bits(ext, lay, rows, _pos(l, seed=k + l))
    empty = torch.empty(0, device="cuda", dtype=torch.float32)
    _assert_same_bits(ext, lay, rows, empty)


@pytest.mark.parametrize("k", [k for _, _, k in LAYOUTS])
def test_float_ids_match_int16(ext, layouts, k):
    lay = layouts[k]
    rows = _ids(lay, 3, 100, seed=77 * k).cuda()
    pos = _pos(100, seed=k)
    _assert_same_bits(ext, lay, rows, pos)
    _assert_same_bits(ext, lay, rows.float(), pos)
    a = ext.fused_embed_condense(rows, *lay["tabs"], lay["img"], pos, N_OUT)
    f = ext.fused_embed_condense(rows.float(), *lay["tabs"], lay["img"], pos,
                                 N_OUT)
    assert torch.equal(_bits(a), _bits(f))


@pytest.mark.parametrize("k", [k for _, _, k in LAYOUTS])
def test_rows_past_m_do_not_gather(ext, layouts, k):
    """rows is the leading slice of a larger buffer whose tail holds ids
    far outside every table (32767; the tables hold ~8 K elements).
    B * L = 111 is no multiple of 32, so the last row group and the rest
    of the tile are lanes of rows >= M: they must hold zero fragments and
    issue no loads, and the output must equal the reference."""
    lay = layouts[k]
    b, l = 3, 37
    ids = _ids(lay, b, l, seed=5 * k)
    nrow = ids.shape[1]
    buf = torch.full(((b + 8) * nrow * l,), 32767, dtype=torch.int16,
                     device="cuda")
    rows = buf[: b * nrow * l].view(b, nrow, l)
    rows.copy_(ids)
    assert bool((buf[b * nrow * l:] == 32767).all())
    _assert_same_bits(ext, lay, rows, _pos(l, seed=k))


def test_op_checks_its_map(ext, layouts):
    lay = layouts[560]
    rows = _ids(lay, 1, 8, seed=3).cuda()
    tf, rs, rv, cc, ce = lay["tabs"]
    empty = torch.empty(0, device="cuda", dtype=torch.float32)
    with pytest.raises(RuntimeError):  # one row too few in shift / vocab
        ext.fused_embed_condense(rows, tf, rs[:-1], rv[:-1], cc, ce,
                                 lay["img"], empty, N_OUT)
    with pytest.raises(RuntimeError):  # 69 chunks: K = 552
        ext.fused_embed_condense(rows, tf, rs, rv, cc[:-1], ce[:-16],
                                 lay["img"], empty, N_OUT)
    with pytest.raises(RuntimeError):  # entries do not match the chunks
        ext.fused_embed_condense(rows, tf, rs, rv, cc, ce[:-16],
                                 lay["img"], empty, N_OUT)
    with pytest.raises(RuntimeError):  # the 568 image under a 560 map
        ext.fused_embed_condense(rows, tf, rs, rv, cc, ce,
                                 layouts[568]["img"], empty, N_OUT)
    with pytest.raises(RuntimeError):  # R > 160
        ext.fused_embed_condense(
            torch.zeros(1, 161, 8, dtype=torch.int16, device="cuda"), tf,
            rs, rv, cc, ce, lay["img"], empty, N_OUT)


def test_runner_switch_gives_equal_bits(monkeypatch):
    """encode_native with the fused op (default) and with DC_FUSED_EMBED=0
    (embed_gather + fused_condense), each in a fresh runner, at B = 3."""
    params = _params(20, False)
    torch.manual_seed(23)
    model = get_model(params)
    rng = np.random.default_rng(9)
    R, L, mp = params.total_rows, params.max_length, params.max_passes
    rows = np.zeros((3, R, L), dtype=np.int16)
    rows[:, 0:mp] = rng.integers(0, 5, size=(3, mp, L))
    rows[:, mp:3 * mp] = rng.integers(0, 256, size=(3, 2 * mp, L))
    rows[:, 3 * mp:4 * mp] = rng.integers(0, 3, size=(3, mp, L))
    rows[:, 4 * mp] = rng.integers(0, 5, size=(3, L))
    rows[:, -4:] = rng.integers(0, 501, size=(3, 4, 1))
    rows = torch.from_numpy(rows).cuda()

    monkeypatch.delenv("DC_FUSED_CONDENSE", raising=False)
    monkeypatch.delenv("DC_FUSED_EMBED", raising=False)
    fused = InferenceRunner(params, model, device="cuda:0")
    monkeypatch.setenv("DC_FUSED_EMBED", "0")
    split = InferenceRunner(params, model, device="cuda:0")
    assert fused.native and split.native
    assert fused.cond_img is not None and split.cond_img is not None
    assert fused.fused_embed and not split.fused_embed
    a = fused.encode_native(rows)
    b = split.encode_native(rows)
    assert a.shape == (3, L, N_OUT)
    assert torch.equal(_bits(a), _bits(b))
