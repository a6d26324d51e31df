"""GPU tests of the distillation kernels (ops/hip/distill_loss.hip), the
native teacher forward and a distill run with both device modes on.

Outputs land in the leading rows of NaN-filled buffers and inputs are
followed by NaN rows: the guards must stay NaN and every output finite, so
a read or write past row M shows.
"""
import copy
import glob
import math
import os

import numpy as np
import pytest
import torch

from deepconsensus_amd import ops as dc_ops
from deepconsensus_amd.models import config as cfg
from deepconsensus_amd.models import losses as losses_lib
from deepconsensus_amd.models.model import get_model
from deepconsensus_amd.models.runner import InferenceRunner

import distill_probes as dp
import kernel_probes as kp

pytestmark = pytest.mark.gpu

TEMPS_EXACT = (1.0, 2.0, 0.5)
# Allowance over the fp32 torch-autograd error against the float64 twin.
YARDSTICK_FACTOR = 4.0


@pytest.fixture(scope="module")
def ext():
    return dc_ops.get_ext(required=True)


def _with_nan_tail(a) -> torch.Tensor:
    """a on the device as the leading rows of a buffer whose next
    GUARD_ROWS rows hold NaN."""
    t = torch.as_tensor(np.asarray(a)) if not torch.is_tensor(a) else a
    t = t.cuda()
    tail = torch.full((dp.GUARD_ROWS,) + tuple(t.shape[1:]), float("nan"),
                      dtype=t.dtype, device="cuda")
    return torch.cat([t, tail])[: t.shape[0]]


def _guarded_out(m: int):
    buf = torch.full((m + dp.GUARD_ROWS, 5), float("nan"), device="cuda")
    return buf, buf[:m]


def _assert_guard(buf, m, what):
    assert torch.isnan(buf[m:]).all(), f"{what}: guard rows written"
    assert torch.isfinite(buf[:m]).all(), f"{what}: non-finite output"


def _loss_call(ext, teacher, student, temperature, kind):
    """(loss float32 numpy scalar, grad float32 numpy [M, 5])."""
    m = len(teacher)
    buf, out = _guarded_out(m)
    loss, grad = ext.distill_loss_fwd(
        _with_nan_tail(teacher), _with_nan_tail(student), temperature,
        dp.KIND_ID[kind], out)
    assert grad.data_ptr() == out.data_ptr()
    _assert_guard(buf, m, f"distill_loss_fwd M={m} {kind} T={temperature}")
    assert loss.shape == () and loss.dtype == torch.float32
    assert math.isfinite(float(loss))
    return loss.cpu().numpy(), grad.cpu().numpy()


def _ulps(got32, want64):
    """|got - want| in units of float32 spacing at want."""
    want64 = np.asarray(want64, dtype=np.float64)
    spacing = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got32, dtype=np.float64) - want64) / spacing


# ===========================================================================
# 1. distill_loss_fwd, exact cases
# ===========================================================================

@pytest.mark.parametrize("kind", dp.KINDS)
@pytest.mark.parametrize("M", dp.MS)
def test_loss_equal_logits_is_exactly_zero(ext, M, kind):
    """Teacher == student: loss and gradient are exactly 0. Rows of five
    equal logits, random rows in [-4, 4] (at T = 0.5 the widest gap is 16
    and exp(-16) stays above the 1e-12 clamp: a clamped class keeps the
    gradient s_j A even when teacher and student agree), and
    (0, -200 x 4) rows, on which the masked terms cancel once
    exp(-200 / T) has underflowed to 0 (T = 1 and 0.5; at T = 2 exp(-100)
    is still a float32 denormal and the true gradient is not 0)."""
    rng = np.random.default_rng(M)
    peaked = np.array([0, -200, -200, -200, -200], dtype=np.float32)
    cases = {
        "uniform": (np.repeat(rng.uniform(-8, 8, (M, 1)), 5, 1), TEMPS_EXACT),
        "random": (rng.uniform(-4, 4, (M, 5)), TEMPS_EXACT),
        "peaked": (np.tile(peaked, (M, 1)), (1.0, 0.5)),
    }
    for name, (logits, temps) in cases.items():
        logits = logits.astype(np.float32)
        for temperature in temps:
            loss, grad = _loss_call(ext, logits, logits.copy(), temperature,
                                    kind)
            tag = f"{name} T={temperature}"
            assert loss == 0.0, (tag, loss)
            assert not grad.any(), (tag, np.abs(grad).max())


@pytest.mark.parametrize("temperature", TEMPS_EXACT)
@pytest.mark.parametrize("M", dp.MS)
def test_kl_peaked_teacher_uniform_student(ext, M, temperature):
    """Teacher (0, -200 x 4), uniform student: KL = log 5 within 2 ulp of
    float32, gradient rows (0.2 - 1, 0.2 x 4) / (T M) within 1 ulp."""
    teacher = np.tile(np.array([0, -200, -200, -200, -200], np.float32),
                      (M, 1))
    student = np.full((M, 5), 1.5, dtype=np.float32)
    loss, grad = _loss_call(ext, teacher, student, temperature,
                            "kl_divergence")
    u = _ulps(loss, math.log(5.0))
    print(f"M={M} T={temperature}: loss {loss!r}, {u:.2f} ulp from log 5")
    assert u <= 2.0, (loss, u)
    want = np.array([0.2 - 1, 0.2, 0.2, 0.2, 0.2]) / (temperature * M)
    gu = _ulps(grad, np.tile(want, (M, 1)))
    print(f"M={M} T={temperature}: grad max {gu.max():.2f} ulp")
    assert gu.max() <= 1.0, gu.max()


# ===========================================================================
# 2. distill_loss_fwd, general case
# ===========================================================================

@pytest.mark.parametrize("kind", dp.KINDS)
@pytest.mark.parametrize("temperature", [1.0, 2.0])
@pytest.mark.parametrize("M", dp.MS)
def test_loss_general_against_twin(ext, M, temperature, kind):
    """Random logits in [-8, 8] plus the clamp rows against the float64
    twin on the same fp32 inputs. The allowance is 4x the largest error of
    fp32 DistillationLoss under torch autograd on CPU against the same
    twin, per gradient element and for the scalar: measured here, not
    fixed in advance."""
    teacher, student = dp.random_logits(M, 100 + M)
    want_loss, want_grad = dp.distill_twin(teacher, student, temperature,
                                           kind)
    ref_loss, ref_grad = dp.torch_loss_and_grad(
        teacher, student, temperature, kind, torch.float32)
    yard_grad = np.abs(ref_grad - want_grad).max()
    yard_loss = abs(ref_loss - want_loss)
    loss, grad = _loss_call(ext, teacher, student, temperature, kind)
    err_grad = np.abs(grad.astype(np.float64) - want_grad).max()
    err_loss = abs(float(loss) - want_loss)
    print(f"M={M} T={temperature} {kind}: yardstick grad {yard_grad:.3e} "
          f"loss {yard_loss:.3e}; kernel grad {err_grad:.3e} "
          f"loss {err_loss:.3e} (loss {want_loss:.6g}, "
          f"max |grad| {np.abs(want_grad).max():.3e})")
    assert err_grad <= YARDSTICK_FACTOR * yard_grad, (err_grad, yard_grad)
    assert err_loss <= YARDSTICK_FACTOR * yard_loss, (err_loss, yard_loss)
    # Fixed-order reduction: a second launch gives the same bits.
    loss2, grad2 = _loss_call(ext, teacher, student, temperature, kind)
    assert loss.tobytes() == loss2.tobytes()
    assert grad.tobytes() == grad2.tobytes()


@pytest.mark.parametrize("kind", dp.KINDS)
def test_fused_impl_autograd(ext, kind):
    """impl="fused": same loss bits as the kernel, and backward hands
    student_logits the kernel's gradient times the upstream scalar; the
    teacher gets none."""
    teacher, student = dp.random_logits(257, 7)
    t = torch.from_numpy(teacher).cuda().view(1, 257, 5).requires_grad_(True)
    s = torch.from_numpy(student).cuda().view(1, 257, 5).requires_grad_(True)
    want_loss, want_grad = ext.distill_loss_fwd(
        t.detach().view(-1, 5), s.detach().view(-1, 5), 2.0,
        dp.KIND_ID[kind])
    loss = losses_lib.DistillationLoss(2.0, kind, impl="fused")(t, s)
    assert torch.equal(loss, want_loss)
    (loss * 3.0).backward()
    assert t.grad is None
    assert s.grad.shape == s.shape
    assert torch.equal(s.grad.view(-1, 5), want_grad * 3.0)


# ===========================================================================
# 3. ln_head_logits
# ===========================================================================

def _logits_ref64(x, gamma, beta, w_head, b_head):
    xd = x.double()
    n = torch.nn.functional.layer_norm(
        xd, (xd.shape[-1],), gamma.double(), beta.double(), kp.LN_EPS)
    return n @ w_head.double().t() + b_head.double()


@pytest.mark.parametrize("H,dtype", [(280, kp.BF16), (32, torch.float32)])
def test_ln_head_logits_conditioning(ext, H, dtype):
    """kernel_probes.ln_rows (near-constant rows down to s/|c| = 1e-4 at
    means up to 300, and exactly constant rows) through LayerNorm + head:
    softmax of the kernel's logits against float64 LayerNorm + head +
    softmax of the same stored inputs, inside kernel_probes.ln_bound, the
    bound the LN + head stage of fused_ln_head_qv is held to."""
    x, labels = kp.ln_rows(H, 800 + H)
    x = x.to(dtype)
    n = x.shape[0]
    for pname, params in kp.ln_param_sets(H):
        tag = f"H={H} {pname}"
        buf, out = _guarded_out(n)
        got = ext.ln_head_logits(
            _with_nan_tail(x), *(p.float().cuda() for p in params), out)
        assert got.data_ptr() == out.data_ptr()
        _assert_guard(buf, n, tag)
        fresh = ext.ln_head_logits(
            x.cuda(), *(p.float().cuda() for p in params))
        assert fresh.shape == (n, 5) and fresh.dtype == torch.float32
        assert torch.equal(fresh, got)
        logits = got.cpu().double()
        ref = kp.ln_head_ref(x, *params)
        err = (torch.softmax(logits, -1) - ref).abs()
        print(f"{tag}: max |softmax(logits) - ref64| = "
              f"{err.max().item():.3e}")
        ok = err <= kp.ln_bound(ref)
        where = kp.first_bad(ok)
        assert ok.all(), (
            f"{tag}: row {where[0]} (c, s)={labels[where[0]]} class "
            f"{where[1]}")
        # Exactly constant rows normalise to 0: the logits are
        # beta @ w_head^T + b_head whatever the constant.
        const = [i for i, (_, s) in enumerate(labels) if s == 0.0]
        ref_logits = _logits_ref64(x, *params)
        assert (logits[const] - ref_logits[const]).abs().max() <= 1e-4


@pytest.mark.parametrize("N", [1, 3, 5, 8197])
def test_ln_head_logits_persistent_loop(ext, N):
    """N = 8197 > 2048 blocks x 4 waves: rows of a wave's second trip too.
    Well-conditioned rows, so the logits themselves are compared: bf16
    inputs are exact in float64, the rest is fp32 arithmetic over H = 280
    terms, far inside atol 2e-4 + rtol 1e-3."""
    H = 280
    g = torch.Generator().manual_seed(N)
    x = (2.0 * torch.randn(N, H, generator=g)).to(kp.BF16)
    params = kp.ln_params_random(H, 31)
    buf, out = _guarded_out(N)
    ext.ln_head_logits(_with_nan_tail(x),
                       *(p.float().cuda() for p in params), out)
    _assert_guard(buf, N, f"N={N}")
    ref = _logits_ref64(x, *params)
    err = (out.cpu().double() - ref).abs()
    assert (err <= kp.LN_ATOL + kp.LN_RTOL * ref.abs()).all(), err.max()


# ===========================================================================
# 4. Native teacher
# ===========================================================================

def test_native_teacher_logits():
    """A randomly initialised 280/2048 teacher at B = 8, L = 100."""
    from test_gpu_kernels import _make_rows

    params = cfg.get_config("transformer_learn_values+custom")
    cfg.modify_params(params, is_training=False)
    torch.manual_seed(7)
    model = get_model(params)
    ref_model = copy.deepcopy(model).float()
    runner = InferenceRunner(params, model, device="cuda:0")
    assert runner.native
    rows = _make_rows(params, B=8)
    logits = runner.logits_native(rows)
    assert logits.shape == (8, 100, 5) and logits.dtype == torch.float32
    assert torch.isfinite(logits).all()
    with torch.no_grad():
        ref = ref_model.encode(rows.float(), training=False)["logits"]
    agree = (logits.argmax(-1).cpu() == ref.argmax(-1)).float().mean()
    print(f"argmax agreement with torch: {float(agree):.4f}")
    assert agree > 0.98, float(agree)
    # Same rows through the serving head: the calls match wherever the
    # top two probabilities are more than 0.01 apart.
    bases, _ = runner.forward_windows(rows)
    probs = torch.softmax(logits, -1)
    top2 = probs.topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > 0.01
    assert clear.any()
    assert torch.equal(probs.argmax(-1)[clear], bases.long()[clear])


# ===========================================================================
# 5. End to end
# ===========================================================================

def _distill_run(out_dir, teacher_dir, train_file, seed, teacher_mode,
                 distill_loss):
    from deepconsensus_amd.models import distill as distill_lib

    params = cfg.get_config("transformer_learn_values_distill+test")
    params.train_path = [train_file]
    params.eval_path = [train_file]
    params.batch_size = 4
    params.num_epochs = 4
    params.n_examples_train = 12
    params.seed = seed
    cfg.modify_params(params)
    return distill_lib.train_model(
        out_dir, teacher_dir, params, device="cuda:0", eval_every=2,
        limit_steps=4, use_bf16=True, teacher_mode=teacher_mode,
        distill_loss_impl=distill_loss,
    )


def test_distill_e2e_device_modes(tmp_path):
    """distill --bf16 --teacher_mode native --distill_loss fused for 4 steps:
    both checkpoints, finite metrics, and eval/distill_loss no further from
    the two torch/torch runs (dropout seeds 1 and 2) than they are from
    each other: |x - (a + b) / 2| <= |a - b|."""
    from test_train import make_training_data

    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "distill_digest", os.path.join(root, "scripts", "distill_digest.py"))
    digest = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(digest)

    train_file, _ = make_training_data(tmp_path)
    teacher_dir = digest.make_teacher(tmp_path, train_file)
    torch_runs = [
        _distill_run(str(tmp_path / f"torch{seed}"), teacher_dir,
                     train_file, seed, "torch", "torch")
        for seed in (1, 2)
    ]
    out_dir = str(tmp_path / "device")
    got = _distill_run(out_dir, teacher_dir, train_file, 1, "native",
                       "fused")
    assert got["steps"] == 4
    names = sorted(os.path.basename(p)
                   for p in glob.glob(os.path.join(out_dir, "checkpoint-*")))
    assert names == ["checkpoint-2.pt", "checkpoint-4.pt"]
    for key, value in got.items():
        assert math.isfinite(value), (key, value)
    a, b = (r["eval/distill_loss"] for r in torch_runs)
    x = got["eval/distill_loss"]
    print(f"eval/distill_loss: torch/torch {a:.6e} {b:.6e}, "
          f"native/fused {x:.6e}")
    assert abs(x - (a + b) / 2) <= abs(a - b), (x, a, b)
