"""Distillation trainer.

Parity with reference model_distillation.py:104-522: a frozen teacher loaded
from a checkpoint, a smaller student (transformer_learn_values_distill
config) initialized from a teacher layer map, combined loss
student_alpha * AlignmentLoss + distill_alpha * DistillationLoss on logits,
and train.py's loop contracts (model_distillation.py:170-470): evaluation
every eval_every steps and at the end, a checkpoint of student + optimizer
with its metrics at every evaluation, best/eval checkpoint sidecars, resume
from the latest checkpoint, train/eval event files, training_summary.json.
The teacher is reloaded from its own checkpoint on every start and never
saved.

Two opt-in device paths (both default to torch):
  * --teacher_mode native runs the frozen teacher on the serving kernels
    (InferenceRunner.logits_native: encode_native + ln_head_logits); its
    activations are bf16 whether or not --bf16 is given;
  * --distill_loss fused computes the distillation loss and its gradient in
    one HIP kernel (ops/hip/distill_loss.hip).

Resume differs from train.py in one point: a run that finishes all its
epochs records num_epochs (not num_epochs - 1) as its epoch, and every
checkpoint carries the torch RNG state, so that continuing a finished run
with a larger --epochs repeats nothing and, on CPU, gives the weights of
one uninterrupted run.
"""
from __future__ import annotations

import argparse
import logging
import os
import time
from typing import List, Optional

import torch

from deepconsensus_amd.models import checkpoint as ckpt_lib
from deepconsensus_amd.models import config as cfg
from deepconsensus_amd.models import data_device
from deepconsensus_amd.models import lamb as lamb_lib
from deepconsensus_amd.models import losses as losses_lib
from deepconsensus_amd.models.model import get_model
from deepconsensus_amd.models import train as train_lib
from deepconsensus_amd.models.train import _prepare_batch  # noqa: F401
from deepconsensus_amd.parallel import comm
from deepconsensus_amd.utils import trace

log = logging.getLogger(__name__)

TEACHER_MODES = ("torch", "native")


def resolve_teacher_mode(mode: Optional[str] = None) -> str:
    """Flag value, else DC_TEACHER_MODE, else torch."""
    mode = mode or os.environ.get("DC_TEACHER_MODE") or "torch"
    if mode not in TEACHER_MODES:
        raise ValueError(
            f"unknown teacher mode {mode!r}; choices: "
            f"{', '.join(TEACHER_MODES)}"
        )
    return mode


def check_device_modes(device: str, teacher_mode: str,
                       distill_loss: str) -> None:
    """The device-only modes fail at start-up elsewhere: no fallback."""
    on_gpu = torch.device(device).type == "cuda"
    if teacher_mode == "native" and not on_gpu:
        raise ValueError(
            f"--teacher_mode native runs the teacher on the HIP serving "
            f"kernels and needs a cuda device, not {device!r}"
        )
    if distill_loss == "fused" and not on_gpu:
        raise ValueError(
            f"--distill_loss fused is a HIP kernel and needs a cuda "
            f"device, not {device!r}"
        )


def _rng_state(device: str) -> dict:
    state = {"rng_state": torch.get_rng_state()}
    if torch.device(device).type == "cuda":
        state["cuda_rng_state"] = torch.cuda.get_rng_state(device)
    return state


def _restore_rng_state(payload: dict, device: str) -> None:
    if payload.get("rng_state") is not None:
        torch.set_rng_state(payload["rng_state"])
    if (payload.get("cuda_rng_state") is not None
            and torch.device(device).type == "cuda"):
        torch.cuda.set_rng_state(payload["cuda_rng_state"], device)


def get_teacher_model(teacher_ckpt: str, device: str):
    """Loads and freezes the teacher (model_distillation.py:147-167)."""
    params = ckpt_lib.load_params(teacher_ckpt)
    cfg.modify_params(params, is_training=False)
    model = get_model(params)
    ckpt_lib.load_checkpoint(teacher_ckpt, model)
    model.to(device).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model, params


def init_student_from_teacher(student, teacher, params) -> None:
    """Copies mapped encoder layers + non-encoder weights
    (model_distillation.py:104-144)."""
    if params.get("init_encoder_stack", False):
        for t_i, s_i in zip(
            params.teacher_encoder_layers, params.student_encoder_layers
        ):
            student.layers[s_i].load_state_dict(
                teacher.layers[t_i].state_dict()
            )
    if params.get("init_nonencoder_layers", False):
        student.bases_embedding.load_state_dict(
            teacher.bases_embedding.state_dict()
        )
        student.pw_embedding.load_state_dict(
            teacher.pw_embedding.state_dict()
        )
        student.ip_embedding.load_state_dict(
            teacher.ip_embedding.state_dict()
        )
        student.strand_embedding.load_state_dict(
            teacher.strand_embedding.state_dict()
        )
        student.sn_embedding.load_state_dict(
            teacher.sn_embedding.state_dict()
        )
        if student.condense and teacher.condense:
            student.condenser.load_state_dict(
                teacher.condenser.state_dict()
            )
        student.output_norm.load_state_dict(
            teacher.output_norm.state_dict()
        )
        student.fc1.load_state_dict(teacher.fc1.state_dict())


def train_model(
    out_dir: str,
    teacher_ckpt: str,
    params: cfg.Params,
    device: str = "cpu",
    eval_every: int = 3000,
    limit_steps: int = 0,
    use_bf16: bool = False,
    input_mode: Optional[str] = None,
    input_workers: Optional[int] = None,
    write_checkpoint_metrics: bool = True,
    teacher_mode: Optional[str] = None,
    distill_loss_impl: Optional[str] = None,
    log_every: int = 10,
) -> dict:
    """Runs the distillation loop; returns the final eval metrics + steps.

    teacher_mode / distill_loss_impl: see the module docstring
    (DC_TEACHER_MODE / DC_DISTILL_LOSS set the defaults). limit_steps
    counts this call's steps, as in train.
    """
    from deepconsensus_amd.utils.tuned_gemm import enable_tuned_gemms

    enable_tuned_gemms()
    input_mode = data_device.resolve_input_mode(input_mode)
    teacher_mode = resolve_teacher_mode(teacher_mode)
    distill_loss_impl = losses_lib.resolve_distill_loss_impl(
        distill_loss_impl
    )
    check_device_modes(device, teacher_mode, distill_loss_impl)
    rank, world = comm.init_distributed()
    main = rank == 0
    os.makedirs(out_dir, exist_ok=True)
    if main:
        cfg.save_params_as_json(out_dir, params)

    teacher, teacher_params = get_teacher_model(teacher_ckpt, device)
    teacher_runner = None
    if teacher_mode == "native":
        from deepconsensus_amd.models.runner import InferenceRunner

        teacher_runner = InferenceRunner(
            teacher_params, model=teacher, device=device
        )
        if not teacher_runner.native:
            raise ValueError(
                "--teacher_mode native needs a learned-values teacher with "
                f"a condenser; {teacher_params.model_name!r} is not one"
            )
    torch.manual_seed(params.seed)
    student = get_model(params).to(device)

    global_batch, steps_per_epoch, decay_steps = (
        train_lib.decay_schedule_steps(params, world)
    )
    optimizer, schedule = lamb_lib.create_optimizer(
        params, decay_steps, student
    )

    # Resume; a fresh start seeds the student from the teacher instead.
    resume_path, initial_epoch, step = (
        ckpt_lib.get_checkpoint_and_initial_epoch(out_dir)
    )
    if resume_path:
        payload = ckpt_lib.load_checkpoint(resume_path, student, optimizer)
        _restore_rng_state(payload, device)
        log.info("resumed from %s (epoch %d step %d)", resume_path,
                 initial_epoch, step)
    else:
        init_student_from_teacher(student, teacher, params)
    comm.broadcast_parameters(student)
    reducer = comm.FlatGradAllreducer(student)

    align_loss = losses_lib.AlignmentLoss(
        del_cost=params.del_cost, loss_reg=params.loss_reg,
        width=params.get("band_width"), reduction="sum",
    )
    distill_loss = losses_lib.DistillationLoss(
        temperature=params.get("temperature", 1.0),
        logit_loss=params.get("logit_loss_identifier", "kl_divergence"),
        impl=distill_loss_impl,
    )
    student_alpha = params.get("student_alpha", 1.0)
    distill_alpha = params.get("distill_alpha", 1.0)

    train_ds = data_device.make_input(
        params.train_path, params, params.batch_size, device,
        input_mode=input_mode, input_workers=input_workers, rank=rank,
        world_size=world, seed=params.seed, limit=params.get("limit", -1),
    )
    eval_ds = data_device.make_input(
        params.eval_path, params, params.batch_size, device,
        input_mode=input_mode, input_workers=input_workers, shuffle=False,
        rank=rank, world_size=world, limit=params.get("limit", -1),
    )

    def teacher_logits(rows):
        with trace.range("teacher_forward"), torch.no_grad():
            if teacher_runner is not None:
                return teacher_runner.logits_native(rows)
            return teacher.encode(rows, training=False)["logits"]

    def forward_pair(rows, training):
        """(teacher logits, student logits). bf16 autocast: both forwards
        take the fused MFMA banded-attention path on GPU (model.py); losses
        stay fp32."""
        if use_bf16 and rows.is_cuda:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                t_logits = teacher_logits(rows)
                with trace.range("student_forward"):
                    s_out = student.encode(rows, training=training)
        else:
            t_logits = teacher_logits(rows)
            with trace.range("student_forward"):
                s_out = student.encode(rows, training=training)
        return t_logits, s_out["logits"]

    def losses_of(t_logits, s_logits, label, batch_div):
        probs = torch.softmax(s_logits.float(), -1)
        l_student = align_loss(label, probs) / batch_div
        l_distill = distill_loss(t_logits.float(), s_logits.float())
        loss = student_alpha * l_student + distill_alpha * l_distill
        return loss, l_student, l_distill, probs

    def run_eval() -> dict:
        student.eval()
        eval_metrics = train_lib.EvalMetrics(params.max_passes)
        totals, n_batches = [0.0, 0.0, 0.0], 0
        with torch.no_grad():
            for rows, label in eval_ds.iterate():
                t_logits, s_logits = forward_pair(rows, training=False)
                loss, l_student, l_distill, probs = losses_of(
                    t_logits, s_logits, label, max(label.shape[0], 1)
                )
                for i, v in enumerate((loss, l_student, l_distill)):
                    totals[i] += float(v)
                n_batches += 1
                eval_metrics.update(rows, label, probs)
        student.train()
        n = max(n_batches, 1)
        metrics = {
            name: comm.allreduce_scalar(total / n) / world
            for name, total in zip(
                ("eval/loss", "eval/student_loss", "eval/distill_loss"),
                totals,
            )
        }
        metrics.update(eval_metrics.result())
        return metrics

    train_writer = eval_writer = None
    if main:
        train_writer, eval_writer = train_lib.open_summary_writers(out_dir)

    def evaluate_and_save(epoch_to_record: int) -> dict:
        metrics = run_eval()
        if main:
            train_lib.save_eval_checkpoint(
                out_dir, step, epoch_to_record, student, optimizer, params,
                metrics, write_checkpoint_metrics, extra=_rng_state(device),
            )
            log.info("eval @%d: %s", step, metrics)
            eval_writer.add_scalars(step, metrics)
            eval_writer.flush()
            train_writer.flush()
        return metrics

    student.train()
    metrics = None
    last_eval_step = -1
    steps_this_session = 0
    epoch = initial_epoch
    stopped_early = False
    t0 = time.time()
    for epoch in range(initial_epoch, params.num_epochs):
        for rows, label in train_ds.iterate(epoch):
            lr = schedule.apply(optimizer, step)
            reducer.zero_()
            with trace.range("distill_step"):
                t_logits, s_logits = forward_pair(rows, training=True)
                with trace.range("losses"):
                    loss, l_student, l_distill, _ = losses_of(
                        t_logits, s_logits, label, global_batch
                    )
                with trace.range("backward"):
                    loss.backward()
                with trace.range("allreduce"):
                    reducer.reduce()
                with trace.range("lamb_step"):
                    optimizer.step()
            step += 1
            steps_this_session += 1
            if main and step % log_every == 0:
                steps_per_sec = steps_this_session / (time.time() - t0)
                log.info(
                    "epoch %d step %d loss %.4f (student %.4f distill %.6f) "
                    "lr %.2e (%.2f steps/s)",
                    epoch, step, float(loss.detach()),
                    float(l_student.detach()), float(l_distill.detach()),
                    lr, steps_per_sec,
                )
                train_writer.add_scalars(step, {
                    "train/loss": float(loss.detach()),
                    "train/student_loss": float(l_student.detach()),
                    "train/distill_loss": float(l_distill.detach()),
                    "train/learning_rate": lr,
                    "train/steps_per_second": steps_per_sec,
                })
            stopped_early = bool(
                limit_steps and steps_this_session >= limit_steps
            )
            if step % eval_every == 0 or stopped_early:
                metrics = evaluate_and_save(epoch)
                last_eval_step = step
            if stopped_early:
                break
        if stopped_early:
            break

    # Final eval + checkpoint. A run that went through all its epochs
    # records num_epochs, so a later call with more epochs starts at the
    # next one; a run cut short by limit_steps resumes inside its epoch.
    final_epoch = epoch if stopped_early else params.num_epochs
    if last_eval_step != step or metrics is None:
        metrics = evaluate_and_save(final_epoch)
    elif main and not stopped_early:
        ckpt_lib.save_checkpoint(
            out_dir, step, final_epoch, student, optimizer, params,
            extra=_rng_state(device),
        )
    summary = dict(metrics)
    summary["steps"] = step
    if main:
        train_writer.close()
        eval_writer.close()
        train_lib.write_training_summary(out_dir, summary)
    return summary


def main(argv: Optional[List[str]] = None) -> None:
    ap = argparse.ArgumentParser("deepconsensus distill")
    ap.add_argument("--params",
                    default="transformer_learn_values_distill+test")
    ap.add_argument("--teacher_checkpoint", required=True)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--train_path", default=None)
    ap.add_argument("--eval_path", default=None,
                    help="eval data (default: the train path)")
    ap.add_argument("--n_examples_train", type=int, default=None)
    ap.add_argument("--n_examples_eval", type=int, default=None)
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--eval_every", type=int, default=3000)
    ap.add_argument("--limit_steps", type=int, default=0)
    ap.add_argument("--device", default=None)
    ap.add_argument("--bf16", action="store_true",
                    help="autocast forwards to bf16 (fused MFMA "
                    "attention path on GPU)")
    ap.add_argument("--input_mode", default=None,
                    help="host (default) or device: as for train "
                    "(DC_INPUT_MODE sets the default)")
    ap.add_argument("--input_workers", type=int, default=None,
                    help="reader processes of --input_mode device "
                    "(0 reads in-process)")
    ap.add_argument("--write_checkpoint_metrics", type=lambda v: v != "false",
                    default=True,
                    help="append eval metrics to checkpoint_metrics.tsv")
    ap.add_argument("--eval_and_log_every_step", action="store_true",
                    help="debug: log every step and eval every step")
    ap.add_argument("--teacher_mode", default=None, choices=TEACHER_MODES,
                    help="torch (default): teacher.encode; native: the "
                    "frozen teacher runs on the HIP serving kernels (cuda, "
                    "learned-values model with a condenser). "
                    "DC_TEACHER_MODE sets the default")
    ap.add_argument("--distill_loss", default=None,
                    choices=losses_lib.DISTILL_LOSS_IMPLS,
                    help="torch (default): elementwise chain under "
                    "autograd; fused: one HIP kernel for loss and gradient "
                    "(cuda). DC_DISTILL_LOSS sets the default")
    args = ap.parse_args(argv)
    params = cfg.get_config(args.params)
    if args.train_path:
        params.train_path = [args.train_path]
        params.eval_path = [args.train_path]
    if args.eval_path:
        params.eval_path = [args.eval_path]
    if args.batch_size:
        params.batch_size = args.batch_size
    if args.epochs:
        params.num_epochs = args.epochs
    if args.n_examples_train:
        params.n_examples_train = args.n_examples_train
    if args.n_examples_eval:
        params.n_examples_eval = args.n_examples_eval
    cfg.modify_params(params)
    device = args.device or (
        "cuda" if torch.cuda.is_available() else "cpu"
    )
    try:
        teacher_mode = resolve_teacher_mode(args.teacher_mode)
        distill_loss = losses_lib.resolve_distill_loss_impl(
            args.distill_loss
        )
        check_device_modes(device, teacher_mode, distill_loss)
    except ValueError as e:
        ap.error(str(e))
    every_step = args.eval_and_log_every_step
    train_model(args.out_dir, args.teacher_checkpoint, params,
                device=device,
                eval_every=1 if every_step else args.eval_every,
                limit_steps=args.limit_steps,
                use_bf16=getattr(args, "bf16", False),
                input_mode=args.input_mode,
                input_workers=args.input_workers,
                write_checkpoint_metrics=args.write_checkpoint_metrics,
                teacher_mode=teacher_mode, distill_loss_impl=distill_loss,
                log_every=1 if every_step else 10)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
