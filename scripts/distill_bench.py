#!/usr/bin/env python3
"""Distillation-step benchmark: what the teacher forward and the loss chain
cost, and what --teacher_mode native / --distill_loss fused change.

A resident synthetic batch, a randomly initialised 6-layer teacher and the
5-layer transformer_learn_values_distill student seeded from it. Four arms,
each with its own student and optimizer: teacher torch|native x loss
torch|fused (torch/torch is the default path). After a warm-up of every arm
the arms alternate, --rounds rounds of --steps steps each, every round
timed by a host clock around work that ends in a device synchronise. A
last pass times the phases of one step of every arm with device events
(teacher forward, student forward, losses, backward, optimizer); it
synchronises between phases, so its sum exceeds the step time above.

Prints one JSON object (and writes it to --out). Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deepconsensus_amd.models import config as cfg
from deepconsensus_amd.models import distill as distill_lib
from deepconsensus_amd.models import lamb as lamb_lib
from deepconsensus_amd.models import losses as losses_lib
from deepconsensus_amd.models.model import get_model
from deepconsensus_amd.models.runner import InferenceRunner
from deepconsensus_amd.parallel import comm

ARMS = (("torch", "torch"), ("native", "torch"), ("torch", "fused"),
        ("native", "fused"))
PHASES = ("teacher_forward", "student_forward", "losses", "backward",
          "optimizer")


def synthetic_batch(params, batch, device):
    rng = np.random.default_rng(42)
    L, mp = params.max_length, params.max_passes
    rows = np.zeros((batch, params.total_rows, L), dtype=np.float32)
    rows[:, 0:mp] = rng.integers(0, 5, size=(batch, mp, L))
    rows[:, mp:2 * mp] = rng.integers(0, 256, size=(batch, mp, L))
    rows[:, 2 * mp:3 * mp] = rng.integers(0, 256, size=(batch, mp, L))
    rows[:, 3 * mp:4 * mp] = rng.integers(0, 3, size=(batch, mp, L))
    rows[:, 4 * mp] = rng.integers(0, 5, size=(batch, L))
    rows[:, -4:] = rng.integers(5, 30, size=(batch, 4, 1))
    label = rng.integers(0, 5, size=(batch, L)).astype(np.int64)
    return (torch.from_numpy(rows).to(device),
            torch.from_numpy(label).to(device))


class Arm:
    """One (teacher mode, loss impl) pair: models/distill.py's step."""

    def __init__(self, teacher, runner, params, teacher_mode, loss_impl,
                 bf16, device):
        self.name = f"{teacher_mode}/{loss_impl}"
        self.teacher = teacher
        self.runner = runner if teacher_mode == "native" else None
        self.bf16 = bf16
        torch.manual_seed(params.seed)
        self.student = get_model(params).to(device)
        distill_lib.init_student_from_teacher(self.student, teacher, params)
        self.student.train()
        self.optimizer, self.schedule = lamb_lib.create_optimizer(
            params, 10000, self.student)
        self.reducer = comm.FlatGradAllreducer(self.student)
        self.align = losses_lib.AlignmentLoss(
            del_cost=params.del_cost, loss_reg=params.loss_reg,
            width=params.get("band_width"), reduction="sum")
        self.distill = losses_lib.DistillationLoss(
            temperature=params.get("temperature", 1.0),
            logit_loss=params.get("logit_loss_identifier", "kl_divergence"),
            impl=loss_impl)
        self.alphas = (params.get("student_alpha", 1.0),
                       params.get("distill_alpha", 1.0))
        self.i = 0

    def _autocast(self):
        return torch.autocast("cuda", dtype=torch.bfloat16,
                              enabled=self.bf16)

    def step(self, rows, label, mark=None):
        """One step; mark(phase) is called where each phase ends."""
        mark = mark or (lambda phase: None)
        self.schedule.apply(self.optimizer, self.i)
        self.reducer.zero_()
        with self._autocast():
            with torch.no_grad():
                if self.runner is not None:
                    t_logits = self.runner.logits_native(rows)
                else:
                    t_logits = self.teacher.encode(
                        rows, training=False)["logits"]
            mark("teacher_forward")
            s_logits = self.student.encode(rows, training=True)["logits"]
        mark("student_forward")
        probs = torch.softmax(s_logits.float(), -1)
        l_student = self.align(label, probs) / rows.shape[0]
        l_distill = self.distill(t_logits.float(), s_logits.float())
        loss = self.alphas[0] * l_student + self.alphas[1] * l_distill
        mark("losses")
        loss.backward()
        self.reducer.reduce()
        mark("backward")
        self.optimizer.step()
        mark("optimizer")
        self.i += 1
        return loss


def time_phases(arm, rows, label, repeats):
    """Mean ms per phase over `repeats` steps, by device events."""
    totals = dict.fromkeys(PHASES, 0.0)
    for _ in range(repeats):
        events = [torch.cuda.Event(enable_timing=True)]
        torch.cuda.synchronize()
        events[0].record()

        def mark(phase):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            e.synchronize()
            events.append(e)

        arm.step(rows, label, mark)
        for phase, a, b in zip(PHASES, events, events[1:]):
            totals[phase] += a.elapsed_time(b)
    return {phase: total / repeats for phase, total in totals.items()}


def main():
    from deepconsensus_amd.utils.tuned_gemm import enable_tuned_gemms

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--phase-steps", type=int, default=3)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("distill_bench.py measures on a GPU; none is visible")
    enable_tuned_gemms()
    device = "cuda:0"

    t_params = cfg.get_config("transformer_learn_values+custom")
    cfg.modify_params(t_params, is_training=False)
    torch.manual_seed(7)
    teacher = get_model(t_params).to(device).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    runner = InferenceRunner(t_params, model=teacher, device=device)
    assert runner.native
    s_params = cfg.get_config("transformer_learn_values_distill+custom")
    cfg.modify_params(s_params)
    rows, label = synthetic_batch(s_params, args.batch_size, device)

    arms = [Arm(teacher, runner, s_params, tm, li, args.bf16, device)
            for tm, li in ARMS]
    for arm in arms:
        for _ in range(args.warmup):
            arm.step(rows, label)
    torch.cuda.synchronize()

    ms = {arm.name: [] for arm in arms}
    for _ in range(args.rounds):
        for arm in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                arm.step(rows, label)
            torch.cuda.synchronize()
            ms[arm.name].append(
                (time.perf_counter() - t0) / args.steps * 1000)
    phases = {arm.name: time_phases(arm, rows, label, args.phase_steps)
              for arm in arms}
    result = {
        "device": torch.cuda.get_device_name(0),
        "batch_size": args.batch_size, "bf16": args.bf16,
        "teacher_layers": t_params.num_hidden_layers,
        "student_layers": s_params.num_hidden_layers,
        "logit_loss": s_params.get("logit_loss_identifier"),
        "steps_per_round": args.steps, "warmup": args.warmup,
        "ms_per_step_by_round": ms,
        "ms_per_step_median": {k: float(np.median(v))
                               for k, v in ms.items()},
        "phase_ms": phases,
    }
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
