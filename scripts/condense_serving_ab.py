"""Serving A/B for the condenser: DC_FUSED_CONDENSE unset vs wide.

Builds one model for the chosen layout and two InferenceRunners in one
process (library fallback vs fused_condense at the layout's width), then
alternates them for --rounds rounds of --steps graphed serving steps,
timed with HIP events. Independent of bench.py (which only runs the
560 layout). Prints windows/s per arm and round.

  python scripts/condense_serving_ab.py --bq            # 86 rows, K=568
  python scripts/condense_serving_ab.py --max_passes 32 # 133 rows, K=872
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from deepconsensus_amd.models import config as cfg
from deepconsensus_amd.models.model import get_model
from deepconsensus_amd.models.runner import InferenceRunner


def make_rows(params, batch, seed=0):
    rng = np.random.default_rng(seed)
    R, L, mp = params.total_rows, params.max_length, params.max_passes
    rows = np.zeros((batch, R, L), dtype=np.float32)
    rows[:, 0:mp] = rng.integers(0, 5, size=(batch, mp, L))
    rows[:, mp:3 * mp] = rng.integers(0, 256, size=(batch, 2 * mp, L))
    rows[:, 3 * mp:4 * mp] = rng.integers(0, 3, size=(batch, mp, L))
    rows[:, 4 * mp] = rng.integers(0, 5, size=(batch, L))
    if params.use_ccs_bq:
        rows[:, 4 * mp + 1] = rng.integers(-1, 94, size=(batch, L))
    rows[:, -4:] = rng.integers(0, 501, size=(batch, 4, 1))
    return torch.from_numpy(rows)


def make_runner(params, model, value):
    if value is None:
        os.environ.pop("DC_FUSED_CONDENSE", None)
    else:
        os.environ["DC_FUSED_CONDENSE"] = value
    return InferenceRunner(params, model, device="cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bq", action="store_true")
    ap.add_argument("--max_passes", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    params = cfg.get_config("transformer_learn_values+custom")
    params.use_ccs_bq = args.bq
    params.max_passes = args.max_passes
    cfg.modify_params(params, is_training=False)
    torch.manual_seed(0)
    model = get_model(params)
    arms = {
        "unset": make_runner(params, model, None),
        "wide": make_runner(params, model, "wide"),
    }
    os.environ.pop("DC_FUSED_CONDENSE", None)
    k = arms["wide"].cond_wt.shape[0]
    assert arms["wide"].cond_img is not None, f"width {k} not supported"
    rows = make_rows(params, args.batch).to("cuda:0")
    for r in arms.values():
        for _ in range(args.warmup):
            r.forward_windows_graphed(rows)
    torch.cuda.synchronize()

    per_arm = {name: [] for name in arms}
    for rnd in range(args.rounds):
        for name, r in arms.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.steps):
                r.forward_windows_graphed(rows)
            t1.record()
            t1.synchronize()
            ms = t0.elapsed_time(t1) / args.steps
            per_arm[name].append(ms)
            print(f"round {rnd} {name:5s} fused={r.cond_img is not None} "
                  f"{ms:.3f} ms/step {args.batch / ms * 1e3:.0f} windows/s")
    for name, ms in per_arm.items():
        print(f"{name:5s} rows={params.total_rows} K={k} batch={args.batch} "
              f"median {statistics.median(ms):.3f} ms/step "
              f"min..max {min(ms):.3f}..{max(ms):.3f}")


if __name__ == "__main__":
    main()
