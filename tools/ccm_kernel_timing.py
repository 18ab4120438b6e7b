#!/usr/bin/env python3
"""Kernel time of the cell_cycle_marker likelihood on the GPU: the wavefront-per-evaluation kernel
against the one-lane-per-evaluation variant (BCM3HIP_OPT_CCM_ONE_LANE), on a synthetic track of 240
frames at 8, 256 and 65536 evaluations (DESIGN.md §4 "cell cycle marker").

Device-resident batches; every launch is timed by its own HIP event pair (BCM3HIP_OPT_TIMING_LOG).
Each size is warmed up in both variants, then timed in rounds that alternate the variants, and the
two results are compared bit for bit. Prints one JSON line per (variant, n); --out appends them to a
file. Usage: python tools/ccm_kernel_timing.py [--out FILE] [--frames 240] [--rounds 7] [--launches 50]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 256, 65536])
    a = ap.parse_args()

    import torch
    import ccm_reference as R
    from bcm3_amd import _hip
    assert torch.cuda.is_available(), "needs a GPU"

    # a track drawn from the model: S entry at 40, mitosis at 200, t(4) noise of the model's scale
    rng = np.random.default_rng(1)
    truth = np.array([40.0, 90.0, 70.0, 6.0, 1.2, 0.2, 0.3, 0.2, 0.5, 0.02])
    clean = np.empty(a.frames)
    for i in range(a.frames):
        x = truth[3]
        if i > 200.0:
            x += (90.0 * 1.2 + 70.0 * 0.2) * 0.3 - 0.2 * (i - 200.0)
        elif i > 130.0:
            x += 90.0 * 1.2 + (i - 130.0) * 0.2
        elif i > 40.0:
            x += 1.2 * (i - 40.0)
        clean[i] = x
    track = clean + (0.5 + 0.02 * clean) * rng.standard_t(4, a.frames)
    track[[17, a.frames // 2]] = np.nan

    ctx = _hip.Context.cell_cycle_marker(track)
    ctx.set_option(_hip.OPT_TIMING_LOG, 1)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []
    for n in a.sizes:
        xd = torch.tensor(R.draws(n, 5), dtype=torch.float64, device="cuda:0")
        out = {v: torch.empty(n, dtype=torch.float64, device="cuda:0") for v in (0, 1)}
        st = torch.empty(n, dtype=torch.int32, device="cuda:0")

        def run(variant, launches):
            ctx.set_option(_hip.OPT_CCM_ONE_LANE, variant)
            for _ in range(launches):
                ctx.eval_device(n, xd.data_ptr(), out[variant].data_ptr(), st.data_ptr(), stream)
            torch.cuda.synchronize()
            total_ms, count, _ = ctx.kernel_time_log()
            assert count == launches
            return total_ms / launches

        for v in (0, 1):
            run(v, 10)  # warm-up: code objects loaded, clocks up
        per_round = {0: [], 1: []}
        for _ in range(a.rounds):
            for v in (0, 1):
                per_round[v].append(run(v, a.launches))
        same = bool(np.array_equal(out[0].cpu().numpy().view(np.uint64), out[1].cpu().numpy().view(np.uint64)))
        for v, name in ((0, "wavefront_per_evaluation"), (1, "one_lane_per_evaluation")):
            ms = np.array(per_round[v])
            lines.append(dict(what="ccm_kernel_ms", measured_on="MI355X", kernel=name, frames=a.frames, n=n,
                              rounds=a.rounds, launches_per_round=a.launches, median_ms=float(np.median(ms)),
                              min_ms=float(ms.min()), max_ms=float(ms.max()),
                              us_per_evaluation=float(np.median(ms)) * 1e3 / n, bit_identical_variants=same))
    ctx.close()
    text = "".join(json.dumps(line) + "\n" for line in lines)
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
