#!/usr/bin/env python3
"""Times of the cell_cycle_marker predictive checks on the GPU (DESIGN.md §4 "predictive checks of the
cell cycle marker"): bcm3_amd.predict.measurements(loo=True) and posterior_predictive on a synthetic track
of 240 frames (the track of tools/ccm_kernel_timing.py), at 256 and 8192 draws, the grid at 240 and 4096
frames.

Every figure is a HIP-event time of the library (the *_last_ms accessors): the predict kernel, the
quantile launches, the WAIC kernel, the PSIS-LOO kernel, the whole call from the upload of the draws to
the last copy back, and the chain kernel's own launch inside the call. Each case is warmed up, then run
in rounds; the median, minimum and maximum over the rounds are printed, one JSON line per case; --out
appends them to a file. Usage: python tools/ccm_predict_timing.py [--out FILE] [--rounds 9] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def synthetic_track(frames: int) -> np.ndarray:
    """a track drawn from the model: S entry at 40, mitosis at 200, t(4) noise of the model's scale"""
    rng = np.random.default_rng(1)
    clean = np.empty(frames)
    for i in range(frames):
        x = 6.0
        if i > 200.0:
            x += (90.0 * 1.2 + 70.0 * 0.2) * 0.3 - 0.2 * (i - 200.0)
        elif i > 130.0:
            x += 90.0 * 1.2 + (i - 130.0) * 0.2
        elif i > 40.0:
            x += 1.2 * (i - 40.0)
        clean[i] = x
    track = clean + (0.5 + 0.02 * clean) * rng.standard_t(4, frames)
    track[[17, frames // 2]] = np.nan
    return track


def summary(rows):
    a = np.array(rows, dtype=np.float64)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 8192])
    ap.add_argument("--grids", type=int, nargs="+", default=[240, 4096])
    a = ap.parse_args()

    import torch
    import ccm_reference as R
    from bcm3_amd import _hip, predict
    assert torch.cuda.is_available(), "needs a GPU"

    ctx = _hip.Context.cell_cycle_marker(synthetic_track(a.frames))
    probs = (0.05, 0.5, 0.95)
    lines = []
    for n in a.sizes:
        x = R.draws(n, 5)
        names = ("predict_kernel_ms", "quantile_ms", "waic_ms", "total_ms", "loo_ms", "chain_kernel_ms")
        cols = {k: [] for k in names}
        for r in range(a.warmup + a.rounds):
            predict.measurements(ctx, x, probs, seed=r, loo=True)
            ms = ctx.ccm_predict_last_ms("obs") + ctx.ccm_predict_last_ms("loo")
            if r >= a.warmup:
                for k, v in zip(names, ms):
                    cols[k].append(v)
        # the ordinary launch of the same batch, by its own event pair (after the LOO call it is no longer the last)
        for r in range(a.warmup + a.rounds):
            ctx.eval(x)
            if r >= a.warmup:
                cols["chain_kernel_ms"].append(ctx.last_kernel_ms())
        line = dict(what="ccm_predict_ms", measured_on="MI355X", call="measurements(loo=True)", frames=a.frames, n=n,
                    rounds=a.rounds, warmup=a.warmup)
        line.update({k: summary(v) for k, v in cols.items()})
        lines.append(line)
        for G in a.grids:
            names = ("predict_kernel_ms", "quantile_ms", "total_ms")
            cols = {k: [] for k in names}
            for r in range(a.warmup + a.rounds):
                predict.posterior_predictive(ctx, x, probs, frames=G)
                if r >= a.warmup:
                    for k, v in zip(names, ctx.ccm_predict_last_ms("grid")):
                        cols[k].append(v)
            line = dict(what="ccm_predict_ms", measured_on="MI355X", call="posterior_predictive(frames=G)",
                        frames=a.frames, G=G, n=n, rounds=a.rounds, warmup=a.warmup)
            line.update({k: summary(v) for k, v in cols.items()})
            lines.append(line)
    ctx.close()
    text = "".join(json.dumps(line) + "\n" for line in lines)
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
