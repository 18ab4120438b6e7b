#!/usr/bin/env python3
"""Regenerate the fixtures of the cell_cycle_marker tests under tests/golden/:

  ccm_tracks.tsv       3 synthetic tracks x 130 frames, drawn from the model itself (fixed parameters
                       plus Student-t(4) noise of the model's own scale); two frames NA, one nan, one
                       line ending in CRLF
  ccm_prior.xml        10 uniform variables, the noise parameters bounded away from 0
  ccm_likelihood.xml   type cell_cycle_marker on ccm_tracks.tsv
  ccm_golden.npz       x [64, 10] drawn inside the prior, tracks [3, 130] as the file reads, and
                       logp [3, 64] from the numpy restatement tests/ccm_reference.py

Deterministic (seeded); needs numpy only. Usage: python tools/make_ccm_fixtures.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ccm_reference as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FRAMES, NDRAWS = 130, 64
NAMES = ["S_entry_time", "S_duration", "plateau_duration", "base_signal", "S_signal_increase",
         "plateau_signal_increase", "mitosis_signal_fraction", "mitosis_signal_decrease", "additive_noise",
         "proportional_noise"]
# the parameters each track is drawn from
TRUTH = [
    [20.0, 40.0, 45.0, 6.0, 1.5, 0.3, 0.3, 0.2, 0.5, 0.02],
    [12.0, 55.0, 30.0, 4.0, 1.1, 0.15, 0.4, 0.35, 0.3, 0.03],
    [33.0, 35.0, 70.0, 9.0, 2.2, 0.5, 0.25, 0.1, 0.8, 0.015],
]
# (track, frame) -> the token written instead of a number
MISSING = {(0, 17): "NA", (1, 64): "nan", (2, 129): "NA"}
CRLF_LINE = 2  # the file's third line (track 1) ends in \r\n


def signal(v, frames):
    """the model's x_i, as tests/ccm_reference.py computes it"""
    s_entry, s_dur, p_dur, base, s_inc, p_inc, m_frac, m_dec = v[:8]
    plateau, mitosis = s_entry + s_dur, s_entry + s_dur + p_dur
    x = np.full(frames, base)
    for i in range(frames):
        if i > mitosis:
            x[i] += (s_dur * s_inc + p_dur * p_inc) * m_frac - m_dec * (i - mitosis)
        elif i > plateau:
            x[i] += s_dur * s_inc + (i - plateau) * p_inc
        elif i > s_entry:
            x[i] += s_inc * (i - s_entry)
    return x


def main():
    rng = np.random.default_rng(20261020)
    lines = ["track\t" + "\t".join(f"t{i}" for i in range(FRAMES))]
    for k, v in enumerate(TRUTH):
        x = signal(v, FRAMES)
        y = x + (v[8] + v[9] * np.maximum(x, 0.0)) * rng.standard_t(4, FRAMES)
        tokens = [MISSING.get((k, i), f"{y[i]:.2f}") for i in range(FRAMES)]
        lines.append(f"cell{k + 1}\t" + "\t".join(tokens))
    with open(os.path.join(GOLDEN, "ccm_tracks.tsv"), "w", newline="") as f:
        for n, line in enumerate(lines):
            f.write(line + ("\r\n" if n == CRLF_LINE else "\n"))

    with open(os.path.join(GOLDEN, "ccm_prior.xml"), "w") as f:
        f.write('<?xml version="1.0" encoding="utf-8"?>\n<variableset>\n')
        for name, lo, hi in zip(NAMES, R.PRIOR_LOWER, R.PRIOR_UPPER):
            f.write(f'  <variable name="{name}" distribution="uniform" lower="{lo:g}" upper="{hi:g}"/>\n')
        f.write("</variableset>\n")
    with open(os.path.join(GOLDEN, "ccm_likelihood.xml"), "w") as f:
        f.write('<?xml version="1.0" encoding="utf-8"?>\n<bcm_likelihood type="cell_cycle_marker" data_file="ccm_tracks.tsv"/>\n')

    # the tracks as the file reads: the written tokens, NA / nan as NaN
    tracks = np.array([[float("nan") if t in ("NA", "nan") else float(t) for t in line.split("\t")[1:]]
                       for line in lines[1:]])
    x = R.draws(NDRAWS, 7)
    logp = np.array([R.logp(x, t) for t in tracks])
    assert np.all(np.isfinite(logp))
    np.savez(os.path.join(GOLDEN, "ccm_golden.npz"), x=x, tracks=tracks, logp=logp)
    print("tracks", tracks.shape, "NaN frames", int(np.isnan(tracks).sum()), "logp range", logp.min(), logp.max())


if __name__ == "__main__":
    main()
