#!/usr/bin/env python3
"""What TBX_QUERY_LOOKAHEAD_SAMPLES costs (include/toybox_amd.h): leaf-frames/s per game at 4 096 envs x 64 samples x 64 frames,
hold = 4, rest drawn, salt 0, agent layer off, one process.  A leaf-frame is one frame of one played future: a call plays
N x n_legal x samples x frames of them (an upper count where a game ends early).

Two arms, interleaved on one box:
  fused     one tbx_reduce_device(TBX_QUERY_LOOKAHEAD_SAMPLES) call;
  composed  what the engine offered before for the salt-0 half: `samples` tbx_reduce_device(TBX_QUERY_LOOKAHEAD_ALL) calls under
            sample_seed(seed, s), each into its own slice of one device array, then the eight fields summed over the samples on
            the device (torch, on the same stream).
Both play the same leaves; the rows of both arms are compared once (they must be equal) before anything is timed.  Every arm is
timed with events on one stream in REGIONS interleaved regions after one warm-up; median (min - max).

    python scripts/sample_rate.py [--out profiles/samples.md]

Needs a GPU; prints the markdown it writes and keeps the file from "## Launch budget" on, which is written by hand."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fork_rate import make  # noqa: E402
from toybox_amd import _abi  # noqa: E402
from toybox_amd.engine import lookahead_args, sample_args, sample_seed  # noqa: E402

REGIONS = 5
KEEP = "## Launch budget"
GAMES, N, SAMPLES, FRAMES, HOLD, SEED = ("breakout", "space_invaders", "amidar", "gridworld"), 4096, 64, 64, 4, 77


def measure(game, torch):
    e = make(game, N, "raw")
    for t in range(16, 400):                                 # mid-game states
        e.step_synthetic(1337, t, auto_reset=True)
    e.sync()
    L = len(e.legal_actions)
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    fused_out = torch.empty((N, L, 8), dtype=torch.float64, device="cuda")
    leaves = torch.empty((SAMPLES, N, L, 5), dtype=torch.float64, device="cuda")
    composed_out = torch.empty((N, L, 8), dtype=torch.float64, device="cuda")
    fused_args = sample_args(game, N, FRAMES, SAMPLES, hold=HOLD, seed=SEED)[0]
    all_args = [lookahead_args(N, FRAMES, hold=HOLD, seed=sample_seed(SEED, k))[0] for k in range(SAMPLES)]

    def fused():
        e.reduce_device(_abi.QUERY_LOOKAHEAD_SAMPLES, fused_out.data_ptr(), fused_args, stream=s)

    def composed():
        for k in range(SAMPLES):
            e.reduce_device(_abi.QUERY_LOOKAHEAD_ALL, leaves[k].data_ptr(), all_args[k], stream=s)
        with torch.cuda.stream(ts):
            ret, lives, run, lost_at = leaves[..., 0], leaves[..., 2], leaves[..., 3], leaves[..., 4]
            composed_out[..., 0] = float(SAMPLES)
            composed_out[..., 1] = ret.sum(0)
            composed_out[..., 2] = ret.amin(0)
            composed_out[..., 3] = ret.amax(0)
            composed_out[..., 4] = lives.sum(0)
            composed_out[..., 5] = (lost_at >= 0).sum(0)
            composed_out[..., 6] = (lives <= 0).sum(0)
            composed_out[..., 7] = torch.where(lost_at < 0, run, lost_at).sum(0)

    def region_ms(body):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ts)
        body()
        b.record(ts)
        b.synchronize()
        return a.elapsed_time(b)

    try:
        bodies = {"fused": fused, "composed": composed}
        for body in bodies.values():                         # warm-ups, and the rows of both arms against one another
            region_ms(body)
        chunks = e.sample_chunks
        if not torch.equal(fused_out, composed_out):
            raise SystemExit("%s: the fused rows and the summed TBX_QUERY_LOOKAHEAD_ALL rows differ" % game)
        arms = {k: [] for k in bodies}
        for _ in range(REGIONS):
            for k, body in bodies.items():
                arms[k].append(region_ms(body))
    finally:
        ts.synchronize()
        e.sync()
    box = e.device_identity()
    e.close()
    return {k: np.asarray(v) for k, v in arms.items()}, chunks, L, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "samples.md"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sample_rate.py measures on a GPU; none found")
    rows, box = [], None
    for game in GAMES:
        arms, chunks, L, box = measure(game, torch)
        f, c = arms["fused"], arms["composed"]
        leaf_frames = N * L * SAMPLES * FRAMES
        rows.append("| %s | %d | %d | %.2f (%.2f - %.2f) | %.1f | %.2f (%.2f - %.2f) | %.1f | %.3f | %.1f %% / %.1f %% |" % (
            game, L, chunks, np.median(f), f.min(), f.max(), leaf_frames / np.median(f) / 1e3, np.median(c), c.min(), c.max(), leaf_frames / np.median(c) / 1e3,
            np.median(c) / np.median(f), 100.0 * (f.max() - f.min()) / np.median(f), 100.0 * (c.max() - c.min()) / np.median(c)))
        print(rows[-1], flush=True)
    lines = ["# Sampled lookahead rate (scripts/sample_rate.py)", "",
             "Box: %s (%s, %d CUs), one process, agent layer off, %d envs x %d samples x %d frames, hold = %d, rest drawn, salt 0.  ms per call as "
             "the median (min - max) of %d interleaved regions after one warm-up, events on one stream.  A leaf-frame is one frame of one played "
             "future; a call counts N x n_legal x samples x frames of them.  fused: one TBX_QUERY_LOOKAHEAD_SAMPLES call.  composed: %d "
             "TBX_QUERY_LOOKAHEAD_ALL calls under sample_seed(seed, s) and the sum over the samples on the device (torch); its rows equalled the "
             "fused rows on every game before the timing." % (
                 box["name"] or "device %d at %s" % (box["ordinal"], box["pci"]), box["arch"], box["compute_units"], N, SAMPLES, FRAMES, HOLD, REGIONS, SAMPLES), "",
             "| game | n_legal | chunks | fused ms | fused M leaf-frames/s | composed ms | composed M leaf-frames/s | composed / fused | spread (max - min) / median, fused / composed |",
             "|---|---|---|---|---|---|---|---|---|"] + rows
    if os.path.exists(args.out):
        old = open(args.out).read()
        if KEEP in old:
            lines += ["", old[old.index(KEEP):].rstrip()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
