#!/usr/bin/env python3
"""What TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES costs (include/toybox_amd.h): ms per call and leaf-frames/s per game at 4 096 envs x
64 frames, hold = 4, depth 2, 16 samples, rest drawn, salt 0, agent layer off, one process.  A leaf-frame is one frame of one played
future: a call plays N x n_legal^depth x samples x frames of them (an upper count where a game ends early; the fused query replays
its winners once more, which is not counted).

Two arms, interleaved on one box:
  fused     one tbx_reduce_device(TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES) call;
  composed  what the engine offered before, possible for salt 0 only: n_legal^depth x samples tbx_reduce_device(
            TBX_QUERY_LOOKAHEAD_PLAN) calls, one per (code, sample) under sample_seed(seed, s), each into its own slice of one
            device array, then the eight sums per plan and the pick per first action on the device (torch, on the same stream).
Both play the same leaves; the rows of both arms are compared once (they must be equal) before anything is timed.  Every arm is
timed with events on one stream in REGIONS interleaved regions after one warm-up; median (min - max).  No ratio is fixed in advance:
a game where the fused query loses is reported as such.

    python scripts/search_samples_rate.py [--out profiles/search_samples.md] [--games breakout,gridworld]

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
from toybox_amd.engine import plan_args, sample_seed, search_samples_args  # noqa: E402

REGIONS = 5
KEEP = "## Launch budget"
GAMES, N, FRAMES, HOLD, DEPTH, SAMPLES, SEED = ("breakout", "space_invaders", "amidar", "gridworld"), 4096, 64, 4, 2, 16, 77


def measure(game, torch):
    e = make(game, N, "raw")
    for t in range(16, 400):                                 # mid-game states
        e.step_synthetic(1337, t, auto_reset=True)
    e.sync()
    L = len(e.legal_actions)
    codes = L ** DEPTH
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    fused_out = torch.empty((N, L, 9), dtype=torch.float64, device="cuda")
    leaves = torch.empty((SAMPLES, codes, N, 5), dtype=torch.float64, device="cuda")
    composed_out = torch.empty((N, L, 9), dtype=torch.float64, device="cuda")
    fused_args = search_samples_args(game, N, FRAMES, DEPTH, SAMPLES, hold=HOLD, objective=0, seed=SEED)[0]
    call_args = [[plan_args(game, N, FRAMES, hold=HOLD, depth=DEPTH, code=c, seed=sample_seed(SEED, k))[0] for c in range(codes)] for k in range(SAMPLES)]
    index = torch.arange(codes, device="cuda")
    group = [index[index % L == a] for a in range(L)]

    def fused():
        e.reduce_device(_abi.QUERY_LOOKAHEAD_SEARCH_SAMPLES, fused_out.data_ptr(), fused_args, stream=s)

    def composed():
        for k in range(SAMPLES):
            for c in range(codes):
                e.reduce_device(_abi.QUERY_LOOKAHEAD_PLAN, leaves[k, c].data_ptr(), call_args[k][c], stream=s)
        with torch.cuda.stream(ts):
            ret, lives, run, lost_at = (leaves[..., i].to(torch.int64) for i in (0, 2, 3, 4))            # [S, codes, N]
            sums = torch.stack([torch.full_like(ret[0], SAMPLES), ret.sum(0), ret.amin(0), ret.amax(0), lives.sum(0), (lost_at >= 0).sum(0), (lives <= 0).sum(0),
                                torch.where(lost_at < 0, run, lost_at).sum(0)], dim=-1)                  # [codes, N, 8]
            # objective 0: the larger ret_sum, the smaller lost, the larger safe_frames_sum, the smaller code -- one integer key
            key = (sums[..., 1] * (SAMPLES + 1) + (SAMPLES - sums[..., 5])) * (SAMPLES * FRAMES + 1) + sums[..., 7]
            key = key * codes + (codes - 1 - index)[:, None]
            for a in range(L):
                win = group[a][key[group[a]].argmax(0)]                                                  # [N]
                composed_out[:, a, :8] = sums[win, torch.arange(N, device="cuda")].to(torch.float64)
                composed_out[:, a, 8] = win.to(torch.float64)

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
        chunks, launches = e.search_samples_chunks, e.search_samples_launches
        if not torch.equal(fused_out, composed_out):
            raise SystemExit("%s: the fused rows and the rows composed of TBX_QUERY_LOOKAHEAD_PLAN calls differ" % game)
        arms = {k: [] for k in bodies}
        for _ in range(REGIONS):
            for k, body in bodies.items():
                arms[k].append(region_ms(body))
    finally:
        ts.synchronize()
        e.sync()
    box = e.device_identity()
    e.close()
    return {k: np.asarray(v) for k, v in arms.items()}, chunks, launches, L, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_samples.md"))
    ap.add_argument("--games", default=",".join(GAMES))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("search_samples_rate.py measures on a GPU; none found")
    rows, box = [], None
    for game in args.games.split(","):
        arms, chunks, launches, L, box = measure(game, torch)
        f, c = arms["fused"], arms["composed"]
        leaf_frames = N * L ** DEPTH * SAMPLES * FRAMES
        rows.append("| %s | %d | %d | %d | %d | %.2f (%.2f - %.2f) | %.1f | %.2f (%.2f - %.2f) | %.1f | %.3f | %.1f %% / %.1f %% |" % (
            game, L, L ** DEPTH * SAMPLES, chunks, launches, np.median(f), f.min(), f.max(), leaf_frames / np.median(f) / 1e3, np.median(c), c.min(), c.max(),
            leaf_frames / np.median(c) / 1e3, np.median(c) / np.median(f), 100.0 * (f.max() - f.min()) / np.median(f), 100.0 * (c.max() - c.min()) / np.median(c)))
        print(rows[-1], flush=True)
    lines = ["# Search over sampled futures: rate (scripts/search_samples_rate.py)", "",
             "Box: %s (%s, %d CUs), one process, agent layer off, %d envs x %d frames, hold = %d, depth %d, %d samples, objective return, rest drawn, salt 0.  "
             "ms per call as the median (min - max) of %d interleaved regions after one warm-up, events on one stream.  A leaf-frame is one frame of one "
             "played future; a call counts N x n_legal^depth x samples x frames of them.  fused: one TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES call.  composed: "
             "n_legal^depth x samples TBX_QUERY_LOOKAHEAD_PLAN calls under sample_seed(seed, s), the sums and the pick on the device (torch); its rows "
             "equalled the fused rows on every game before the timing." % (
                 box["name"] or "device %d at %s" % (box["ordinal"], box["pci"]), box["arch"], box["compute_units"], N, FRAMES, HOLD, DEPTH, SAMPLES, REGIONS), "",
             "| game | n_legal | plan calls of the composed arm | chunks | launches | fused ms | fused M leaf-frames/s | composed ms | composed M leaf-frames/s | composed / fused | spread (max - min) / median, fused / composed |",
             "|---|---|---|---|---|---|---|---|---|---|---|"] + rows
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
