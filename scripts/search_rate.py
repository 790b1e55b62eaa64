#!/usr/bin/env python3
"""What TBX_QUERY_LOOKAHEAD_SEARCH costs (include/toybox_amd.h): leaf-frames/s per game at 4 096 envs, frames = 64, hold = 4,
depth 1, 2 and 3, agent layer off, one process.  A leaf-frame is one frame of one played plan: a call plays
N x n_legal^depth x frames of them (an upper count where a game ends early).

Two comparisons:
  (a) TBX_QUERY_LOOKAHEAD_ALL at the same frames and hold on the same engine.  The depth-1 search runs the same step bodies; what it
      adds is the reload and the compare.  Reported: search(depth 1) / ALL as a ratio, beside ALL's own run-to-run spread.
  (b) depth 2 only, reported and not gated: the composition the engine offered before -- one TBX_EDIT_CHECKPOINT_SAVE, then per leaf
      a TBX_EDIT_CHECKPOINT_RESTORE, `frames` tbx_step_device launches with the plan's constant action rows and a device-side copy
      of the score and lives outputs -- all device forms on one caller's stream.

Every arm is timed with HIP events on the caller's stream in REGIONS interleaved regions after one warm-up; median (min - max).
The depth-1 search is measured first; a deeper configuration whose time, estimated from that rate, exceeds MAX_SECONDS is not run.

    python scripts/search_rate.py [--out profiles/search.md]

Needs a GPU; prints the markdown it writes and keeps the file from "## Launch budget" on, which is written by hand (the budget
derived from the slowest game's rate, the compiler's resource remarks)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fork_rate import make  # noqa: E402
from toybox_amd import _abi, hip  # noqa: E402

REGIONS = 5
KEEP = "## Launch budget"
GAMES, N, FRAMES, HOLD, DEPTHS = ("breakout", "space_invaders", "amidar", "gridworld"), 4096, 64, 4, (1, 2, 3)
MAX_SECONDS = 3.0


def region_ms(stream, body):
    a, b = hip.Event(), hip.Event()
    a.record(stream)
    body()
    b.record(stream)
    b.synchronize()
    return a.elapsed_ms(b)


def measure(game):
    e = make(game, N, "raw")
    for t in range(16, 400):                                 # mid-game states
        e.step_synthetic(1337, t, auto_reset=True)
    e.checkpoint_slots(1)
    legal = e.legal_actions
    L = len(legal)
    s = hip.Stream()
    rows = [hip.malloc(4 * N) for _ in legal]
    for p, a in zip(rows, legal):
        hip.memcpy_htod(p, np.full(N, a, np.int32), 4 * N)
    aside = hip.malloc(8 * N)
    out = hip.malloc(8 * 6 * N * L)
    arms = {}
    try:
        def search(depth):
            return lambda: e.reduce_device(_abi.QUERY_LOOKAHEAD_SEARCH, out, [FRAMES, HOLD, depth, 0, legal[0]], stream=s.ptr)

        def all_actions():
            e.reduce_device(_abi.QUERY_LOOKAHEAD_ALL, out, [FRAMES, HOLD, -1, legal[0]], stream=s.ptr)

        def composition():                                   # depth 2: every (first, second) pair, then the rest action
            e.edit_device(_abi.EDIT_CHECKPOINT_SAVE, [0], stream=s.ptr)
            for first in rows:
                for second in rows:
                    e.edit_device(_abi.EDIT_CHECKPOINT_RESTORE, [0], stream=s.ptr)
                    for j in range(FRAMES):
                        e.step_device(first if j < HOLD else second if j < 2 * HOLD else rows[0], auto_reset=False, stream=s.ptr)
                    for k, which in enumerate((_abi.BUF_SCORE, _abi.BUF_LIVES)):
                        src, nbytes = e.device_buffer(which)
                        hip.memcpy_dtod_async(aside + 4 * N * k, src, nbytes, s)
            e.edit_device(_abi.EDIT_CHECKPOINT_RESTORE, [0], stream=s.ptr)

        bodies = {"all": all_actions, "search1": search(1)}
        region_ms(s, bodies["search1"])
        est = region_ms(s, bodies["search1"]) / 1e3           # seconds per N x L x frames leaf-frames
        skipped = []
        for depth in DEPTHS[1:]:
            if est * L ** (depth - 1) <= MAX_SECONDS:
                bodies["search%d" % depth] = search(depth)
            else:
                skipped.append(depth)
        bodies["composition"] = composition
        for body in bodies.values():                         # warm-ups
            region_ms(s, body)
        arms = {k: [] for k in bodies}
        for _ in range(REGIONS):
            for k, body in bodies.items():
                arms[k].append(region_ms(s, body))
        chunks = {}
        for depth in DEPTHS:
            if "search%d" % depth in bodies:
                bodies["search%d" % depth]()
                chunks[depth] = e.get_option(_abi.OPT_SEARCH_CHUNKS)
    finally:
        s.synchronize()
        e.sync()
        for p in rows + [aside, out]:
            hip.free(p)
        s.close()
    box = e.device_identity()
    e.close()
    return {k: np.asarray(v) for k, v in arms.items()}, skipped, chunks, L, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search.md"))
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("search_rate.py measures on a GPU; none found")
    rate_rows, ratio_rows, comp_rows, slowest, box = [], [], [], None, None
    for game in GAMES:
        arms, skipped, chunks, L, box = measure(game)
        for depth in DEPTHS:
            k = "search%d" % depth
            if k not in arms:
                rate_rows.append("| %s | %d | %d | not run: estimated above %.0f s | | |" % (game, depth, L ** depth, MAX_SECONDS))
                continue
            t = arms[k]
            med = float(np.median(t))
            rate = N * L ** depth * FRAMES / med * 1e3
            slowest = rate if slowest is None else min(slowest, rate)
            rate_rows.append("| %s | %d | %d | %d | %.3f (%.3f - %.3f) | %.1f |" % (game, depth, L ** depth, chunks[depth], med, t.min(), t.max(), rate / 1e6))
            print(rate_rows[-1], flush=True)
        a, s1 = arms["all"], arms["search1"]
        ratio_rows.append("| %s | %.3f (%.3f - %.3f) | %.1f %% | %.3f (%.3f - %.3f) | %.3f |" % (
            game, np.median(a), a.min(), a.max(), 100.0 * (a.max() - a.min()) / np.median(a), np.median(s1), s1.min(), s1.max(), np.median(s1) / np.median(a)))
        print(ratio_rows[-1], flush=True)
        if "search2" in arms:
            c, s2 = arms["composition"], arms["search2"]
            comp_rows.append("| %s | %.2f (%.2f - %.2f) | %.3f (%.3f - %.3f) | %.1f |" % (game, np.median(c), c.min(), c.max(), np.median(s2), s2.min(), s2.max(),
                                                                                    np.median(c) / np.median(s2)))
            print(comp_rows[-1], flush=True)
    lines = ["# Search rate (scripts/search_rate.py)", "",
             "Box: %s (%s, %d CUs), one process, agent layer off, %d envs, frames = %d, hold = %d, rest = the first legal action, objective 0.  ms per "
             "call as the median (min - max) of %d interleaved regions after one warm-up, HIP events on the caller's stream.  A leaf-frame is one "
             "frame of one played plan; a call counts N x n_legal^depth x frames of them." % (
                 box["name"] or "device %d at %s" % (box["ordinal"], box["pci"]), box["arch"], box["compute_units"], N, FRAMES, HOLD, REGIONS), "",
             "| game | depth | plans per env | chunks | ms per call | M leaf-frames/s |", "|---|---|---|---|---|---|"] + rate_rows
    lines += ["", "Slowest measured rate: %.1f M leaf-frames/s; half a second of it is %.2e leaf-frames." % (slowest / 1e6, slowest / 2), "",
              "## (a) depth-1 search against TBX_QUERY_LOOKAHEAD_ALL, same frames and hold", "",
              "| game | ALL ms | ALL spread (max - min) / median | search depth 1 ms | search / ALL |", "|---|---|---|---|---|"] + ratio_rows
    lines += ["", "## (b) depth 2 against the checkpoint / restore / step composition (reported, not gated)", "",
              "| game | composition ms | search depth 2 ms | composition / search |", "|---|---|---|---|"] + comp_rows
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
