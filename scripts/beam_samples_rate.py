#!/usr/bin/env python3
"""What TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES costs (include/toybox_amd.h) at 4 096 envs, frames = 64, hold = 4, depth =
TBX_PLAN_MAX_DEPTH(game), width 4, 16 samples, rest = -1, agent layer off, one process, one call per game.

Two arms, interleaved in the same session, both host forms timed on the wall clock from the call to the rows on the host:
  (a) the query (salt 0 here, as arm (b) cannot salt a plan's game RNG; the salted query, salt 1, is timed beside it);
  (b) the same beam driven from the host with what the engine offered before: per level one TBX_QUERY_LOOKAHEAD_PLAN call per
      candidate column (first action, slot, digit) and sample under sample_seed(seed, s) with per-env code rows, the rows read back,
      summed with numpy integers, the kept set chosen by a numpy lexsort.
The two arms must return identical rows (asserted).  ms per call as the median (min - max) of REGIONS interleaved regions after one
warm-up of each arm.  No ratio is gated: nobody had measured either arm before this script.

Reported beside it: the time of ONE level launch at the budgeted range size -- a depth-1 query (one play launch and its select) of
64 samples x 1 024 frames on as many envs as tbx_search_samples_budget(game) leaf-frames allow, the device form between HIP events
on a caller's stream -- against the 0.25 s that budget was derived for.

    python scripts/beam_samples_rate.py [--out profiles/beam_samples.md]

Needs a GPU; prints the markdown it writes and keeps the file from "## Kernel resources" on, which is written by hand."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fork_rate import make  # noqa: E402
from toybox_amd import _abi, hip  # noqa: E402
from toybox_amd.engine import SAMPLE_FIELDS, plan_args, sample_seed  # noqa: E402
from search_rate import region_ms  # noqa: E402

REGIONS = 3
EVENT_REGIONS = 3
KEEP = "## Kernel resources"
GAMES, N, FRAMES, HOLD, WIDTH, SAMPLES, SEED = ("breakout", "space_invaders", "amidar", "gridworld"), 4096, 64, 4, 4, 16, 77
# tbx_search_samples_budget (toybox_amd/csrc/tbx_common.hpp), leaf-frames per level launch; Breakout: its thread form
BUDGET = {"breakout": 1 << 32, "space_invaders": 1 << 29, "amidar": 1 << 27, "gridworld": 1 << 30}
LEVEL_SAMPLES, LEVEL_FRAMES = 64, 1024
ROW_FIELDS = SAMPLE_FIELDS + ("code",)


def host_beam(e, game, depth):
    """arm (b): the beam of include/toybox_amd.h out of TBX_QUERY_LOOKAHEAD_PLAN calls and numpy; the query's nine fields [N, L]"""
    L = len(e.legal_actions)
    seeds = [sample_seed(SEED, s) for s in range(SAMPLES)]
    kept = np.tile(np.arange(L, dtype=np.int64)[None, :, None], (N, 1, 1))
    for d in range(1, depth + 1):
        cand = kept if d == 1 else (kept[..., None] + np.arange(L, dtype=np.int64) * L ** (d - 1)).reshape(N, L, -1)
        J = cand.shape[2]
        rows = np.empty((SAMPLES, N, L, J, 5), np.int64)
        for a in range(L):
            for j in range(J):
                for s in range(SAMPLES):
                    args, _ = plan_args(game, N, FRAMES, hold=HOLD, depth=d, code=cand[:, a, j], rest=None, seed=seeds[s])
                    rows[s, :, a, j] = e.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args)
        ret, lives, run, lost_at = rows[..., 0], rows[..., 2], rows[..., 3], rows[..., 4]
        sums = dict(samples=np.full((N, L, J), SAMPLES, np.int64), ret_sum=ret.sum(0), ret_min=ret.min(0), ret_max=ret.max(0), lives_sum=lives.sum(0),
                    lost=(lost_at >= 0).sum(0), ended=(lives <= 0).sum(0), safe_frames_sum=np.where(lost_at < 0, run, lost_at).sum(0))
        # objective 0: the larger ret_sum, the smaller lost, the larger safe_frames_sum, the smaller code (the last key is the primary one)
        order = np.lexsort((cand, -sums["safe_frames_sum"], sums["lost"], -sums["ret_sum"]), axis=2)
        kept = np.take_along_axis(cand, order[..., :min(WIDTH, J)], axis=2)
    out = {k: np.take_along_axis(v, order[..., :1], axis=2)[..., 0] for k, v in sums.items()}
    out["code"] = kept[..., 0]
    return out


def wall_ms(body):
    t0 = time.perf_counter()
    out = body()
    return (time.perf_counter() - t0) * 1e3, out


def mid_game(game, n):
    e = make(game, n, "raw")
    for t in range(16, 400):                                 # mid-game states
        e.step_synthetic(1337, t, auto_reset=True)
    e.sync()
    return e


def measure(game):
    e = mid_game(game, N)
    L, top = len(e.legal_actions), _abi.PLAN_MAX_DEPTH[game]

    def query(salt=0):
        return e.lookahead_beam_samples(FRAMES, top, WIDTH, SAMPLES, hold=HOLD, salt=salt, seed=SEED)

    def composed():
        return host_beam(e, game, top)

    a, b = wall_ms(query)[1], wall_ms(composed)[1]           # one warm-up of each arm, and the two arms agree
    for k in ROW_FIELDS:
        assert np.array_equal(np.asarray(a[k], np.int64), np.asarray(b[k], np.int64)), "%s: the arms differ in %s" % (game, k)
    ta, tb, tsalt = [], [], []
    for _ in range(REGIONS):
        ta.append(wall_ms(query)[0])
        tb.append(wall_ms(composed)[0])
        tsalt.append(wall_ms(lambda: query(1))[0])
        print(game, ta[-1], tb[-1], tsalt[-1], flush=True)
    ranges, chunks = e.beam_samples_ranges, e.beam_samples_chunks
    box = e.device_identity()
    e.close()
    # one level launch at the budgeted range size
    envs = BUDGET[game] // (L * LEVEL_SAMPLES * LEVEL_FRAMES)
    e = mid_game(game, envs)
    s = hip.Stream()
    out = hip.malloc(8 * 9 * envs * L)
    tl = []
    try:
        def body():
            e.reduce_device(_abi.QUERY_LOOKAHEAD_BEAM_SAMPLES, out, [LEVEL_FRAMES, HOLD, 1, 0, -1, SEED, 0, 0, 0, 1, LEVEL_SAMPLES, 1], stream=s.ptr)
        region_ms(s, body)                                   # warm-up
        for _ in range(EVENT_REGIONS):
            tl.append(region_ms(s, body))
        assert e.beam_samples_ranges == 1
    finally:
        s.synchronize()
        e.sync()
        hip.free(out)
        s.close()
    e.close()
    return np.asarray(ta), np.asarray(tb), np.asarray(tsalt), ranges, chunks, envs, np.asarray(tl), L, top, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_samples.md"))
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("beam_samples_rate.py measures on a GPU; none found")
    arm_rows, level_rows, box = [], [], None
    for game in GAMES:
        ta, tb, tsalt, ranges, chunks, envs, tl, L, top, box = measure(game)
        arm_rows.append("| %s | %d | %d | %d | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.0f (%.0f - %.0f) | %.1f |" % (
            game, top, ranges, chunks, np.median(ta), ta.min(), ta.max(), np.median(tsalt), tsalt.min(), tsalt.max(), np.median(tb), tb.min(), tb.max(),
            float(np.median(tb) / np.median(ta))))
        level_rows.append("| %s | 2^%d | %d | %.1f (%.1f - %.1f) | %s |" % (game, BUDGET[game].bit_length() - 1, envs, np.median(tl), tl.min(), tl.max(),
                                                                        "above 250 ms" if np.median(tl) > 250.0 else "within 250 ms"))
    lines = ["# Beam search over sampled futures (scripts/beam_samples_rate.py)", "",
             "Box: %s (%s, %d CUs), one process, agent layer off, %d envs, frames = %d, hold = %d, depth = TBX_PLAN_MAX_DEPTH(game), width %d, %d samples, "
             "rest = -1, seed %d, objective 0.  Both arms are host forms timed on the wall clock from the call to the rows on the host: ms per call as "
             "the median (min - max) of %d interleaved regions after one warm-up of each arm.  Arm (a) is TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES with salt 0 "
             "(and, beside it, with salt 1); arm (b) drives the same beam from the host, per level one TBX_QUERY_LOOKAHEAD_PLAN call per candidate "
             "column and sample with per-env code rows, numpy sums and the kept set by a numpy lexsort -- salt 0 in both arms, since a plan call "
             "cannot salt the game RNG.  The arms returned identical rows (asserted).  No ratio is gated." % (
                 box["name"] or "device %d at %s" % (box["ordinal"], box["pci"]), box["arch"], box["compute_units"], N, FRAMES, HOLD, WIDTH, SAMPLES, SEED, REGIONS), "",
             "| game | depth | env ranges | most sample chunks | (a) query ms | (a) salted ms | (b) host-driven ms | (b) / (a) |", "|---|---|---|---|---|---|---|---|"] + arm_rows
    lines += ["", "## One level launch at the budgeted range size", "",
              "A depth-1 query (one play launch, one select) of %d samples x %d frames, hold %d, salt 1, on as many envs as the game's "
              "tbx_search_samples_budget leaf-frames allow: the device form between HIP events on a caller's stream, the median (min - max) of %d "
              "regions after one warm-up, against the 0.25 s the budgets were derived for (profiles/search_samples.md).  Breakout is its thread form; "
              "Breakout's wave forms (custom bricks, TBX_OPT_STEP_FORM = 2) have no measured rate behind their budget of 2^27, here as there." % (
                  LEVEL_SAMPLES, LEVEL_FRAMES, HOLD, EVENT_REGIONS), "",
              "| game | budget (leaf-frames) | envs | ms per level launch | against 0.25 s |", "|---|---|---|---|---|"] + level_rows
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
