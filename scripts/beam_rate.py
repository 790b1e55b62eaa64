#!/usr/bin/env python3
"""What TBX_QUERY_LOOKAHEAD_BEAM costs (include/toybox_amd.h) at 4 096 envs, frames = 64, hold = 4, depth = TBX_PLAN_MAX_DEPTH(game),
widths 4 and 16, agent layer off, one process, one call per game and width.

Two arms, interleaved in the same session, both host forms timed on the wall clock from the call to the rows on the host:
  (a) the query;
  (b) the same beam driven from the host with what the engine offered before: per level one TBX_QUERY_LOOKAHEAD_PLAN call per
      (first action, slot, digit) with per-env code rows, the rows read back, the kept set chosen by a numpy lexsort.
The two arms must return identical rows (asserted).  The gate: (a) is not slower than (b) in any game (asserted at the end, after
the file is written).  ms per call as the median (min - max) of REGIONS interleaved regions after one warm-up of each arm.

Reported beside it and not gated: the time per leaf-frame of a full-width beam (width = n_legal^(depth - 2)) and of the exhaustive
search at the deepest depth at which TBX_BEAM_MAX_WIDTH is wide enough, both device forms between HIP events on a caller's stream
in EVENT_REGIONS interleaved regions, as scripts/search_rate.py times its calls; the beam plays about L / (L - 1) times the leaves,
plus the selects.

    python scripts/beam_rate.py [--out profiles/beam.md]

Needs a GPU; prints the markdown it writes and keeps the file from "## Budgets" on, which is written by hand."""
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
from toybox_amd.engine import plan_args  # noqa: E402
from search_rate import region_ms  # noqa: E402

REGIONS = 3
EVENT_REGIONS = 5
KEEP = "## Budgets"
GAMES, N, FRAMES, HOLD, WIDTHS = ("breakout", "space_invaders", "amidar", "gridworld"), 4096, 64, 4, (4, 16)
SEARCH_DEPTH = {"breakout": 6, "space_invaders": 4, "amidar": 4, "gridworld": 5}
FIELDS = ("ret", "score", "lives", "frames_run", "life_lost_at", "code")


def host_beam(e, game, depth, width, objective, rest):
    """arm (b): the beam of include/toybox_amd.h out of TBX_QUERY_LOOKAHEAD_PLAN calls and numpy; the query's six fields [N, L]"""
    L = len(e.legal_actions)
    kept = np.tile(np.arange(L, dtype=np.int64)[None, :, None], (N, 1, 1))
    for d in range(1, depth + 1):
        cand = kept if d == 1 else (kept[..., None] + np.arange(L, dtype=np.int64) * L ** (d - 1)).reshape(N, L, -1)
        J = cand.shape[2]
        rows = np.empty((N, L, J, 5))
        for a in range(L):
            for j in range(J):
                args, _ = plan_args(game, N, FRAMES, hold=HOLD, depth=d, code=cand[:, a, j], rest=rest)
                rows[:, a, j] = e.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args)
        ret, lives, loss = rows[..., 0], rows[..., 2], np.where(rows[..., 4] < 0, _abi.LOOKAHEAD_MAX_FRAMES + 1, rows[..., 4])
        keys = (ret, lives, loss) if objective == 0 else (lives, loss, ret)
        order = np.lexsort((cand,) + tuple(-k for k in reversed(keys)), axis=2)      # the last key is the primary one
        kept = np.take_along_axis(cand, order[..., :min(width, J)], axis=2)
    best = np.take_along_axis(rows, order[..., :1, None], axis=2)[:, :, 0]
    out = {k: best[..., i] for i, k in enumerate(FIELDS[:5])}
    out["code"] = kept[..., 0]
    return out


def wall_ms(body):
    t0 = time.perf_counter()
    out = body()
    return (time.perf_counter() - t0) * 1e3, out


def measure(game):
    e = make(game, N, "raw")
    for t in range(16, 400):                                 # mid-game states
        e.step_synthetic(1337, t, auto_reset=True)
    e.sync()
    L, top, rest = len(e.legal_actions), _abi.PLAN_MAX_DEPTH[game], e.legal_actions[0]
    arms = {}
    for width in WIDTHS:
        def query():
            return e.lookahead_beam(FRAMES, top, width, hold=HOLD, rest=rest)

        def composed():
            return host_beam(e, game, top, width, 0, rest)

        a, b = wall_ms(query)[1], wall_ms(composed)[1]       # one warm-up of each arm, and the two arms agree
        for k in FIELDS:
            assert np.array_equal(np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)), "%s width %d: the arms differ in %s" % (game, width, k)
        ta, tb = [], []
        for _ in range(REGIONS):
            ta.append(wall_ms(query)[0])
            tb.append(wall_ms(composed)[0])
        arms[width] = (np.asarray(ta), np.asarray(tb), e.beam_ranges)
        print(game, width, np.median(ta), np.median(tb), flush=True)
    # per leaf-frame, not gated: a full-width beam against the exhaustive search, device forms on a caller's stream between HIP events,
    # as scripts/search_rate.py times its calls (so the nanoseconds compare with those of profiles/search.md)
    depth = max(d for d in range(2, SEARCH_DEPTH[game] + 1) if L ** (d - 2) <= _abi.BEAM_MAX_WIDTH)
    full = L ** (depth - 2)
    s = hip.Stream()
    out = hip.malloc(8 * 6 * N * L)
    tq, ts = [], []
    try:
        bodies = (lambda: e.reduce_device(_abi.QUERY_LOOKAHEAD_BEAM, out, [FRAMES, HOLD, depth, 0, rest, 0, 0, 0, 0, full], stream=s.ptr),
                  lambda: e.reduce_device(_abi.QUERY_LOOKAHEAD_SEARCH, out, [FRAMES, HOLD, depth, 0, rest], stream=s.ptr))
        for body in bodies:                                  # warm-ups
            region_ms(s, body)
        for _ in range(EVENT_REGIONS):
            tq.append(region_ms(s, bodies[0]))
            ts.append(region_ms(s, bodies[1]))
    finally:
        s.synchronize()
        e.sync()
        hip.free(out)
        s.close()
    leaves = (sum(L ** d for d in range(1, depth + 1)), L ** depth)          # per env: every level's candidates; the plans
    box = e.device_identity()
    e.close()
    return arms, (depth, full, np.asarray(tq), np.asarray(ts), leaves), L, top, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam.md"))
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("beam_rate.py measures on a GPU; none found")
    arm_rows, leaf_rows, slower, box = [], [], [], None
    for game in GAMES:
        arms, (depth, full, tq, ts, leaves), L, top, box = measure(game)
        for width, (ta, tb, ranges) in arms.items():
            ratio = float(np.median(tb) / np.median(ta))
            arm_rows.append("| %s | %d | %d | %d | %.1f (%.1f - %.1f) | %.0f (%.0f - %.0f) | %.1f |" % (
                game, top, width, ranges, np.median(ta), ta.min(), ta.max(), np.median(tb), tb.min(), tb.max(), ratio))
            if ratio < 1.0:
                slower.append((game, width, ratio))
        per = [float(np.median(t)) * 1e6 / (N * FRAMES * c) for t, c in zip((tq, ts), leaves)]
        leaf_rows.append("| %s | %d | %d | %.1f | %.3f | %.1f | %.3f |" % (game, depth, full, np.median(tq), per[0], np.median(ts), per[1]))
    lines = ["# Beam search (scripts/beam_rate.py)", "",
             "Box: %s (%s, %d CUs), one process, agent layer off, %d envs, frames = %d, hold = %d, depth = TBX_PLAN_MAX_DEPTH(game), rest = the first "
             "legal action, objective 0.  Both arms are host forms timed on the wall clock from the call to the rows on the host: ms per call as the "
             "median (min - max) of %d interleaved regions after one warm-up of each arm.  Arm (a) is TBX_QUERY_LOOKAHEAD_BEAM; arm (b) drives the same "
             "beam from the host, per level one TBX_QUERY_LOOKAHEAD_PLAN call per (first action, slot, digit) with per-env code rows and the kept set "
             "by a numpy lexsort.  The arms returned identical rows (asserted)." % (
                 box["name"] or "device %d at %s" % (box["ordinal"], box["pci"]), box["arch"], box["compute_units"], N, FRAMES, HOLD, REGIONS), "",
             "| game | depth | width | env ranges | (a) query ms | (b) host-driven ms | (b) / (a) |", "|---|---|---|---|---|---|---|"] + arm_rows
    lines += ["", "## Per leaf-frame against the exhaustive search (reported, not gated)", "",
              "The deepest depth the search accepts at which TBX_BEAM_MAX_WIDTH is wide enough, width = n_legal^(depth - 2): the beam returns the "
              "search's rows and plays every level's candidates, about L / (L - 1) times the search's leaves, plus a select per level.  Device forms "
              "between HIP events on a caller's stream, the median of %d interleaved regions after one warm-up, as profiles/search.md times its "
              "calls; ns per leaf-frame over the leaf-frames each plays." % EVENT_REGIONS, "",
              "| game | depth | width | beam ms | beam ns per leaf-frame | search ms | search ns per leaf-frame |", "|---|---|---|---|---|---|---|"] + leaf_rows
    if os.path.exists(args.out):
        old = open(args.out).read()
        if KEEP in old:
            lines += ["", old[old.index(KEEP):].rstrip()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    assert not slower, "the gate: the query is slower than the host-driven beam: %r" % (slower,)
    return 0


if __name__ == "__main__":
    sys.exit(main())
