#!/usr/bin/env python3
"""What TBX_QUERY_LOOKAHEAD_EVOLVE costs (include/toybox_amd.h) at 4 096 envs, frames = 64, hold = 4, depth = TBX_PLAN_MAX_DEPTH(game),
generations = 8, elite = population / 4, populations 16 and 64, agent layer off, one process, one call per game and population.

Two arms, interleaved in the same session, both host forms timed on the wall clock from the call to the rows on the host:
  (a) the query;
  (b) the same evolution driven from the host with what the engine offered before: per generation one TBX_QUERY_LOOKAHEAD_PLAN call
      per (first action, individual that is not a carried elite) with per-env code rows, the rows read back, ranking and breeding in
      numpy.  The draw words depend on nothing but their indices, so arm (b) draws them BEFORE the clock starts: its time is the
      calls, the ranking and the gathers -- the baseline is given that head start on purpose.
The two arms must return identical rows (asserted).  Nothing is gated: the expectation is that (a) is not slower in any game, and a
game that loses is named in the file.  ms per call as the median (min - max) of REGIONS interleaved regions after one warm-up of
each arm.

    python scripts/evolve_rate.py [--out profiles/evolve.md]

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

REGIONS = 3
KEEP = "## Budgets"
GAMES, N, FRAMES, HOLD, GENERATIONS, POPULATIONS = ("breakout", "space_invaders", "amidar", "gridworld"), 4096, 64, 4, 8, (16, 64)
PLAN_SEED, MUTATION = 12345, 64
FIELDS = ("ret", "score", "lives", "frames_run", "life_lost_at", "code")


def splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def draws(L, depth, P, E):
    """everything of the definition that does not depend on an outcome: the codes of generation 0 [N, L, P] and, per later
    generation, the parent's rank [N, L, P - E] and the redrawn digits [N, L, P - E, depth] (-1: the parent's stays)"""
    env = np.arange(N, dtype=np.uint64)[:, None]
    a = np.arange(L, dtype=np.uint64)[None, :]
    base = splitmix64(splitmix64(np.uint64(PLAN_SEED) ^ (a << np.uint64(32))) ^ env)                      # [N, L]
    p = np.arange(depth, dtype=np.uint64)

    def words(g, i):                                                                                       # [N, L, len(i), depth]
        return splitmix64(base[:, :, None, None] ^ np.uint64(g << 40) ^ (i.astype(np.uint64) << np.uint64(8))[None, None, :, None] ^ p[None, None, None, :])
    pow_ = (L ** np.arange(depth)).astype(np.int64)
    d0 = ((words(0, np.arange(P)) >> np.uint64(32)) % np.uint64(L)).astype(np.int64)
    d0[..., 0] = np.arange(L)[None, :, None]
    first = (d0 * pow_).sum(axis=-1)
    later = []
    for g in range(1, GENERATIONS + 1):
        w = words(g, np.arange(E, P))
        redrawn = np.where((w & np.uint64(0xff)) < np.uint64(MUTATION), ((w >> np.uint64(32)) % np.uint64(L)).astype(np.int8), np.int8(-1))
        redrawn[..., 0] = -1
        later.append((((w[..., 0] >> np.uint64(32)) % np.uint64(E)).astype(np.int64), redrawn))
    return first, later, pow_


def host_evolve(e, game, depth, P, E, objective, rest, drawn):
    """arm (b): the evolution of include/toybox_amd.h out of TBX_QUERY_LOOKAHEAD_PLAN calls and numpy; the query's six fields [N, L]"""
    L = len(e.legal_actions)
    codes, later, pow_ = drawn
    rows = np.empty((N, L, P, 5))
    index = np.broadcast_to(np.arange(P), (N, L, P))
    for g in range(GENERATIONS + 1):
        for a in range(L):
            for i in range(E if g else 0, P):
                args, _ = plan_args(game, N, FRAMES, hold=HOLD, depth=depth, code=codes[:, a, i], rest=rest)
                rows[:, a, i] = e.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args)
        ret, lives, loss = rows[..., 0], rows[..., 2], np.where(rows[..., 4] < 0, _abi.LOOKAHEAD_MAX_FRAMES + 1, rows[..., 4])
        keys = (ret, lives, loss) if objective == 0 else (lives, loss, ret)
        order = np.lexsort((index, codes) + tuple(-k for k in reversed(keys)), axis=2)                    # the last key is the primary one
        ranked = np.take_along_axis(codes, order, axis=2)
        rows = np.take_along_axis(rows, order[..., None], axis=2)                                          # slots 0 .. E-1: the elites, carried
        if g == GENERATIONS:
            break
        parent_rank, redrawn = later[g]
        parent = np.take_along_axis(ranked, parent_rank, axis=2)
        digits = parent[..., None] // pow_ % L
        child = (np.where(redrawn >= 0, redrawn, digits) * pow_).sum(axis=-1)
        codes = np.concatenate([ranked[..., :E], child], axis=2)
    out = {k: rows[:, :, 0, i] for i, k in enumerate(FIELDS[:5])}
    out["code"] = ranked[..., 0]
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
    for P in POPULATIONS:
        E = P // 4
        drawn = draws(L, top, P, E)

        def query():
            return e.lookahead_evolve(FRAMES, top, P, GENERATIONS, elite=E, mutation=MUTATION, plan_seed=PLAN_SEED, hold=HOLD, rest=rest)

        def composed():
            return host_evolve(e, game, top, P, E, 0, rest, drawn)

        a, b = wall_ms(query)[1], wall_ms(composed)[1]       # one warm-up of each arm, and the two arms agree
        for k in FIELDS:
            assert np.array_equal(np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)), "%s population %d: the arms differ in %s" % (game, P, k)
        ta, tb = [], []
        for _ in range(REGIONS):
            ta.append(wall_ms(query)[0])
            tb.append(wall_ms(composed)[0])
        arms[P] = (np.asarray(ta), np.asarray(tb), e.evolve_ranges)
        print(game, P, np.median(ta), np.median(tb), flush=True)
    box = e.device_identity()
    e.close()
    return arms, L, top, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evolve.md"))
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("evolve_rate.py measures on a GPU; none found")
    arm_rows, slower, box = [], [], None
    for game in GAMES:
        arms, L, top, box = measure(game)
        for P, (ta, tb, ranges) in arms.items():
            ratio = float(np.median(tb) / np.median(ta))
            plays = L * (P + GENERATIONS * (P - P // 4))
            arm_rows.append("| %s | %d | %d | %d | %d | %.1f (%.1f - %.1f) | %.0f (%.0f - %.0f) | %.1f |" % (
                game, top, P, plays, ranges, np.median(ta), ta.min(), ta.max(), np.median(tb), tb.min(), tb.max(), ratio))
            if ratio < 1.0:
                slower.append("%s at population %d (%.2f)" % (game, P, ratio))
    lines = ["# Evolutionary plan search (scripts/evolve_rate.py)", "",
             "Box: %s (%s, %d CUs), one process, agent layer off, %d envs, frames = %d, hold = %d, depth = TBX_PLAN_MAX_DEPTH(game), generations = %d, "
             "elite = population / 4, mutation = %d, rest = the first legal action, objective 0.  Both arms are host forms timed on the wall clock from the "
             "call to the rows on the host: ms per call as the median (min - max) of %d interleaved regions after one warm-up of each arm.  Arm (a) is "
             "TBX_QUERY_LOOKAHEAD_EVOLVE; arm (b) drives the same evolution from the host, per generation one TBX_QUERY_LOOKAHEAD_PLAN call per (first "
             "action, individual that is not a carried elite) with per-env code rows, ranking and breeding in numpy, the draw words drawn before the "
             "clock starts.  The arms returned identical rows (asserted).  Plays: plans played per env and call, elites carried." % (
                 box["name"] or "device %d at %s" % (box["ordinal"], box["pci"]), box["arch"], box["compute_units"], N, FRAMES, HOLD, GENERATIONS, MUTATION, REGIONS), "",
             "| game | depth | population | plays per env | env ranges | (a) query ms | (b) host-driven ms | (b) / (a) |", "|---|---|---|---|---|---|---|---|"] + arm_rows
    lines += ["", "The query is slower than the host-driven evolution in: %s." % ", ".join(slower) if slower else
              "The query is not slower than the host-driven evolution in any game."]
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
