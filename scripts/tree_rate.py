#!/usr/bin/env python3
"""What TBX_QUERY_LOOKAHEAD_TREE costs (include/toybox_amd.h) at 4 096 envs, frames = 64, hold = 4, depth 8, 256 simulations, explore
chosen per game (about one step of the game's score), salt 0, agent layer off, one process, one call per game.

Two arms, interleaved in the same session, both host forms timed on the wall clock from the call to the rows on the host:
  (a) the query;
  (b) the same tree driven from the host with what the engine offered before: per simulation one TBX_QUERY_LOOKAHEAD_PLAN call per
      first action with per-env depth and code rows under the seed of future m, the rows read back, and the trees of all envs in
      numpy arrays (selection, expansion, backup and the principal variation vectorised over envs and first actions).
The two arms must return identical rows (asserted).  Nothing is gated: no ratio is fixed in advance.  ms per call as the median
(min - max) of REGIONS interleaved regions after one warm-up of each arm.

    python scripts/tree_rate.py [--out profiles/tree.md] [--envs 4096] [--simulations 256]

Needs a GPU; prints the markdown it writes and keeps the file from "## Scratch" on, which is written by hand."""
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
from toybox_amd.engine import TREE_FIELDS, plan_args, sample_seed  # noqa: E402

REGIONS = 3
KEEP = "## Scratch"
GAMES, FRAMES, HOLD, DEPTH, SEED = ("breakout", "space_invaders", "amidar", "gridworld"), 64, 4, 8, 77
EXPLORE = {"breakout": 4, "space_invaders": 16, "amidar": 4, "gridworld": 1}


def isqrt(x):
    """the exact floor square root of int64 x < 2^52"""
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    r -= r * r > x
    r += (r + 1) * (r + 1) <= x
    return r


def host_tree(e, game, N, M, objective, explore, rest):
    """arm (b): the tree of include/toybox_amd.h out of TBX_QUERY_LOOKAHEAD_PLAN calls and numpy; the query's twelve fields [N, L]"""
    L = len(e.legal_actions)
    I, A = np.meshgrid(np.arange(N), np.arange(L), indexing="ij")
    n, v = np.zeros((N, L, M + 1), np.int64), np.zeros((N, L, M + 1), np.int64)
    child = np.zeros((N, L, M + 1, L), np.int64)              # 0: no child
    count = np.ones((N, L), np.int64)
    sums = {k: np.zeros((N, L), np.int64) for k in TREE_FIELDS[:8]}
    for m in range(M):
        cur, d, code, done = np.zeros((N, L), np.int64), np.ones((N, L), np.int64), A.copy(), np.zeros((N, L), bool)
        for level in range(1, DEPTH):
            ch = child[I, A, cur]                             # [N, L, L]
            absent = ch == 0
            grow = ~done & absent.any(-1)
            k = absent.argmax(-1)
            child[I[grow], A[grow], cur[grow], k[grow]] = count[grow]
            count[grow] += 1
            nk, vk = n[I[..., None], A[..., None], ch], v[I[..., None], A[..., None], ch]
            root = isqrt(n[I, A, cur] << 16)
            P = vk * 256 // np.maximum(nk, 1) + (explore * root)[..., None] // (1 + nk)
            walk = ~done & ~grow
            k = np.where(grow, k, P.argmax(-1))               # argmax: the first, the smaller k
            step = grow | walk
            code = np.where(step, code + k * L ** level, code)
            d += step
            cur = np.where(walk, np.take_along_axis(ch, k[..., None], -1)[..., 0], cur)
            done |= grow
        f = np.empty((N, L, 5))
        for a in range(L):
            args, _ = plan_args(game, N, FRAMES, hold=HOLD, depth=d[:, a], code=code[:, a], rest=rest, seed=sample_seed(SEED, m))
            f[:, a] = e.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args)
        ret, lives, run, lost_at = (f[..., i].astype(np.int64) for i in (0, 2, 3, 4))
        safe = np.where(lost_at < 0, run, lost_at)
        value = ret if objective == 0 else safe
        cur = np.zeros((N, L), np.int64)
        for level in range(1, DEPTH + 1):
            on = level <= d
            n[I[on], A[on], cur[on]] += 1                     # (one node per tree and level: no index twice)
            v[I[on], A[on], cur[on]] += value[on]
            digit = code // L ** level % L
            cur = np.where(level < d, child[I, A, cur, digit], cur)
        sums["ret_min"] = ret.copy() if m == 0 else np.minimum(sums["ret_min"], ret)
        sums["ret_max"] = ret.copy() if m == 0 else np.maximum(sums["ret_max"], ret)
        sums["samples"] += 1; sums["ret_sum"] += ret; sums["lives_sum"] += lives; sums["lost"] += lost_at >= 0; sums["ended"] += lives <= 0
        sums["safe_frames_sum"] += safe
    cur, d, code = np.zeros((N, L), np.int64), np.ones((N, L), np.int64), A.copy()
    for level in range(1, DEPTH):
        ch = child[I, A, cur]
        nk, vk = n[I[..., None], A[..., None], ch], v[I[..., None], A[..., None], ch]
        key = np.where(ch > 0, nk * (1 << 40) + vk, -1)      # the larger n, then the larger v_sum (below 2^40), then the smaller k
        k = key.argmax(-1)
        go = (ch > 0).any(-1) & (d == level)
        code, d = np.where(go, code + k * L ** level, code), d + go
        cur = np.where(go, np.take_along_axis(ch, k[..., None], -1)[..., 0], cur)
    return dict(sums, code=code, pv_depth=d, pv_visits=n[I, A, cur], pv_value=v[I, A, cur])


def wall_ms(body):
    t0 = time.perf_counter()
    out = body()
    return (time.perf_counter() - t0) * 1e3, out


def measure(game, N, M):
    e = make(game, N, "raw")
    for t in range(16, 400):                                 # mid-game states
        e.step_synthetic(1337, t, auto_reset=True)
    e.sync()
    rest = e.legal_actions[0]

    def query():
        return e.lookahead_tree(FRAMES, DEPTH, M, explore=EXPLORE[game], hold=HOLD, rest=rest, seed=SEED)

    def composed():
        return host_tree(e, game, N, M, 0, EXPLORE[game], rest)

    a, b = wall_ms(query)[1], wall_ms(composed)[1]           # one warm-up of each arm, and the two arms agree
    for k in TREE_FIELDS:
        assert np.array_equal(np.asarray(a[k]).astype(np.int64), np.asarray(b[k]).astype(np.int64)), "%s: the arms differ in %s" % (game, k)
    ta, tb = [], []
    for _ in range(REGIONS):
        ta.append(wall_ms(query)[0])
        tb.append(wall_ms(composed)[0])
    print(game, np.median(ta), np.median(tb), flush=True)
    out = (np.asarray(ta), np.asarray(tb), e.tree_ranges, float(a["pv_depth"].mean()), len(e.legal_actions), e.device_identity())
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree.md"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--simulations", type=int, default=256)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("tree_rate.py measures on a GPU; none found")
    N, M = args.envs, args.simulations
    rows, slower, box = [], [], None
    for game in GAMES:
        ta, tb, ranges, pv, L, box = measure(game, N, M)
        ratio = float(np.median(tb) / np.median(ta))
        rows.append("| %s | %d | %d | %.1f | %d | %.1f (%.1f - %.1f) | %.0f (%.0f - %.0f) | %.1f |" % (
            game, EXPLORE[game], L * M, pv, ranges, np.median(ta), ta.min(), ta.max(), np.median(tb), tb.min(), tb.max(), ratio))
        if ratio < 1.0:
            slower.append("%s (%.2f)" % (game, ratio))
    lines = ["# Tree search (scripts/tree_rate.py)", "",
             "Box: %s (%s, %d CUs), one process, agent layer off, %d envs, frames = %d, hold = %d, depth = %d, simulations = %d, salt 0, rest = the first "
             "legal action, objective 0, explore per game (about one step of the game's score).  Both arms are host forms timed on the wall clock from the "
             "call to the rows on the host: ms per call as the median (min - max) of %d interleaved regions after one warm-up of each arm.  Arm (a) is "
             "TBX_QUERY_LOOKAHEAD_TREE; arm (b) drives the same trees from the host, per simulation one TBX_QUERY_LOOKAHEAD_PLAN call per first action with "
             "per-env depth and code rows under the seed of future m, the trees of all envs in numpy arrays.  The arms returned identical rows "
             "(asserted).  Plays: plans played per env and call.  PV depth: the mean depth of the principal variation over all rows." % (
                 box["name"] or "device %d at %s" % (box["ordinal"], box["pci"]), box["arch"], box["compute_units"], N, FRAMES, HOLD, DEPTH, M, REGIONS), "",
             "| game | explore | plays per env | PV depth | env ranges | (a) query ms | (b) host-driven ms | (b) / (a) |", "|---|---|---|---|---|---|---|---|"] + rows
    lines += ["", "The query is slower than the host-driven tree in: %s." % ", ".join(slower) if slower else "The query is not slower than the host-driven tree in any game."]
    lines += ["", "Arm (b)'s time is its %d x L plan calls with their row uploads and read-backs PLUS the numpy trees of %d x L units (fancy-indexed arrays, "
              "vectorised over envs); the two shares are not measured apart, so the ratio says what a caller of the host form pays, not what the plan "
              "kernel costs." % (M, N)]
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
