#!/usr/bin/env python3
"""What TBX_QUERY_LOOKAHEAD_TREE_ACT costs and what its carried trees buy (include/toybox_amd.h), at profiles/tree.md's settings:
4 096 envs, frames = 64, hold = 4, depth 8, 256 simulations, the per-game explore, salt 1, drawn rest, objective 0, agent layer off, one
process.

  1. the call: TBX_QUERY_LOOKAHEAD_TREE (160), 161 with reuse = 0 and 161 with reuse = 1 (from the store the call before it left),
     host forms timed on the wall clock from the call to the rows on the host, interleaved, one warm-up of each, median (min - max) of
     REGIONS regions.  All three run on THIS tree's library: the parent commit's 160 is not an arm here.
  2. the loop: --loop-periods periods queued on one stream -- reduce_device(161, reuse = 1), `hold` step_device calls on the action
     buffer, TBX_EDIT_TREE_DROP behind every step with the done buffer as its mask, one synchronisation at the end: exactly what the
     adapters' plan_rollout(k, "tree", reuse=True) queues, without their copies of rewards and dones and their frame delivery --
     against the loop driven from the host: lookahead_tree (160), plan_pick on the host, step() with the uploaded actions.  With
     reuse the two loops pick differently and end in different states; both play the same number of frames.  A loop counts as
     slower or faster only where every region of one arm lies beyond every region of the other.
  3. what reuse buys: from the same start states --periods periods with reuse = 1 at M, reuse = 0 at M and reuse = 1 at M / 2: the
     mean return per env over the window (the sum of the steps' rewards), lives lost per env, the mean pv_depth and pv_visits of the
     picked rows, the time, and -- in the reuse = 1 arm at M -- the share of (env, period) pairs in which the pick differs from
     query 160's pick on the same state.
Nothing is gated: no ratio is fixed in advance.

    python scripts/tree_act_rate.py [--out profiles/tree_act.md] [--envs 4096] [--simulations 256] [--loop-periods 32] [--periods 64]

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
from toybox_amd.engine import plan_pick, tree_act_args  # noqa: E402
from tree_rate import EXPLORE, FRAMES, DEPTH, GAMES, HOLD, SEED  # noqa: E402

REGIONS = 3
LOOP_REGIONS = 2
KEEP = "## Scratch"
SALT = 1


def world(game, N):
    e = make(game, N, "raw")
    for t in range(16, 400):                                 # mid-game states
        e.step_synthetic(1337, t, auto_reset=True)
    e.sync()
    return e


def wall_ms(body):
    t0 = time.perf_counter()
    out = body()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(t):
    t = np.asarray(t)
    return "%.1f (%.1f - %.1f)" % (np.median(t), t.min(), t.max())


def the_call(game, N, M):
    e = world(game, N)
    kw = dict(explore=EXPLORE[game], salt=SALT, hold=HOLD, seed=SEED)
    arms = {"160": lambda: e.lookahead_tree(FRAMES, DEPTH, M, **kw), "161 reuse 0": lambda: e.lookahead_tree_act(FRAMES, DEPTH, M, reuse=False, **kw),
            "161 reuse 1": lambda: e.lookahead_tree_act(FRAMES, DEPTH, M, reuse=True, **kw)}
    times = {k: [] for k in arms}
    for region in range(REGIONS + 1):
        for k, body in arms.items():
            ms = wall_ms(body)[0]
            if region:
                times[k].append(ms)
    out = (times, e.tree_ranges, e.device_identity())
    e.close()
    return out


def device_loop(e, game, M, periods, reuse, stream, rows):
    n = e.n_envs
    for p in range(periods):
        args = tree_act_args(game, FRAMES, DEPTH, M, EXPLORE[game], SALT, reuse, hold=HOLD, seed=SEED, t=p)
        e.reduce_device(_abi.QUERY_LOOKAHEAD_TREE_ACT, rows + p * n * 14 * 8, args, stream=stream.ptr)
        pa = e.plan_action_ptr
        for _ in range(HOLD):
            e.step_device(pa, auto_reset=True, stream=stream.ptr)
            if reuse:
                e.tree_drop_device(e.device_buffer(_abi.BUF_DONE)[0], stream=stream.ptr)
    stream.synchronize()


def host_loop(e, game, M, periods):
    legal = np.asarray(e.legal_actions, np.int32)
    for p in range(periods):
        out = e.lookahead_tree(FRAMES, DEPTH, M, explore=EXPLORE[game], salt=SALT, hold=HOLD, seed=SEED, t=p)
        rows = np.stack([out[k] for k in ("samples", "ret_sum", "ret_min", "ret_max", "lives_sum", "lost", "ended", "safe_frames_sum", "code")], axis=2)
        action = legal[plan_pick(rows, 0, sampled=True)]
        for _ in range(HOLD):
            e.step(action, auto_reset=True)


def the_loop(game, N, M, periods):
    a, b = world(game, N), world(game, N)
    stream = hip.Stream()
    rows = hip.malloc(periods * N * 14 * 8)
    ta, tb = [], []
    for region in range(LOOP_REGIONS + 1):
        x = wall_ms(lambda: device_loop(a, game, M, periods, True, stream, rows))[0]
        y = wall_ms(lambda: host_loop(b, game, M, periods))[0]
        if region:
            ta.append(x)
            tb.append(y)
    a.sync()
    hip.free(rows)
    stream.close()
    a.close()
    b.close()
    return ta, tb


def what_reuse_buys(game, N, M, periods):
    out = {}
    for name, sims, reuse in (("reuse 1 at M", M, True), ("reuse 0 at M", M, False), ("reuse 1 at M/2", M // 2, True)):
        e = world(game, N)
        legal = np.asarray(e.legal_actions, np.int32)
        score0, lives0 = (np.asarray(x).astype(np.int64) for x in e.scalars()[:2])
        ret, lost, depth, visits, differ, t0 = np.zeros(N), np.zeros(N), [], [], [], time.perf_counter()
        for p in range(periods):
            kw = dict(explore=EXPLORE[game], salt=SALT, hold=HOLD, seed=SEED, t=p)
            if name == "reuse 1 at M":                        # the pick of query 160 on the same state (it leaves the store alone)
                plain = e.lookahead_tree(FRAMES, DEPTH, sims, **kw)
                rows = np.stack([plain[k] for k in ("samples", "ret_sum", "ret_min", "ret_max", "lives_sum", "lost", "ended", "safe_frames_sum", "code")], axis=2)
                base = plan_pick(rows, 0, sampled=True)
            got = e.lookahead_tree_act(FRAMES, DEPTH, sims, reuse=reuse, **kw)
            if name == "reuse 1 at M":
                differ.append(float((got["action_index"] != base).mean()))
            depth.append(float(got["pv_depth"].mean()))
            visits.append(float(got["pv_visits"].mean()))
            for _ in range(HOLD):
                reward, done, lives, _ = e.step(legal[got["action_index"]], auto_reset=True)
                ret += np.asarray(reward)
                lost += np.asarray(lives) < lives0
                lives0 = np.asarray(lives).astype(np.int64)
                if reuse:
                    e.tree_drop(np.asarray(done).astype(bool))
        out[name] = dict(ret=ret.mean(), lost=lost.mean(), depth=np.mean(depth), visits=np.mean(visits), differ=np.mean(differ) if differ else None,
                         seconds=time.perf_counter() - t0)
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_act.md"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--simulations", type=int, default=256)
    ap.add_argument("--loop-periods", type=int, default=32)
    ap.add_argument("--periods", type=int, default=64)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("tree_act_rate.py measures on a GPU; none found")
    N, M, K = args.envs, args.simulations, args.periods
    call_rows, loop_rows, buy_rows, box, slower, faster = [], [], [], None, [], []
    for game in GAMES:
        times, ranges, box = the_call(game, N, M)
        call_rows.append("| %s | %d | %s | %s | %s | %.3f |" % (game, ranges, fmt(times["160"]), fmt(times["161 reuse 0"]), fmt(times["161 reuse 1"]),
                                                             np.median(times["161 reuse 0"]) / np.median(times["160"])))
        print(call_rows[-1], flush=True)
        ta, tb = the_loop(game, N, M, args.loop_periods)
        loop_rows.append("| %s | %s | %s | %.2f |" % (game, fmt(ta), fmt(tb), np.median(tb) / np.median(ta)))
        if min(ta) > max(tb):                                # apart by more than the regions' own spread, or it is called level
            slower.append(game)
        elif max(ta) < min(tb):
            faster.append(game)
        print(loop_rows[-1], flush=True)
        for name, r in what_reuse_buys(game, N, M, K).items():
            buy_rows.append("| %s | %s | %.2f | %.3f | %.2f | %.1f | %s | %.1f |" % (game, name, r["ret"], r["lost"], r["depth"], r["visits"],
                                                                                  "-" if r["differ"] is None else "%.3f" % r["differ"], r["seconds"]))
            print(buy_rows[-1], flush=True)
    lines = ["# Closed-loop tree search (scripts/tree_act_rate.py)", "",
             "Box: %s (%s, %d CUs), one process, agent layer off, %d envs, frames = %d, hold = %d, depth = %d, simulations M = %d, salt %d, drawn rest, objective 0, "
             "explore per game as in profiles/tree.md.  Wall-clock times, median (min - max) of %d interleaved regions (the loops: 2) after one warm-up of each arm." % (
                 box["name"] or "device %d at %s" % (box["ordinal"], box["pci"]), box["arch"], box["compute_units"], N, FRAMES, HOLD, DEPTH, M, SALT, REGIONS), "",
             "## 1. The call", "",
             "Host forms, from the call to the rows on the host, ms.  All three arms run on this tree's library; the env ranges are those of the last 161 "
             "(its working trees have 2 M + 2 nodes, query 160's M + 2).", "",
             "| game | env ranges (161) | 160 ms | 161 reuse 0 ms | 161 reuse 1 ms | 161 reuse 0 / 160 |", "|---|---|---|---|---|---|"] + call_rows
    lines += ["", "## 2. The loop", "",
              "%d periods.  Device: reduce_device(161, reuse 1), %d step_device calls on TBX_BUF_PLAN_ACTION, TBX_EDIT_TREE_DROP behind each with the done buffer as its "
              "mask, one synchronisation at the end: what plan_rollout(k, \"tree\", reuse=True) queues, without its reward and done copies and its frame delivery.  Host: "
              "lookahead_tree (160), plan_pick in numpy, step() with the uploaded actions.  ms per loop." % (args.loop_periods, HOLD), "",
              "| game | device loop ms | host loop ms | host / device |", "|---|---|---|---|"] + loop_rows
    lines += ["", "A loop counts as slower or faster only where every region of one arm lies beyond every region of the other; otherwise the two are level.",
              "THE DEVICE LOOP IS SLOWER THAN THE HOST LOOP IN: %s." % ", ".join(slower) if slower else "The device loop is not slower than the host loop in any game.",
              "The device loop is faster than the host loop in: %s." % ", ".join(faster) if faster else "THE DEVICE LOOP IS NOT FASTER THAN THE HOST LOOP IN ANY GAME."]
    lines += ["", "## 3. What reuse buys", "",
              "%d periods from the same start states, host forms, every env's picked action played for %d frames with auto-reset; with reuse the envs whose game "
              "ended are dropped (TBX_EDIT_TREE_DROP, host mask).  return: mean over envs of the rewards of the window; lives lost: mean per env; pv depth / pv visits: "
              "means over the picked rows; pick differs: share of (env, period) pairs in which the pick differs from query 160's pick on the same state (that arm "
              "pays one extra query 160 a period: its seconds are not comparable).  No threshold is set." % (K, HOLD), "",
              "| game | arm | return | lives lost | pv depth | pv visits | pick differs | seconds |", "|---|---|---|---|---|---|---|---|"] + buy_rows
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
