#!/usr/bin/env python3
"""What the closed loop costs with and without the host in it (TBX_QUERY_LOOKAHEAD_ACT, include/toybox_amd.h): 4 096 envs, frames = 64,
hold = 4, depth = TBX_PLAN_MAX_DEPTH(game), 32 closed-loop periods per region, agent layer off, one process.  Planner 158 at
population 64 / generations 8 / elite 16 (mutation 64), planner 156 at width 4; rest = the first legal action, objective "return".

Two arms on two env batches made and played alike, interleaved in the same session, each timed on the wall clock from its first call
to the last period's results on the host:
  (a) ToyboxVecEnv.plan_rollout: the device loop -- per period the query and `hold` tbx_step_device calls reading TBX_BUF_PLAN_ACTION,
      queued back to back on one stream, ONE synchronisation at the end (and the frames of the last state, which step() returns);
  (b) the loop as it could be run before: the planner through tbx_reduce (Engine.lookahead_evolve / lookahead_beam), the pick in
      numpy (one lexsort), the actions through the host form of the step, and for the evolution init_plan = np.roll(best_plan, -1)
      per env -- per-env rows that tbx_reduce scans on the host, so this arm does not pay the worst case either.
Both arms must choose identical actions in every period of every region (asserted), so they stay on the same states.  ms per region
as the median (min - max) of REGIONS interleaved regions after one warm-up region of each arm.  Nothing is gated: the expectation is
that (a) is not slower in any game; a ratio near 1 where play dominates is a finding, recorded as one.

    python scripts/act_rate.py [--out profiles/act.md] [--planners evolve beam] [--games ...]

Needs a GPU; prints the markdown it writes and keeps the file from "## Kernels" on, which is written by hand."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from toybox_amd import _abi, hip  # noqa: E402
from toybox_amd.envs import vec_env  # noqa: E402
from toybox_amd.envs.vec_env import ToyboxVecEnv  # noqa: E402

REGIONS = 3
KEEP = "## Kernels"
GAMES, N, FRAMES, HOLD, PERIODS = ("breakout", "space_invaders", "amidar", "gridworld"), 4096, 64, 4, 32
POPULATION, GENERATIONS, ELITE, MUTATION, PLAN_SEED, WIDTH = 64, 8, 16, 64, 12345, 4


def make(game):
    env = ToyboxVecEnv(game, N, seed=1234, cache_terminal_state=False, obs_pool=1)
    env.reset()
    for t in range(16, 400):                                 # mid-game states
        env.engine.step_synthetic(1337, t, auto_reset=True)
    env.engine.sync()
    return env


def device_loop(env, planner, depth, t0):
    """arm (a) -> the action indices [PERIODS, N]"""
    kw = dict(population=POPULATION, generations=GENERATIONS, elite=ELITE, mutation=MUTATION, plan_seed=PLAN_SEED) if planner == "evolve" else dict(width=WIDTH)
    env.plan_rollout(PERIODS, planner, steps=FRAMES // HOLD, depth=depth, hold=HOLD, rest=0, t=t0, **kw)
    return env.plan_actions()


def host_loop(env, planner, depth, t0, plan):
    """arm (b) -> (the action indices [PERIODS, N], the last best_plan).  plan: the best_plan of the period before, or None"""
    actions = np.empty((PERIODS, N), np.int64)
    for p in range(PERIODS):
        if planner == "evolve":
            out = vec_env._evolve(env, FRAMES, HOLD, depth, POPULATION, GENERATIONS, ELITE, MUTATION, PLAN_SEED, None if plan is None else np.roll(plan, -1, axis=1),
                                  "return", 0, 0, t0 + p)
        else:
            out = vec_env._beam(env, FRAMES, HOLD, depth, WIDTH, "return", 0, 0, t0 + p)
        plan = out["best_plan"]
        actions[p] = out["best_action"]
        ale = env._lut[actions[p]]
        for _ in range(HOLD):
            env.engine.step(ale, auto_reset=True)
    return actions, plan


def wall_ms(body):
    t0 = time.perf_counter()
    out = body()
    return (time.perf_counter() - t0) * 1e3, out


def measure(game, planner):
    a, b = make(game), make(game)
    depth = _abi.PLAN_MAX_DEPTH[game]
    ta, tb, plan = [], [], None
    for region in range(REGIONS + 1):                        # region 0: the warm-up of each arm
        t0 = region * PERIODS
        ms_a, got = wall_ms(lambda: device_loop(a, planner, depth, t0))
        ms_b, (want, plan) = wall_ms(lambda: host_loop(b, planner, depth, t0, plan))
        assert np.array_equal(got, want), "%s %s region %d: the arms chose different actions in %d places" % (game, planner, region, int((got != want).sum()))
        if region:
            ta.append(ms_a)
            tb.append(ms_b)
        print(game, planner, region, "%.0f ms  %.0f ms" % (ms_a, ms_b), flush=True)
    assert bytes(a.engine.get_states()) == bytes(b.engine.get_states()), "%s %s: the arms ended in different states" % (game, planner)
    box = a.engine.device_identity()
    a.close()
    b.close()
    return np.asarray(ta), np.asarray(tb), depth, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "act.md"))
    ap.add_argument("--planners", nargs="+", default=["evolve", "beam"])
    ap.add_argument("--games", nargs="+", default=list(GAMES))
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("act_rate.py measures on a GPU; none found")
    rows, slower, box = [], [], None
    for planner in args.planners:
        for game in args.games:
            ta, tb, depth, box = measure(game, planner)
            ratio = float(np.median(tb) / np.median(ta))
            rows.append("| %s | %s | %d | %.0f (%.0f - %.0f) | %.0f (%.0f - %.0f) | %.2f |" % (
                game, "158, P %d / G %d / E %d" % (POPULATION, GENERATIONS, ELITE) if planner == "evolve" else "156, width %d" % WIDTH, depth,
                np.median(ta), ta.min(), ta.max(), np.median(tb), tb.min(), tb.max(), ratio))
            if ratio < 1.0:
                slower.append("%s with planner %s (%.2f)" % (game, planner, ratio))
    lines = ["# Closed-loop planning on the device (scripts/act_rate.py)", "",
             "Box: %s (%s, %d CUs), one process, agent layer off, %d envs, frames = %d, hold = %d, depth = TBX_PLAN_MAX_DEPTH(game), %d closed-loop periods "
             "per region, rest = the first legal action, objective 0.  Arm (a) is ToyboxVecEnv.plan_rollout: TBX_QUERY_LOOKAHEAD_ACT and the steps that "
             "read TBX_BUF_PLAN_ACTION queued on one stream, one synchronisation at the end.  Arm (b) runs the planner through tbx_reduce, picks in numpy, "
             "steps through the host form and hands the evolution init_plan = np.roll(best_plan, -1) per env.  Wall clock from the first call to the last "
             "period's results on the host: ms per region as the median (min - max) of %d interleaved regions after one warm-up region of each arm.  The "
             "arms chose identical actions in every period (asserted)." % (
                 box["name"] or "device %d at %s" % (box["ordinal"], box["pci"]), box["arch"], box["compute_units"], N, FRAMES, HOLD, PERIODS, REGIONS), "",
             "| game | planner | depth | (a) device loop ms | (b) host loop ms | (b) / (a) |", "|---|---|---|---|---|---|"] + rows
    lines += ["", "The device loop is slower than the host loop in: %s." % ", ".join(slower) if slower else "The device loop is not slower than the host loop in any game."]
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
