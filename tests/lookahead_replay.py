"""The yardstick of the lookahead tests (TBX_QUERY_LOOKAHEAD / _ALL, include/toybox_amd.h): CLONE AND PLAY.

The CPU checker has no lookahead and needs none.  What the query must answer is built from what the checker already has: a fresh
checker engine that is given the batch's state records and simulator RNGs (set_states, set_sim_rng) IS that batch -- envs are
nothing else (tests/test_lookahead.py checks that a clone continues byte for byte like its original) -- and tbx_step without
auto-reset plays the schedule on it frame by frame.  The five fields are then plain numpy over the scalars read after every
frame.  An env's row is FROZEN at its first frame with lives <= 0: the query stops there, while the checker goes on changing the
score of a finished Breakout or Amidar game that is stepped on.

batch(lib, game, n) makes the input of every test; expected(lib, game, states, sim_rngs, schedule) the answer."""
import numpy as np

from fork_replay import Raw, sim_rngs
from support import LEGAL, splitmix64
from toybox_amd import Engine, _abi

FIELDS = ("ret", "score", "lives", "frames_run", "life_lost_at")
MAX_FRAMES = 1024


def batch(lib, game, n, frames=400):
    """the input recipe: seeds 1234 + 7 i, a new game, `frames` synthetic frames with auto-reset, then lives = 1 where i % 3 != 0
    (GridWorld has no lives to edit).  lib None: the engine under test on the device."""
    case = Raw(game, n, lives_one=False)
    e = case.make(lib)
    case.run(e, 0, frames)
    if game != "gridworld":
        e.edit(_abi.EDIT_SET_LIVES, [1], mask=case.lives_mask)
    return e


def clone(lib, game, states, rngs):
    """a fresh checker engine that holds these state records and simulator RNGs"""
    e = Engine(game, len(states), lib=lib)
    e.set_states(0, states)
    for i, r in enumerate(np.asarray(rngs, np.uint64)):
        e.set_sim_rng((int(r[0]), int(r[1])), env=i)
    return e


def clone_of(lib, e):
    return clone(lib, e.game, e.get_states(), sim_rngs(e))


def _col(v, n, dtype=np.int64):
    return np.broadcast_to(np.asarray(v, dtype), (n,)).copy()


def schedule_columns(n, frames, hold=1, first=-1, rest=-1, seed=0, t=0, env_offset=0):
    """every column of a schedule as an array [n] (None: -1)"""
    return dict(frames=_col(frames, n), hold=_col(hold, n), first=_col(-1 if first is None else first, n), rest=_col(-1 if rest is None else rest, n),
                seed=_col(seed, n, np.uint64), t=_col(t, n, np.uint64), env_offset=_col(env_offset, n, np.uint64))


def valid_rows(game, s):
    ok = lambda a: (a == -1) | np.isin(a, LEGAL[game])
    return (s["frames"] >= 1) & (s["frames"] <= MAX_FRAMES) & (s["hold"] >= 1) & ok(s["first"]) & ok(s["rest"])


def actions_at(game, s, j):
    """the ALE action of frame j for every env: period p = j // hold plays first (p = 0) or rest; -1 = the synthetic rule with
    counter t + p"""
    n = len(s["frames"])
    legal = np.asarray(LEGAL[game], np.int32)
    p = (j // np.maximum(s["hold"], 1)).astype(np.uint64)
    env = s["env_offset"] + np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = splitmix64(s["seed"] ^ (env << np.uint64(32)) ^ (s["t"] + p))
    drawn = legal[(h % np.uint64(len(legal))).astype(np.int64)]
    a = np.where(p == 0, s["first"], s["rest"])
    return np.where(a < 0, drawn, a).astype(np.int32)


def play(e, game, s):
    """the five fields [n] of the schedule s (schedule_columns) played on the checker engine e, which is stepped in place; a
    refused row is five zeros"""
    n = e.n_envs
    ok = valid_rows(game, s)
    score0, lives0, _, _ = e.scalars()
    prev, lives0 = score0.astype(np.int64), lives0.astype(np.int64)
    ret, run, lost = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    score, lives = prev.copy(), lives0.copy()
    live = ok.copy()                                          # rows that still run
    horizon = int(s["frames"][ok].max()) if ok.any() else 0
    for j in range(horizon):
        live &= j < s["frames"]
        if not live.any():
            break
        a = np.where(ok, actions_at(game, s, j), 0).astype(np.int32)
        _, _, step_lives, step_score = e.step(a, auto_reset=False)
        sc, lv, _, _ = e.scalars()
        assert np.array_equal(sc, step_score) and np.array_equal(lv, step_lives), "the checker's scalars and step outputs disagree"
        sc, lv = sc.astype(np.int64), lv.astype(np.int64)
        ret[live] += np.maximum(sc - prev, 0)[live]
        prev[live], score[live], lives[live] = sc[live], sc[live], lv[live]
        lost[live & (lost < 0) & (lv < lives0)] = j
        run[live] = j + 1
        live &= lv > 0                                        # the freeze: nothing after the first frame with lives <= 0 counts
    out = dict(ret=ret.astype(np.float64), score=score, lives=lives, frames_run=run, life_lost_at=lost)
    for k in out:
        out[k][~ok] = 0
    return out


def expected(lib, game, states, rngs, schedule, all_actions=False):
    """schedule: the keyword arguments of schedule_columns.  -> dict of the five fields, [n] or (all_actions: candidate a plays
    LEGAL[game][a] first) [n, n_legal]"""
    n = len(states)
    if not all_actions:
        e = clone(lib, game, states, rngs)
        out = play(e, game, schedule_columns(n, **schedule))
        e.close()
        return out
    cols = []
    for a in LEGAL[game]:
        e = clone(lib, game, states, rngs)
        cols.append(play(e, game, schedule_columns(n, **dict(schedule, first=a))))
        e.close()
    return {k: np.stack([c[k] for c in cols], axis=1) for k in FIELDS}


def coverage(exp, frames):
    """the coverage conditions on expected arrays: which of them at least one row meets"""
    frames = np.broadcast_to(np.asarray(frames).reshape((-1,) + (1,) * (exp["lives"].ndim - 1)) if np.ndim(frames) else frames, exp["lives"].shape)
    ran = exp["frames_run"] > 0
    return dict(ended=bool((ran & (exp["lives"] <= 0)).any()), full=bool((ran & (exp["lives"] > 0) & (exp["frames_run"] == frames)).any()),
                scored=bool((exp["ret"] > 0).any()), lost_not_ended=bool(((exp["life_lost_at"] >= 0) & (exp["lives"] > 0)).any()))


def merge_coverage(total, cov):
    for k, v in cov.items():
        total[k] = total.get(k, False) or v
    return total


def assert_coverage(game, total):
    need = ["ended", "full", "scored"] + ([] if game == "gridworld" else ["lost_not_ended"])
    missing = [k for k in need if not total.get(k)]
    assert not missing, "%s: the cases together never show: %s" % (game, ", ".join(missing))


def assert_fields_equal(got, want, what):
    for k in FIELDS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            i = tuple(bad[0])
            raise AssertionError("%s: %s differs in %d entries, first at %s: got %r, want %r" % (what, k, len(bad), i, g[i], w[i]))
