"""The yardstick of the plan and search tests (TBX_QUERY_LOOKAHEAD_PLAN / _SEARCH, include/toybox_amd.h): CLONE AND PLAY, as in
tests/lookahead_replay.py, with a plan as the action source.

play_plan steps a checker clone frame by frame with the plan's actions (period p = j // hold plays digit p of the code while
p < depth, `rest` after that) under the same freeze rule; expected_search plays ALL n_legal ** depth codes that way and picks the
winner of every (env, first action) group with a numpy lexicographic sort -- nothing of the device's way of cutting the work up
(chunks, launches, the running best) appears here."""
import numpy as np

from lookahead_replay import FIELDS, MAX_FRAMES, batch, clone, schedule_columns  # noqa: F401  (batch: re-exported for the tests)
from support import LEGAL, splitmix64
from toybox_amd import _abi

SEARCH_FIELDS = FIELDS + ("code",)
MAX_PLANS = 4096
NO_LOSS = MAX_FRAMES + 1
# the search cases of tests/test_gpu_search.py: (envs, frames, hold, depth, frames of synthetic play behind the batch); rest = the
# game's first legal action.  The first case of every game is the one whose coverage figures the GPU module's docstring quotes.
SEARCH_CASES = {"breakout": [(96, 200, 8, 3, 400), (24, 160, 4, 4, 400)], "space_invaders": [(24, 96, 8, 2, 400), (12, 120, 8, 3, 400)],
                "amidar": [(96, 128, 4, 2, 900), (96, 240, 8, 3, 400)], "gridworld": [(96, 40, 2, 4, 40)]}
# ... and one per game with drawn rest actions, a seed above 32 bits and a counter and env offset that are not 0
DRAWN_CASE = dict(n=24, frames=64, hold=4, depth=2, rest=-1, seed=(0xABCDE << 32) | 0x1234567, t=2 ** 32 - 3, env_offset=70000, batch_frames=400)


def case_search(game, case):
    n, frames, hold, depth, _ = case
    return dict(frames=frames, hold=hold, depth=depth, rest=LEGAL[game][0])


def plan_columns(n, frames, hold=1, depth=0, code=0, rest=-1, seed=0, t=0, env_offset=0):
    """every column of a plan row as an array [n]"""
    s = schedule_columns(n, frames, hold=hold, rest=rest, seed=seed, t=t, env_offset=env_offset)
    del s["first"]
    s["depth"] = np.broadcast_to(np.asarray(depth, np.int64), (n,)).copy()
    s["code"] = np.broadcast_to(np.asarray(code, np.int64), (n,)).copy()
    return s


def valid_plan_rows(game, s):
    legal = LEGAL[game]
    ok_rest = (s["rest"] == -1) | np.isin(s["rest"], legal)
    ok = (s["frames"] >= 1) & (s["frames"] <= MAX_FRAMES) & (s["hold"] >= 1) & (s["depth"] >= 0) & (s["depth"] <= _abi.PLAN_MAX_DEPTH[game]) & ok_rest
    count = np.array([len(legal) ** int(d) if o else 0 for d, o in zip(s["depth"], ok)], dtype=object)
    return ok & np.array([0 <= int(c) < int(k) for c, k in zip(s["code"], count)], bool)


def plan_actions_table(game, s, horizon):
    """the ALE action of every frame j < horizon for every env, [horizon, n]"""
    n = len(s["frames"])
    legal = np.asarray(LEGAL[game], np.int32)
    L = len(legal)
    p = np.arange(horizon, dtype=np.int64)[:, None] // np.maximum(s["hold"], 1)[None, :]
    rest = np.broadcast_to(s["rest"], p.shape)
    if (s["rest"] < 0).any():
        env = s["env_offset"] + np.arange(n, dtype=np.uint64)
        with np.errstate(over="ignore"):
            h = splitmix64((s["seed"] ^ (env << np.uint64(32)))[None, :] ^ (s["t"][None, :] + p.astype(np.uint64)))
        rest = np.where(rest < 0, legal[(h % np.uint64(L)).astype(np.int64)], rest)
    digit = (np.clip(s["code"], 0, 2 ** 32)[None, :] // np.int64(L) ** np.clip(p, 0, 15)) % L      # (used where p < depth <= 16 only)
    return np.where(p < s["depth"][None, :], legal[digit], rest).astype(np.int32)


def play_plan(e, game, s, ok=None):
    """the five fields [n] of the plan rows s (plan_columns) played on the checker engine e, which is stepped in place; a refused
    row is five zeros"""
    n = e.n_envs
    ok = valid_plan_rows(game, s) if ok is None else ok
    score0, lives0, _, _ = e.scalars()
    prev, lives0 = score0.astype(np.int64), lives0.astype(np.int64)
    ret, run, lost = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    score, lives = prev.copy(), lives0.copy()
    live = ok.copy()
    horizon = int(s["frames"][ok].max()) if ok.any() else 0
    actions = np.ascontiguousarray(np.where(ok[None, :], plan_actions_table(game, s, horizon), 0).astype(np.int32))
    for j in range(horizon):
        live &= j < s["frames"]
        if not live.any():
            break
        e.step(actions[j], auto_reset=False)
        sc, lv, _, _ = e.scalars()
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


def expected_plan(lib, game, states, rngs, plan):
    """plan: the keyword arguments of plan_columns -> dict of the five fields [n]"""
    e = clone(lib, game, states, rngs)
    out = play_plan(e, game, plan_columns(len(states), **plan))
    e.close()
    return out


def play_all_codes(lib, game, states, rngs, search):
    """search: frames, hold, depth, rest, seed, t, env_offset (depth a scalar or one per env).  -> (leaves, ok): leaves a dict of the
    five fields [n, n_legal ** max depth] (a code beyond an env's own depth: untouched zeros), ok bool [n] the rows that are valid
    search rows apart from the objective"""
    n, L = len(states), len(LEGAL[game])
    sched = {k: v for k, v in search.items() if k != "objective"}
    s = plan_columns(n, **dict(sched, code=0))
    ok = valid_plan_rows(game, s) & (s["depth"] >= 1)
    ok &= np.array([L ** int(d) <= MAX_PLANS if o else False for d, o in zip(s["depth"], ok)], bool)
    top = int(s["depth"][ok].max()) if ok.any() else 0
    leaves = {k: np.zeros((n, L ** top), np.float64 if k == "ret" else np.int64) for k in FIELDS}
    for code in range(L ** top if ok.any() else 0):
        mine = ok & np.array([code < L ** int(d) if o else False for d, o in zip(s["depth"], ok)], bool)
        e = clone(lib, game, states, rngs)
        row = play_plan(e, game, dict(s, code=np.full(n, code, np.int64)), ok=mine)
        e.close()
        for k in FIELDS:
            leaves[k][mine, code] = row[k][mine]
    return leaves, ok, s["depth"]


def pick(game, leaves, ok, depth, objective):
    """the winner of every (env, first action) group of played leaves under `objective` (0 / 1, a scalar or one per env; any other
    value refuses the row): dict of the five fields and code, each [n, n_legal]"""
    n, L = len(ok), len(LEGAL[game])
    objective = np.broadcast_to(np.asarray(objective, np.int64), (n,))
    out = {k: np.zeros((n, L), np.float64 if k == "ret" else np.int64) for k in SEARCH_FIELDS}
    for i in range(n):
        if not ok[i] or objective[i] not in (0, 1):
            continue
        codes = np.arange(L ** int(depth[i]))
        ret, lives = leaves["ret"][i, codes], leaves["lives"][i, codes]
        loss = np.where(leaves["life_lost_at"][i, codes] < 0, NO_LOSS, leaves["life_lost_at"][i, codes])
        keys = (ret, lives, loss) if objective[i] == 0 else (lives, loss, ret)
        for a in range(L):
            grp = codes[codes % L == a]
            # np.lexsort sorts by its LAST key first: the code breaks the last tie, larger-is-better keys are negated
            order = np.lexsort((grp,) + tuple(-np.asarray(k[grp], np.float64) for k in reversed(keys)))
            best = grp[order[0]]
            for k in FIELDS:
                out[k][i, a] = leaves[k][i, best]
            out["code"][i, a] = best
    return out


def expected_search(lib, game, states, rngs, search):
    """search: frames, hold, depth, objective, rest, seed, t, env_offset -> the winners [n, n_legal] (pick) of all codes played"""
    leaves, ok, depth = play_all_codes(lib, game, states, rngs, search)
    return pick(game, leaves, ok, depth, search.get("objective", 0))


def group_stats(game, leaves, ok, depth):
    """what the coverage conditions count, over the (env, first action) groups of played leaves: groups whose winner under the
    return objective is not their smallest code, groups won on the tie-break (two or more plans equal in ret, lives and loss at the
    top), groups where the two objectives choose different plans, envs with a leaf that ended the game, and whether any ret > 0"""
    L = len(LEGAL[game])
    by_ret, by_life = pick(game, leaves, ok, depth, 0), pick(game, leaves, ok, depth, 1)
    not_first = ties = 0
    for i in np.flatnonzero(ok):
        codes = np.arange(L ** int(depth[i]))
        loss = np.where(leaves["life_lost_at"][i, codes] < 0, NO_LOSS, leaves["life_lost_at"][i, codes])
        for a in range(L):
            grp = codes[codes % L == a]
            w = by_ret["code"][i, a]
            not_first += int(w != grp[0])
            same = (leaves["ret"][i, grp] == leaves["ret"][i, w]) & (leaves["lives"][i, grp] == leaves["lives"][i, w]) & (loss[grp] == loss[w])
            ties += int(same.sum() >= 2)
    okm = ok[:, None]
    return dict(winner_not_first=not_first, ties=ties, disagree=int(((by_ret["code"] != by_life["code"]) & okm).sum()),
                ended_envs=int((((leaves["lives"] <= 0) & (leaves["frames_run"] > 0)).any(axis=1) & ok).sum()), scored=bool((leaves["ret"] > 0).any()))


def assert_search_equal(got, want, what):
    for k in SEARCH_FIELDS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g.astype(np.float64), w.astype(np.float64)):
            bad = np.argwhere(g.astype(np.float64) != w.astype(np.float64))
            i = tuple(bad[0])
            raise AssertionError("%s: %s differs in %d entries, first at %s: got %r, want %r" % (what, k, len(bad), i, g[i], w[i]))
