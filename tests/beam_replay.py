"""The yardstick of the beam tests (TBX_QUERY_LOOKAHEAD_BEAM, include/toybox_amd.h): CLONE AND PLAY LEVEL BY LEVEL, built from
search_replay.play_plan and plan_columns.

Level d of first action a: the candidates are the kept prefixes of level d - 1, each extended by every digit (level 1: the one
prefix {a}); candidate j of every env is played at once on ONE checker clone with per-env codes and depth d (rest from period d
on), and the kept set is the first min(width, candidates) of a numpy lexicographic sort per (env, first action) group.  Nothing of
the device's slots, env ranges or scratch appears here.  Beside the rows, expected_beam returns every level's candidate set and
kept set, which the coverage conditions count (beam_stats)."""
import numpy as np

from lookahead_replay import FIELDS, clone
from search_replay import NO_LOSS, SEARCH_FIELDS, plan_columns, play_plan, valid_plan_rows
from support import LEGAL

MAX_WIDTH = 64
# the cases of tests/test_gpu_beam.py: (envs, frames, hold, depth, width, frames of synthetic play behind the batch); rest = the
# game's first legal action.  Per game: the deep case (a depth no enumeration reaches), the shallow-narrow case (depth 3, width 1,
# within the enumeration cap) and, for Breakout, a width above n_legal whose early levels leave slots empty.
BEAM_CASES = {"breakout": [(24, 96, 8, 8, 3, 400), (96, 200, 8, 3, 1, 400), (24, 64, 4, 4, 8, 400)],
              "space_invaders": [(12, 96, 8, 6, 3, 400), (24, 96, 8, 3, 1, 400)],
              "amidar": [(24, 96, 4, 6, 3, 400), (96, 128, 8, 3, 1, 900)],
              "gridworld": [(24, 40, 2, 7, 4, 40), (96, 40, 2, 3, 1, 80)]}
# ... and one per game with drawn rest actions, a seed above 32 bits and a counter and env offset that are not 0
DRAWN_BEAM = dict(rest=-1, seed=(0xABCDE << 32) | 0x1234567, t=2 ** 32 - 3, env_offset=70000)


def case_beam(game, case):
    n, frames, hold, depth, width, _ = case
    return dict(frames=frames, hold=hold, depth=depth, width=width, rest=LEGAL[game][0])


def _keys(fields, objective):
    """the order's keys of candidates, larger is better, most significant first"""
    loss = np.where(fields["life_lost_at"] < 0, NO_LOSS, fields["life_lost_at"])
    return (fields["ret"], fields["lives"], loss) if objective == 0 else (fields["lives"], loss, fields["ret"])


def _order(fields, codes, objective):
    # np.lexsort sorts by its LAST key first: the code breaks the last tie, larger-is-better keys are negated
    return np.lexsort((codes,) + tuple(-np.asarray(k, np.float64) for k in reversed(_keys(fields, objective))))


def expected_beam(lib, game, states, rngs, beam):
    """beam: frames, hold, depth, objective, rest, seed, t, env_offset, width (scalars, or one value per env) -> (rows, levels).
    rows: the five fields and code, each [n, n_legal]; a refused env answers zeros.  levels[d - 1]: dict of code, valid, the five
    fields (each [n, n_legal, J], the candidates of level d in the order they were made) and kept ([n, n_legal, J] bool)."""
    n, L = len(states), len(LEGAL[game])
    sched = {k: v for k, v in beam.items() if k not in ("objective", "width")}
    s = plan_columns(n, **dict(sched, code=0))
    objective = np.broadcast_to(np.asarray(beam.get("objective", 0), np.int64), (n,))
    width = np.broadcast_to(np.asarray(beam.get("width", 1), np.int64), (n,))
    depth = s["depth"]
    ok = valid_plan_rows(game, s) & (depth >= 1) & np.isin(objective, (0, 1)) & (width >= 1) & (width <= MAX_WIDTH)
    rows = {k: np.zeros((n, L), np.float64 if k == "ret" else np.int64) for k in SEARCH_FIELDS}
    levels = []
    # the kept prefixes of the level before: codes [n, L, K] and how many of them there are per env
    kept_codes, kept_count = np.tile(np.arange(L, dtype=np.int64)[None, :, None], (n, 1, 1)), np.ones(n, np.int64)
    for d in range(1, (int(depth[ok].max()) if ok.any() else 0) + 1):
        on = ok & (depth >= d)
        if d == 1:
            cand, count = kept_codes, np.ones(n, np.int64)
        else:
            cand = (kept_codes[:, :, :, None] + np.arange(L, dtype=np.int64)[None, None, None, :] * L ** (d - 1)).reshape(n, L, -1)
            count = kept_count * L
        J = int(count[on].max())
        cand = cand[:, :, :J]
        valid = on[:, None, None] & (np.arange(J)[None, None, :] < count[:, None, None])
        valid = np.broadcast_to(valid, (n, L, J)).copy()
        level = {k: np.zeros((n, L, J), np.float64 if k == "ret" else np.int64) for k in FIELDS}
        for a in range(L):
            for j in range(J):
                mine = valid[:, a, j]
                if not mine.any():
                    continue
                e = clone(lib, game, states, rngs)
                row = play_plan(e, game, dict(s, depth=np.full(n, d, np.int64), code=np.where(mine, cand[:, a, j], 0)), ok=mine)
                e.close()
                for k in FIELDS:
                    level[k][mine, a, j] = row[k][mine]
        keep = np.minimum(width, count)
        kept = np.zeros((n, L, J), bool)
        nxt = np.zeros((n, L, int(keep[on].max())), np.int64)
        for i in np.flatnonzero(on):
            c = int(count[i])
            for a in range(L):
                order = _order({k: level[k][i, a, :c] for k in FIELDS}, cand[i, a, :c], int(objective[i]))
                kept[i, a, order[:keep[i]]] = True
                nxt[i, a, :keep[i]] = cand[i, a, order[:keep[i]]]
                if d == depth[i]:
                    for k in FIELDS:
                        rows[k][i, a] = level[k][i, a, order[0]]
                    rows["code"][i, a] = cand[i, a, order[0]]
        levels.append(dict(level, code=cand.copy(), valid=valid, kept=kept))
        kept_codes, kept_count = nxt, np.where(on, keep, 0)
    return rows, levels


def beam_stats(levels, objective, width, depth):
    """what the coverage conditions count over the (env, first action, level) groups of a replay with shared arguments:
    cut_ties -- groups where the last kept and the first dropped candidate are equal in ret, lives and loss (the code decides who
    stays); kept_not_prefix -- groups whose kept set is not the first `width` candidates in code order; winner_not_first -- final
    groups whose winner is not their smallest code; ended_envs -- envs with a candidate that ended the game; scored -- any ret > 0"""
    cut_ties = kept_not_prefix = winner_not_first = 0
    ended = np.zeros(levels[0]["valid"].shape[0], bool)
    scored = False
    for d, lv in enumerate(levels, 1):
        n, L, J = lv["valid"].shape
        ended |= (lv["valid"] & (lv["lives"] <= 0) & (lv["frames_run"] > 0)).any(axis=(1, 2))
        scored = scored or bool((lv["ret"][lv["valid"]] > 0).any())
        for i in range(n):
            for a in range(L):
                c = int(lv["valid"][i, a].sum())
                if not c:
                    continue
                f = {k: lv[k][i, a, :c] for k in FIELDS}
                codes = lv["code"][i, a, :c]
                order = _order(f, codes, objective)
                if d == depth:
                    winner_not_first += int(codes[order[0]] != codes.min())
                if c > width:
                    x, y = order[width - 1], order[width]
                    cut_ties += int(all(k[x] == k[y] for k in _keys(f, objective)))
                    kept_not_prefix += int(set(codes[order[:width]]) != set(np.sort(codes)[:width]))
    return dict(cut_ties=cut_ties, kept_not_prefix=kept_not_prefix, winner_not_first=winner_not_first, ended_envs=int(ended.sum()), scored=scored)


def not_worse(objective, x, y):
    """rows x are not worse than rows y under the order's keys (the code left out): bool, the shape of the rows"""
    kx, ky = _keys(x, objective), _keys(y, objective)
    better = np.zeros(np.shape(kx[0]), bool)
    equal = np.ones(np.shape(kx[0]), bool)
    for a, b in zip(kx, ky):
        better |= equal & (a > b)
        equal &= a == b
    return better | equal


def case_coverage(game, case, beam, search=None):
    """the coverage counts of one case: beam = {objective: (rows, levels)} of expected_beam under both objectives; search =
    {objective: rows} of search_replay.expected_search where the case stays within the enumeration cap.  worse / equal: groups
    whose beam row is strictly worse than / field for field the search's row; disagree: groups where the two objectives return
    different codes; the others: beam_stats, summed over the objectives"""
    _, _, _, depth, width, _ = case
    total = dict(worse=0, equal=0, disagree=int((beam[0][0]["code"] != beam[1][0]["code"]).sum()))
    for objective in (0, 1):
        rows, levels = beam[objective]
        for k, v in beam_stats(levels, objective, width, depth).items():
            total[k] = total.get(k, 0) + int(v)
        if search is not None:
            total["worse"] += int((~not_worse(objective, rows, search[objective])).sum())
            total["equal"] += int(np.all([np.asarray(rows[k], np.float64) == np.asarray(search[objective][k], np.float64) for k in SEARCH_FIELDS], axis=0).sum())
    return total


def missing_coverage(game, totals):
    """the conditions that the summed counts of a game's cases do not meet (GridWorld's two objectives need not disagree; every
    other condition holds for every game)"""
    need = ["worse", "equal", "cut_ties", "kept_not_prefix", "winner_not_first", "scored", "ended_envs"] + ([] if game == "gridworld" else ["disagree"])
    return [k for k in need if not totals.get(k)]
