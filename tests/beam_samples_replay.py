"""The yardstick of the beam-over-samples tests (TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES, include/toybox_amd.h): per level, per candidate
and per sample SALT the records (tests/sample_replay.py: salted) and PLAY on ONE checker clone with per-env codes
(tests/search_replay.py: play_plan) under sample_seed(seed, s); sum the futures of every candidate with numpy integers; take the
kept set from a plain sort on the key the header states.  Every candidate of an env, at every level, meets the same futures: seed_s
and salt_s depend on s alone.  Nothing of the device's slots, sample chunks, env ranges or scratch appears here.  Beside the rows,
expected_beam_samples returns every level's candidates, sums and kept set, which the coverage conditions count (case_coverage)."""
import numpy as np

from lookahead_replay import clone
from sample_replay import LEAF_FIELDS, MAX_SAMPLES, salted
from search_replay import plan_columns, play_plan, valid_plan_rows
from search_samples_replay import BIG_SEED, BIG_T, ENV_OFFSET, MAX_LEAVES, ROW_FIELDS, aggregate, columns
from support import LEGAL
from toybox_amd.engine import SAMPLE_FIELDS, sample_seed

MAX_WIDTH = 64
KEY_FIELDS = ("ret_sum", "lost", "safe_frames_sum")
# the cases of tests/test_gpu_beam_samples.py: (envs, frames, hold, depth, width, samples, salt, frames of synthetic play behind the
# batch), with rest = -1 and seed 77.  Per game the deep case (Breakout's 4^7 plans are beyond the search over samples) and the
# shallow-narrow case; GridWorld has no game RNG and goes unsalted.
CASES = {"breakout": [(24, 96, 8, 7, 2, 3, 1000, 400), (96, 200, 8, 3, 1, 3, 1000, 400)],
         "space_invaders": [(12, 96, 8, 5, 2, 2, 1000, 400), (24, 96, 8, 3, 1, 3, 1000, 400)],
         "amidar": [(24, 96, 4, 5, 2, 2, 1000, 400), (96, 128, 8, 3, 1, 3, 1000, 900)],
         "gridworld": [(24, 40, 2, 6, 2, 3, 0, 40), (96, 40, 2, 3, 1, 3, 0, 80)]}
# ... and what the drawn case of a game (its deep case) changes: a seed above 32 bits, a counter that leaves 32 bits, an env offset
DRAWN = dict(seed=BIG_SEED, t=BIG_T, env_offset=ENV_OFFSET)


def case_args(case):
    n, frames, hold, depth, width, samples, salt, _ = case
    return dict(frames=frames, hold=hold, depth=depth, width=width, samples=samples, salt=salt, rest=-1, seed=77)


def kept_count(legal, width, level):
    """|B_level|: 1, then min(width, legal * the level before)"""
    kept = 1
    for _ in range(2, level + 1):
        kept = min(width, kept * legal)
    return kept


def leaves_of(legal, width, depth, samples):
    """the candidates of the widest level (the last) of one env, over all first actions, times the samples"""
    return legal * kept_count(legal, width, depth - 1) * (1 if depth == 1 else legal) * samples


def valid_rows(game, c, width):
    """the rows the query answers: the beam's ranges, the sample count and salt ranges, and the leaf cap"""
    L = len(LEGAL[game])
    ok = valid_plan_rows(game, dict(c, code=np.zeros(len(width), np.int64))) & (c["depth"] >= 1) & ((c["objective"] == 0) | (c["objective"] == 1))
    ok &= (width >= 1) & (width <= MAX_WIDTH)
    ok &= (c["samples"] >= 1) & (c["samples"] <= MAX_SAMPLES) & (c["salt"] >= 0) & (c["salt"] < 2 ** 32)
    ok &= (c["salt"] == 0) | (c["salt"] + c["samples"] - 1 < 2 ** 32)
    return ok & np.array([bool(o) and leaves_of(L, int(w), int(d), int(s)) <= MAX_LEAVES for o, w, d, s in zip(ok, width, c["depth"], c["samples"])], bool)


def sort_key(sums, objective, code):
    """smaller is better: objective 0 the larger ret_sum, the smaller lost, the larger safe_frames_sum; objective 1 the smaller lost,
    the larger safe_frames_sum, the larger ret_sum; then the smaller code"""
    r, lo, sf = int(sums["ret_sum"]), int(sums["lost"]), int(sums["safe_frames_sum"])
    return ((-r, lo, -sf) if objective == 0 else (lo, -sf, -r)) + (int(code),)


def _ranked(sums, i, a, codes, objective):
    """the candidate indices of group (i, a) from the best to the worst: a plain sort on sort_key"""
    return sorted(range(len(codes)), key=lambda j: sort_key({k: sums[k][i, a, j] for k in KEY_FIELDS}, objective, codes[j]))


def expected_beam_samples(lib, game, states, rngs, case):
    """case: frames, depth, width, samples, hold, objective, salt, rest, seed, t, env_offset (scalars, or one value per env) ->
    (rows, levels).  rows: the eight sums and the code, each int64 [n, n_legal]; a refused env answers zeros.  levels[d - 1]: dict
    of code and valid [n, n_legal, J] (the candidates of level d in the order they were made), sums and alone (the eight sums of
    every candidate over all its futures / over future 0 alone, each [n, n_legal, J]) and kept ([n, n_legal, J] bool)."""
    n, L = len(states), len(LEGAL[game])
    c = columns(n, **{k: v for k, v in case.items() if k != "width"})
    width = np.broadcast_to(np.asarray(case.get("width", 1), np.int64), (n,)).copy()
    depth, objective, samples = c["depth"], c["objective"], c["samples"]
    ok = valid_rows(game, c, width)
    rows = {k: np.zeros((n, L), np.int64) for k in ROW_FIELDS}
    levels = []
    S = int(samples[ok].max()) if ok.any() else 0
    # the futures: records salted by salt_s, a plan row under seed_s -- the same for every candidate and level
    futures = []
    for s in range(S):
        active = ok & (s < samples)
        records = salted(game, states, np.where(active & (c["salt"] != 0), c["salt"] + s, 0))
        seed_s = np.array([sample_seed(int(x), s) for x in c["seed"]], np.uint64)
        futures.append((active, records, plan_columns(n, c["frames"], hold=c["hold"], rest=c["rest"], seed=seed_s, t=c["t"], env_offset=c["env_offset"])))
    kept_codes, kept_n = np.tile(np.arange(L, dtype=np.int64)[None, :, None], (n, 1, 1)), np.ones(n, np.int64)
    for d in range(1, (int(depth[ok].max()) if ok.any() else 0) + 1):
        on = ok & (depth >= d)
        if d == 1:
            cand, count = kept_codes, np.ones(n, np.int64)
        else:
            cand = (kept_codes[:, :, :, None] + np.arange(L, dtype=np.int64)[None, None, None, :] * L ** (d - 1)).reshape(n, L, -1)
            count = kept_n * L
        J = int(count[on].max())
        cand = cand[:, :, :J]
        valid = np.broadcast_to(on[:, None, None] & (np.arange(J)[None, None, :] < count[:, None, None]), (n, L, J)).copy()
        leaves = {k: np.zeros((S, n, L, J), np.int64) for k in LEAF_FIELDS}
        for s, (active, records, plan) in enumerate(futures):
            for a in range(L):
                for j in range(J):
                    mine = valid[:, a, j] & active
                    if not mine.any():
                        continue
                    e = clone(lib, game, records, rngs)
                    row = play_plan(e, game, dict(plan, depth=np.full(n, d, np.int64), code=np.where(mine, cand[:, a, j], 0)), ok=mine)
                    e.close()
                    for k in LEAF_FIELDS:
                        leaves[k][s, mine, a, j] = np.asarray(row[k]).astype(np.int64)[mine]
        flat = {k: v.reshape(S, n, L * J) for k, v in leaves.items()}
        act = np.array([f[0] & on for f in futures]).reshape(S, n)
        sums = {k: v.reshape(n, L, J) for k, v in aggregate(flat, act).items()}
        alone = {k: v.reshape(n, L, J) for k, v in aggregate(flat, act, order=[0]).items()}
        keep = np.minimum(width, count)
        kept = np.zeros((n, L, J), bool)
        nxt = np.zeros((n, L, int(keep[on].max())), np.int64)
        for i in np.flatnonzero(on):
            m = int(count[i])
            for a in range(L):
                order = _ranked(sums, i, a, cand[i, a, :m], int(objective[i]))
                kept[i, a, order[:keep[i]]] = True
                nxt[i, a, :keep[i]] = cand[i, a, order[:keep[i]]]
                if d == depth[i]:
                    for k in SAMPLE_FIELDS:
                        rows[k][i, a] = sums[k][i, a, order[0]]
                    rows["code"][i, a] = cand[i, a, order[0]]
        levels.append(dict(code=cand.copy(), valid=valid, sums=sums, alone=alone, kept=kept))
        kept_codes, kept_n = nxt, np.where(on, keep, 0)
    return rows, levels


def level_stats(levels, objective, width, depth):
    """what the coverage conditions count over the (env, first action, level) groups of a replay with shared arguments: cut_ties --
    groups whose last kept and first dropped candidate are equal in the three sums the order reads (the code alone decides who
    stays); kept_not_prefix -- groups whose kept set is not the first `width` codes; winner_not_first -- final groups whose winner
    is not their smallest code; spread -- candidates whose futures differ in their return; future0_differs -- groups whose kept
    set (where the level drops a candidate) or final winner under all futures is not the one under future 0 alone"""
    out = dict(cut_ties=0, kept_not_prefix=0, winner_not_first=0, spread=0, future0_differs=0)
    for d, lv in enumerate(levels, 1):
        n, L, J = lv["valid"].shape
        out["spread"] += int((lv["valid"] & (lv["sums"]["ret_min"] < lv["sums"]["ret_max"])).sum())
        for i in range(n):
            for a in range(L):
                m = int(lv["valid"][i, a].sum())
                if not m:
                    continue
                codes = lv["code"][i, a, :m]
                order, order0 = _ranked(lv["sums"], i, a, codes, objective), _ranked(lv["alone"], i, a, codes, objective)
                differs = False
                if d == depth:
                    out["winner_not_first"] += int(codes[order[0]] != codes.min())
                    differs = order[0] != order0[0]
                if m > width:
                    x, y = order[width - 1], order[width]
                    out["cut_ties"] += int(all(lv["sums"][k][i, a, x] == lv["sums"][k][i, a, y] for k in KEY_FIELDS))
                    out["kept_not_prefix"] += int(set(codes[order[:width]]) != set(np.sort(codes)[:width]))
                    differs = differs or set(order[:width]) != set(order0[:width])
                out["future0_differs"] += int(differs)
    return out


def case_coverage(case, replays):
    """the coverage counts of one case: replays = {objective: (rows, levels)} of expected_beam_samples under both objectives; the
    counts of level_stats summed over the objectives, and disagree: groups where the two objectives return different codes"""
    _, _, _, depth, width, _, _, _ = case
    total = dict(disagree=int((replays[0][0]["code"] != replays[1][0]["code"]).sum()))
    for objective in (0, 1):
        for k, v in level_stats(replays[objective][1], objective, width, depth).items():
            total[k] = total.get(k, 0) + int(v)
    return total


COVERAGE = ("cut_ties", "kept_not_prefix", "winner_not_first", "spread", "future0_differs", "disagree")


def missing_coverage(totals):
    """the conditions that the summed counts of a game's cases do not meet: each of the six must be above 0"""
    return [k for k in COVERAGE if not totals.get(k)]
