"""The yardstick of the search-over-samples tests (TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES, include/toybox_amd.h): for every sample s
SALT the records (tests/sample_replay.py: salted) and play ALL codes (tests/search_replay.py: play_all_codes) under
sample_seed(seed, s); then sum the futures of every plan with numpy in a given order and pick per (env, first action) with a plain
loop over the order the header states.  Every plan of an env meets the same futures: seed_s and salt_s depend on s alone.  Nothing
of the device's way of cutting the work up (chunks, launches, a running best, a second pass) appears here."""
import numpy as np

from lookahead_replay import FIELDS
from sample_replay import MAX_SAMPLES, salted
from search_replay import MAX_PLANS, play_all_codes
from support import LEGAL
from toybox_amd import _abi
from toybox_amd.engine import SAMPLE_FIELDS, sample_seed

MAX_LEAVES = 65536
ROW_FIELDS = SAMPLE_FIELDS + ("code",)
BIG_SEED, BIG_T, ENV_OFFSET = (0xABCDE << 32) | 0x1234567, 2 ** 32 - 3, 70000


def _col(v, n, dtype=np.int64):
    return np.broadcast_to(np.asarray(v, dtype), (n,)).copy()


def columns(n, frames, depth=1, samples=1, hold=1, objective=0, salt=0, rest=-1, seed=0, t=0, env_offset=0):
    """every column of a row as an array [n] (rest None: -1)"""
    return dict(frames=_col(frames, n), hold=_col(hold, n), depth=_col(depth, n), objective=_col(objective, n), rest=_col(-1 if rest is None else rest, n),
                seed=_col(seed, n, np.uint64), t=_col(t, n, np.uint64), env_offset=_col(env_offset, n, np.uint64), samples=_col(samples, n), salt=_col(salt, n))


def valid_rows(game, c):
    """the rows the query answers: the search's ranges, the sample count, the leaf cap and the salt ranges"""
    L = len(LEGAL[game])
    ok_rest = (c["rest"] == -1) | np.isin(c["rest"], LEGAL[game])
    ok = (c["frames"] >= 1) & (c["frames"] <= 1024) & (c["hold"] >= 1) & (c["depth"] >= 1) & (c["depth"] <= _abi.PLAN_MAX_DEPTH[game]) & ok_rest
    ok &= (c["objective"] == 0) | (c["objective"] == 1)
    ok &= (c["samples"] >= 1) & (c["samples"] <= MAX_SAMPLES) & (c["salt"] >= 0) & (c["salt"] < 2 ** 32)
    ok &= (c["salt"] == 0) | (c["salt"] + c["samples"] - 1 < 2 ** 32)
    plans = np.array([L ** int(d) if o else 0 for d, o in zip(c["depth"], ok)], dtype=object)
    return ok & np.array([int(p) <= MAX_PLANS and int(p) * int(s) <= MAX_LEAVES for p, s in zip(plans, c["samples"])], bool)


def play_all(lib, game, states, rngs, case):
    """case: the keyword arguments of columns.  -> (leaves, active, ok, depth): leaves a dict of ret, lives, frames_run,
    life_lost_at, each int64 [S, n, n_legal ** top] with S the largest sample count and top the largest depth of a valid row;
    active bool [S, n]: future s of env i is played; ok bool [n]: the valid rows"""
    n = len(states)
    c = columns(n, **case)
    ok = valid_rows(game, c)
    S = int(c["samples"][ok].max()) if ok.any() else 0
    leaves, active = None, np.zeros((S, n), bool)
    for s in range(S):
        active[s] = ok & (s < c["samples"])
        salt_s = np.where(active[s] & (c["salt"] != 0), c["salt"] + s, 0)
        records = salted(game, states, salt_s)
        search = {k: c[k].copy() for k in ("frames", "hold", "depth", "rest", "t", "env_offset")}
        search["seed"] = np.array([sample_seed(int(x), s) for x in c["seed"]], np.uint64)
        search["frames"][~active[s]] = 0                      # (a row that has no future s: refused by play_all_codes, never read)
        played, _, _ = play_all_codes(lib, game, records, rngs, search)
        if leaves is None:                                    # (sample 0 plays every valid row: its width is the widest)
            leaves = {k: np.zeros((S,) + played[k].shape, np.int64) for k in FIELDS}
        for k in FIELDS:
            leaves[k][s, :, :played[k].shape[1]] = played[k].astype(np.int64)
    if leaves is None:
        leaves = {k: np.zeros((0, n, 0), np.int64) for k in FIELDS}
    return leaves, active, ok, c["depth"]


def aggregate(leaves, active, order=None):
    """the eight sums of every plan, each int64 [n, codes], of the futures added one after the other in `order` (None: 0, 1, ...)"""
    S, n, codes = leaves["ret"].shape
    out = {k: np.zeros((n, codes), np.int64) for k in SAMPLE_FIELDS}
    first = np.ones((n, codes), bool)
    for s in (range(S) if order is None else order):
        on = np.broadcast_to(active[s][:, None], (n, codes))
        ret, lost_at = leaves["ret"][s], leaves["life_lost_at"][s]
        out["ret_min"] = np.where(on & (first | (ret < out["ret_min"])), ret, out["ret_min"])
        out["ret_max"] = np.where(on & (first | (ret > out["ret_max"])), ret, out["ret_max"])
        first = first & ~on
        out["samples"] += on
        out["ret_sum"] += np.where(on, ret, 0)
        out["lives_sum"] += np.where(on, leaves["lives"][s], 0)
        out["lost"] += on & (lost_at >= 0)
        out["ended"] += on & (leaves["lives"][s] <= 0)
        out["safe_frames_sum"] += np.where(on, np.where(lost_at < 0, leaves["frames_run"][s], lost_at), 0)
    return out


def plan_key(sums, i, code, objective):
    """smaller is better: objective 0 the larger ret_sum, the smaller lost, the larger safe_frames_sum; objective 1 the smaller
    lost, the larger safe_frames_sum, the larger ret_sum; then the smaller code"""
    r, lo, sf = int(sums["ret_sum"][i, code]), int(sums["lost"][i, code]), int(sums["safe_frames_sum"][i, code])
    return ((-r, lo, -sf) if objective == 0 else (lo, -sf, -r)) + (int(code),)


def pick(game, sums, ok, depth, objective):
    """the best plan of every (env, first action) group, a plain loop: dict of the eight sums and the code, each int64 [n, n_legal];
    a refused env is zeros"""
    n, L = len(ok), len(LEGAL[game])
    objective = np.broadcast_to(np.asarray(objective, np.int64), (n,))
    out = {k: np.zeros((n, L), np.int64) for k in ROW_FIELDS}
    for i in np.flatnonzero(ok):
        for a in range(L):
            best = None
            for code in range(a, L ** int(depth[i]), L):
                if best is None or plan_key(sums, i, code, objective[i]) < plan_key(sums, i, best, objective[i]):
                    best = code
            for k in SAMPLE_FIELDS:
                out[k][i, a] = sums[k][i, best]
            out["code"][i, a] = best
    return out


def expected_search_samples(lib, game, states, rngs, case):
    """case: frames, depth, samples, hold, objective, salt, rest, seed, t, env_offset (scalars or one per env) -> the rows [n, n_legal]"""
    leaves, active, ok, depth = play_all(lib, game, states, rngs, case)
    return pick(game, aggregate(leaves, active), ok, depth, case.get("objective", 0))


def group_stats(game, leaves, active, ok, depth):
    """what the coverage conditions count over the (env, first action) groups of played plans: groups whose winner under the return
    objective is not their smallest code, groups won on the code tie-break (two or more plans equal in the three sums at the top),
    groups where the two objectives pick different plans, plans whose futures differ in their return, and groups whose winner
    under all S futures is not their winner under future 0 alone (either objective)"""
    L = len(LEGAL[game])
    sums = aggregate(leaves, active)
    by_ret, by_life = pick(game, sums, ok, depth, 0), pick(game, sums, ok, depth, 1)
    alone = aggregate(leaves, active, order=[0] if len(active) else [])
    alone_ret, alone_life = pick(game, alone, ok, depth, 0), pick(game, alone, ok, depth, 1)
    not_first = ties = spread = 0
    for i in np.flatnonzero(ok):
        codes = np.arange(L ** int(depth[i]))
        spread += int((sums["ret_min"][i, codes] < sums["ret_max"][i, codes]).sum())
        for a in range(L):
            grp = codes[codes % L == a]
            w = by_ret["code"][i, a]
            not_first += int(w != grp[0])
            same = np.ones(len(grp), bool)
            for k in ("ret_sum", "lost", "safe_frames_sum"):
                same &= sums[k][i, grp] == sums[k][i, w]
            ties += int(same.sum() >= 2)
    okm = ok[:, None]
    return dict(groups=int(ok.sum()) * L, winner_not_first=not_first, ties=ties, disagree=int(((by_ret["code"] != by_life["code"]) & okm).sum()), spread_plans=spread,
                future0_differs=int((((by_ret["code"] != alone_ret["code"]) | (by_life["code"] != alone_life["code"])) & okm).sum()))


def assert_rows_equal(got, want, what):
    for k in ROW_FIELDS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g.astype(np.int64), w.astype(np.int64)):
            bad = np.argwhere(g.astype(np.int64) != w.astype(np.int64))
            i = tuple(bad[0])
            raise AssertionError("%s: %s differs in %d entries, first at %s: got %r, want %r" % (what, k, len(bad), i, g[i], w[i]))


# ---------------------------------------------------------------- the cases of tests/test_gpu_search_samples.py

# name -> (game, envs, frames, hold, depth, samples, salt, frames of synthetic play behind the batch): tests/lookahead_replay.py batch()
CASES = {"breakout-deep": ("breakout", 24, 96, 8, 3, 4, 0, 400), "breakout-wide": ("breakout", 96, 96, 8, 2, 8, 0, 400),
         "space_invaders": ("space_invaders", 12, 96, 8, 2, 5, 1000, 400), "amidar": ("amidar", 24, 96, 4, 2, 4, 0, 400),
         "gridworld": ("gridworld", 24, 24, 2, 3, 3, 0, 40)}
RESTS = ("fixed", "drawn")


def case_args(name, rest):
    """the keyword arguments of columns (without the objective) for a case: "fixed": rest = the game's second legal action, seed
    77; "drawn": rest = -1 under a seed above 32 bits, a counter that crosses 2^32 within the horizon and an env offset"""
    game, _, frames, hold, depth, samples, salt, _ = CASES[name]
    if rest == "fixed":
        return dict(frames=frames, hold=hold, depth=depth, samples=samples, salt=salt, rest=LEGAL[game][1], seed=77)
    assert BIG_T + (frames - 1) // hold >= 2 ** 32
    return dict(frames=frames, hold=hold, depth=depth, samples=samples, salt=salt, rest=-1, seed=BIG_SEED, t=BIG_T, env_offset=ENV_OFFSET)
