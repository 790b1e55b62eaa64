"""The yardstick of the tree-search tests (TBX_QUERY_LOOKAHEAD_TREE, include/toybox_amd.h): SELECT IN PYTHON INTEGERS, CLONE, SALT
AND PLAY, simulation by simulation.

The tree, the selection, the backup and the principal variation are written here from the header's text alone, in Python integers
(math.isqrt); nothing of the product is imported beyond what tests/sample_replay.py imports.  Per simulation m all L trees of all
envs are played at once on ONE checker clone that holds the batch L times over (evolve_replay._tiled's idea: copy a of env i plays
tree a of env i), with per-env depth and code columns through search_replay.play_plan, the game RNG of future m put into the
records by sample_replay.salted and the seed of future m into the seed column.  Nothing of the device's scratch, env ranges or
launch cuts appears here.  Beside the rows expected_tree returns the per-simulation log -- code, depth, value, and how every
selection step was decided -- and tree_stats counts the coverage conditions on it."""
import math

import numpy as np

from evolve_replay import _tiled
from sample_replay import salted
from search_replay import plan_columns, play_plan, valid_plan_rows
from support import LEGAL
from toybox_amd.engine import SAMPLE_FIELDS

QUERY, MAX_SIMULATIONS, MAX_EXPLORE, OPT_RANGES, OPT_LAUNCH_SIMULATIONS = 160, 1024, 1048576, 115, 116
M64 = (1 << 64) - 1
TREE_FIELDS = SAMPLE_FIELDS + ("code", "pv_depth", "pv_visits", "pv_value")
# frames of synthetic play behind the batch of every case (tests/lookahead_replay.py batch()): chosen on the checker so that the
# cases of a game together meet the coverage conditions below
BATCH_FRAMES = {"breakout": 400, "space_invaders": 400, "amidar": 400, "gridworld": 40}
HOLD = {"breakout": 4, "space_invaders": 4, "amidar": 4, "gridworld": 2}
ENVS = 24
# the `drawn` case: evolve_replay.DRAWN_EVOLVE's seed above 32 bits, a counter that leaves 32 bits and an env offset, with a salt
DRAWN_TREE = dict(rest=-1, seed=(0xABCDE << 32) | 0x1234567, t=2 ** 32 - 3, env_offset=70000, salt=1000, objective=1)
# the explore of the `tree` case that changes a played code against explore 0 (tests/test_tree.py asserts the difference): in
# units of the value -- returns are tens to hundreds, safe frames up to the horizon
EXPLORE = {"breakout": 64, "space_invaders": 64, "amidar": 64, "gridworld": 64}


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def case_tree(game, name):
    """the keyword arguments of expected_tree for the case `name` of `game`: tree / tree_explore (depth 3, M = 12 L, explore 0 /
    EXPLORE), drawn, deepest (depth TBX_PLAN_MAX_DEPTH, frames = hold x depth, M = L x depth + 8); rest = the game's first legal
    action where it is not drawn"""
    from toybox_amd import _abi
    L, hold = len(LEGAL[game]), HOLD[game]
    base = dict(frames=hold * 12, hold=hold, depth=3, simulations=12 * L, explore=0, rest=LEGAL[game][0], seed=77)
    if name == "tree":
        return base
    if name == "tree_explore":
        return dict(base, explore=EXPLORE[game])
    if name == "drawn":
        return dict(base, explore=EXPLORE[game], **DRAWN_TREE)
    if name == "deepest":
        depth = _abi.PLAN_MAX_DEPTH[game]
        return dict(base, depth=depth, frames=hold * depth, simulations=L * depth + 8)
    raise KeyError(name)


CASES = ("tree", "tree_explore", "drawn", "deepest")


class Node:
    __slots__ = ("n", "v_sum", "child")

    def __init__(self, L):
        self.n, self.v_sum, self.child = 0, 0, [None] * L


def select(nodes, L, a, depth, explore):
    """one selection in the tree `nodes` (a list in creation order, nodes[0] the root) of first action a -> (d, code, steps):
    steps a list of ("absent", k) / ("priority", k, tie) in path order; an expansion appends its node to `nodes`"""
    cur, d, code, steps = nodes[0], 1, a, []
    while d < depth:
        missing = [k for k in range(L) if cur.child[k] is None]
        if missing:
            k = missing[0]
            cur.child[k] = len(nodes)
            nodes.append(Node(L))
            code += k * L ** d
            d += 1
            steps.append(("absent", k))
            break
        root = math.isqrt(cur.n << 16)
        P = []
        for k in range(L):
            c = nodes[cur.child[k]]
            P.append((c.v_sum * 256) // c.n + (explore * root) // (1 + c.n))
            assert 0 <= P[-1] < 1 << 60
        k = max(range(L), key=lambda j: (P[j], -j))
        steps.append(("priority", k, sorted(P)[-1] == sorted(P)[-2]))
        code += k * L ** d
        d += 1
        cur = nodes[cur.child[k]]
    return d, code, steps


def backup(nodes, L, d, code, v):
    cur = nodes[0]
    for level in range(1, d + 1):
        cur.n += 1
        cur.v_sum += v
        if level < d:
            cur = nodes[cur.child[code // L ** level % L]]


def principal_variation(nodes, L, a):
    """-> (code, depth, n, v_sum, tie_steps): from the root to the child with the largest n, then the larger v_sum, then the smaller
    k, while there is a child; tie_steps counts the steps where two children share the largest n"""
    cur, d, code, ties = nodes[0], 1, a, 0
    while any(c is not None for c in cur.child):
        kids = [k for k in range(L) if cur.child[k] is not None]
        k = max(kids, key=lambda j: (nodes[cur.child[j]].n, nodes[cur.child[j]].v_sum, -j))
        ties += sum(nodes[cur.child[j]].n == nodes[cur.child[k]].n for j in kids) > 1
        code += k * L ** d
        d += 1
        cur = nodes[cur.child[k]]
    return code, d, cur.n, cur.v_sum, ties


def _col(n, v, default):
    return np.broadcast_to(np.asarray(default if v is None else v, np.int64), (n,)).copy()


def expected_tree(lib, game, states, rngs, tree):
    """tree: frames, hold, depth, objective, rest, seed, t, env_offset, simulations, explore, salt (scalars, or one value per env)
    -> (rows, log, trees).  rows: the twelve fields, each int64 [n, n_legal]; a refused env answers zeros.  log[m]: dict of code,
    depth, value, active (the simulation exists), absent (it ended in an expansion), priority and ties (its steps decided by
    priority among a full set of children, and those of them whose two best priorities tie), ended (its game ended) and ret, each
    [n, n_legal].  trees[i][a]: the nodes of the final tree (None: a refused env)."""
    n, L = len(states), len(LEGAL[game])
    own = ("objective", "simulations", "explore", "salt")
    s = plan_columns(n, **dict({k: v for k, v in tree.items() if k not in own}, code=0))
    objective, M, explore, salt = (_col(n, tree.get(k), d) for k, d in (("objective", 0), ("simulations", 1), ("explore", 0), ("salt", 0)))
    depth = s["depth"]
    ok = valid_plan_rows(game, s) & (depth >= 1) & np.isin(objective, (0, 1)) & (M >= 1) & (M <= MAX_SIMULATIONS) & (explore >= 0) & (explore <= MAX_EXPLORE)
    ok &= (salt >= 0) & (salt < 2 ** 32) & ((salt == 0) | (salt + M - 1 < 2 ** 32))
    rows = {k: np.zeros((n, L), np.int64) for k in TREE_FIELDS}
    trees = [[[Node(L)] for _ in range(L)] if ok[i] else None for i in range(n)]
    log = []
    for m in range(int(M[ok].max()) if ok.any() else 0):
        active = ok & (m < M)
        entry = {k: np.zeros((n, L), np.int64) for k in ("code", "depth", "value", "priority", "ties", "ret")}
        entry.update(active=np.broadcast_to(active[:, None], (n, L)).copy(), absent=np.zeros((n, L), bool), ended=np.zeros((n, L), bool))
        for i in np.flatnonzero(active):
            for a in range(L):
                d, code, steps = select(trees[i][a], L, a, int(depth[i]), int(explore[i]))
                entry["depth"][i, a], entry["code"][i, a] = d, code
                entry["absent"][i, a] = bool(steps) and steps[-1][0] == "absent"
                entry["priority"][i, a] = sum(st[0] == "priority" for st in steps)
                entry["ties"][i, a] = sum(st[0] == "priority" and st[2] for st in steps)
        s_m = dict(s, seed=np.array([splitmix64((int(x) + m) & M64) for x in s["seed"]], np.uint64))
        records = salted(game, states, np.where(active & (salt != 0), salt + m, 0))
        e, tiled = _tiled(lib, game, records, rngs, s_m, L)
        tiled["depth"], tiled["code"] = np.where(entry["active"], entry["depth"], 0).T.reshape(-1), np.where(entry["active"], entry["code"], 0).T.reshape(-1)
        f = play_plan(e, game, tiled, ok=np.tile(active, L))
        e.close()
        f = {k: np.asarray(v).astype(np.int64).reshape(L, n).T for k, v in f.items()}
        safe = np.where(f["life_lost_at"] < 0, f["frames_run"], f["life_lost_at"])
        entry["value"] = np.where(objective[:, None] == 0, f["ret"], safe) * entry["active"]
        entry["ended"], entry["ret"] = entry["active"] & (f["lives"] <= 0), f["ret"] * entry["active"]
        for i in np.flatnonzero(active):
            for a in range(L):
                backup(trees[i][a], L, int(entry["depth"][i, a]), int(entry["code"][i, a]), int(entry["value"][i, a]))
        on = entry["active"]
        first = on & (rows["samples"] == 0)
        rows["ret_min"] = np.where(on & (first | (f["ret"] < rows["ret_min"])), f["ret"], rows["ret_min"])
        rows["ret_max"] = np.where(on & (first | (f["ret"] > rows["ret_max"])), f["ret"], rows["ret_max"])
        rows["samples"] += on
        rows["ret_sum"] += np.where(on, f["ret"], 0)
        rows["lives_sum"] += np.where(on, f["lives"], 0)
        rows["lost"] += on & (f["life_lost_at"] >= 0)
        rows["ended"] += on & (f["lives"] <= 0)
        rows["safe_frames_sum"] += np.where(on, safe, 0)
        log.append(entry)
    for i in np.flatnonzero(ok):
        for a in range(L):
            rows["code"][i, a], rows["pv_depth"][i, a], rows["pv_visits"][i, a], rows["pv_value"][i, a], _ = principal_variation(trees[i][a], L, a)
    return rows, log, trees


def tree_stats(game, rows, log, trees, depth):
    """what the coverage conditions count over the replay of a case (depth: a scalar, or one per env): priority -- selection steps
    decided by priority among a full set of children; ties -- those of them whose two best priorities tie; full_depth --
    simulations that reach d == depth and expand nothing; pv_ties -- principal-variation steps decided by the v_sum or k tie-break;
    pv_full -- rows whose pv_depth is the case's depth; ended -- simulations whose game ends; scored -- simulations with a
    return above 0"""
    n, L = rows["samples"].shape
    depth = np.broadcast_to(depth, (n,))
    out = dict(priority=0, ties=0, full_depth=0, pv_ties=0, pv_full=0, ended=0, scored=0)
    for entry in log:
        on = entry["active"]
        out["priority"] += int(entry["priority"][on].sum())
        out["ties"] += int(entry["ties"][on].sum())
        out["full_depth"] += int((on & ~entry["absent"] & (entry["depth"] == depth[:, None]) & (depth[:, None] >= 2)).sum())
        out["ended"] += int(entry["ended"].sum())
        out["scored"] += int((entry["ret"] > 0).sum())
    for i in range(n):
        for a in range(L):
            if trees[i] is not None:
                out["pv_ties"] += principal_variation(trees[i][a], L, a)[4]
    out["pv_full"] = int(((rows["samples"] > 0) & (rows["pv_depth"] == depth[:, None])).sum())
    return out


def played_codes_differ(log_a, log_b):
    """simulations whose played (code, depth) differ between two replays of one batch -- the case pair of condition 4"""
    return sum(int((x["active"] & ((x["code"] != y["code"]) | (x["depth"] != y["depth"]))).sum()) for x, y in zip(log_a, log_b))


# 1 priority, 2 ties, 3 full_depth, 4 explore_changes (the tree / tree_explore pair), 5 pv_ties, 6 pv_full (at the deepest case),
# 7 ended, 8 scored
COVERAGE = ("priority", "ties", "full_depth", "explore_changes", "pv_ties", "pv_full", "ended", "scored")
# a condition a game cannot meet, and why in one line; no condition is dropped for more than one game
ALLOWED_MISSING = {}


def missing_coverage(game, totals):
    """the conditions that the summed counts of a game's cases do not meet"""
    return [k for k in COVERAGE if not totals.get(k) and k not in ALLOWED_MISSING.get(game, {})]


def assert_tree_equal(got, want, what):
    for k in TREE_FIELDS:
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            i = tuple(bad[0])
            raise AssertionError("%s: %s differs in %d entries, first at %s: got %r, want %r" % (what, k, len(bad), i, g[i], w[i]))
