"""The yardstick of the tree-act tests (TBX_QUERY_LOOKAHEAD_TREE_ACT and TBX_EDIT_TREE_DROP, include/toybox_amd.h): START TREES,
SEARCH, PICK, CARRY, STEP.

Written from the header's text alone.  Selection, backup, the principal variation, the node and the seed word are those of
tests/tree_replay.py, imported unchanged; the play of a simulation is that module's too (one checker clone that holds the batch L
times over, salted, with per-env depth and code columns).  New here: the start trees (deep copies of what the store holds, where
it is live), the pick as a sort of tuples of Python integers, the carry -- the subtree's ids collected by a walk, sorted, cut to
`keep`, renumbered, halved -- the store with its key and the drop flags.  Nothing of the product's tree_carry, tree_act_args or
store reader is imported, and nothing of the device's scratch, ranges or launch cuts appears."""
import numpy as np

from evolve_replay import _tiled
from fork_replay import sim_rngs
from sample_replay import salted
from search_replay import plan_columns, play_plan
from support import LEGAL
from tree_replay import BATCH_FRAMES, DRAWN_TREE, ENVS, EXPLORE, HOLD, M64, TREE_FIELDS, Node, backup, principal_variation, select, splitmix64

QUERY, EDIT_DROP, BUF_PLAN_ACTION, BUF_PLAN_TREE, OPT_KEEP, OPT_MAX_VISITS = 161, 44, 17, 19, 117, 118
WIDTH, MAX_VISITS, MOST_ARGUMENTS = 14, 4096, 13


class Kept(Node):
    """a carried node: `cut` holds the digits whose link the carry dropped"""
    __slots__ = ("cut",)

    def __init__(self, L, n, v_sum):
        Node.__init__(self, L)
        self.n, self.v_sum, self.cut = n, v_sum, set()


def copy_tree(nodes, L):
    out = []
    for nd in nodes:
        c = Kept(L, nd.n, nd.v_sum)
        c.child, c.cut = list(nd.child), set(getattr(nd, "cut", ()))
        out.append(c)
    return out


def search(lib, game, states, rngs, tree, start):
    """step 2 on the start trees start[i][a] (lists of nodes, changed in place): tree_replay.expected_tree's loop for shared
    values.  -> (rows, log): the twelve fields [n, L]; log[m] with code, depth, absent and recut (the expansion refilled a link
    that a carry had dropped), each [n, L]"""
    n, L = len(states), len(LEGAL[game])
    s = plan_columns(n, **dict({k: v for k, v in tree.items() if k not in ("objective", "simulations", "explore", "salt")}, code=0))
    objective, M, explore, salt, depth = int(tree.get("objective", 0)), int(tree.get("simulations", 1)), int(tree.get("explore", 0)), int(tree.get("salt", 0)), int(tree["depth"])
    rows = {k: np.zeros((n, L), np.int64) for k in TREE_FIELDS}
    log = []
    for m in range(M):
        entry = {k: np.zeros((n, L), np.int64) for k in ("code", "depth")}
        entry.update(absent=np.zeros((n, L), bool), recut=np.zeros((n, L), bool))
        for i in range(n):
            for a in range(L):
                nodes = start[i][a]
                d, code, steps = select(nodes, L, a, depth, explore)
                entry["depth"][i, a], entry["code"][i, a] = d, code
                if steps and steps[-1][0] == "absent":
                    entry["absent"][i, a] = True
                    parent = nodes[0]
                    for level in range(1, d - 1):
                        parent = nodes[parent.child[code // L ** level % L]]
                    k = steps[-1][1]
                    if k in getattr(parent, "cut", ()):
                        entry["recut"][i, a] = True
                        parent.cut.discard(k)
        s_m = dict(s, seed=np.array([splitmix64((int(x) + m) & M64) for x in s["seed"]], np.uint64))
        records = salted(game, states, np.full(n, salt + m if salt else 0))
        e, tiled = _tiled(lib, game, records, rngs, s_m, L)
        tiled["depth"], tiled["code"] = entry["depth"].T.reshape(-1), entry["code"].T.reshape(-1)
        f = play_plan(e, game, tiled, ok=np.ones(n * L, bool))
        e.close()
        f = {k: np.asarray(v).astype(np.int64).reshape(L, n).T for k, v in f.items()}
        safe = np.where(f["life_lost_at"] < 0, f["frames_run"], f["life_lost_at"])
        value = f["ret"] if objective == 0 else safe
        for i in range(n):
            for a in range(L):
                backup(start[i][a], L, int(entry["depth"][i, a]), int(entry["code"][i, a]), int(value[i, a]))
        rows["ret_min"] = f["ret"].copy() if m == 0 else np.minimum(rows["ret_min"], f["ret"])
        rows["ret_max"] = f["ret"].copy() if m == 0 else np.maximum(rows["ret_max"], f["ret"])
        rows["samples"] += 1
        rows["ret_sum"] += f["ret"]
        rows["lives_sum"] += f["lives"]
        rows["lost"] += f["life_lost_at"] >= 0
        rows["ended"] += f["lives"] <= 0
        rows["safe_frames_sum"] += safe
        log.append(entry)
    for i in range(n):
        for a in range(L):
            rows["code"][i, a], rows["pv_depth"][i, a], rows["pv_visits"][i, a], rows["pv_value"][i, a], _ = principal_variation(start[i][a], L, a)
    return rows, log


def pick(rows, objective):
    """step 3: the winner a* of every env, the sampled planners' order as a sort of tuples of Python integers"""
    n, L = rows["samples"].shape

    def key(i, a):
        ret, lost, safe = int(rows["ret_sum"][i, a]), int(rows["lost"][i, a]), int(rows["safe_frames_sum"][i, a])
        return ((-ret, lost, -safe) if objective == 0 else (lost, -safe, -ret)) + (a,)
    return np.array([min(range(L), key=lambda a: key(i, a)) for i in range(n)], np.int64)


def carry(nodes, L, simulations, keep=0, max_visits=0):
    """step 4 for one env: nodes = the final tree a*.  -> (the L carried trees, [] where absent; stats).  The ids of the subtree
    under the root's child k are collected by a walk and sorted; the first `keep` stay, in that order"""
    keep = min(keep or simulations + 1, simulations + 1)
    max_visits = max_visits or MAX_VISITS
    out, stats = [], dict(truncated=0, halved=0, absent=0, cut_mid=0)
    for k in range(L):
        top = nodes[0].child[k]
        if top is None:
            out.append([])
            stats["absent"] += 1
            continue
        ids, todo = [], [top]
        while todo:
            i = todo.pop()
            ids.append(i)
            todo.extend(c for c in nodes[i].child if c is not None)
        ids.sort()
        assert ids[0] == top and all(c is None or c > i for i in ids for c in nodes[i].child), "ids grow from parent to child"
        kept = ids[:keep]
        new = {i: j for j, i in enumerate(kept)}
        stats["truncated"] += len(ids) > keep
        halve = nodes[top].n > max_visits
        stats["halved"] += halve
        tree = []
        for i in kept:
            src = nodes[i]
            nd = Kept(L, (src.n + 1) // 2 if halve else src.n, src.v_sum // 2 if halve else src.v_sum)
            for j, c in enumerate(src.child):
                if c is not None and c in new:
                    nd.child[j] = new[c]
                elif c is not None:
                    nd.cut.add(j)
            tree.append(nd)
        assert all(nd.n >= 1 and nd.v_sum >= 0 for nd in tree) and all(tree[c].n <= nd.n for nd in tree for c in nd.child if c is not None)
        out.append(tree)
    return out, stats


class TreeActReplay:
    """the engine state of the query: the store with its key, and the drop flags"""

    def __init__(self, game, n):
        self.game, self.n, self.L = game, n, len(LEGAL[game])
        self.store, self.key, self.flags = None, None, np.zeros(n, bool)
        self.keep, self.max_visits = 0, 0

    def drop(self, mask=None):
        """TBX_EDIT_TREE_DROP; False: refused, there is no store yet"""
        if self.store is None:
            return False
        self.flags |= np.ones(self.n, bool) if mask is None else np.asarray(mask, bool)
        return True

    def call(self, lib, states, rngs, tree, reuse):
        """one successful call -> dict: out float64 [n, 14], action int32 [n], best, rows, log, stats; the store is rewritten"""
        n, L = self.n, self.L
        key = tuple(int(tree.get(k, d)) for k, d in (("frames", 0), ("hold", 1), ("depth", 1), ("objective", 0), ("simulations", 1)))
        live = bool(reuse) and self.store is not None and self.key == key
        stats = dict(used=0, start_absent=0, flag_drops=0, truncated=0, halved=0, recut=0)
        start = []
        for i in range(n):
            if live and self.flags[i]:
                stats["flag_drops"] += 1
            on = live and not self.flags[i]
            trees = []
            for a in range(L):
                if on and self.store[i][a]:
                    trees.append(copy_tree(self.store[i][a], L))
                    stats["used"] += 1
                else:
                    trees.append([Node(L)])
                    stats["start_absent"] += bool(on)
            start.append(trees)
        self.flags[:] = False
        rows, log = search(lib, self.game, states, rngs, tree, start)
        best = pick(rows, key[3])
        out = np.zeros((n, WIDTH), np.float64)
        store = []
        for i in range(n):
            a = int(best[i])
            out[i, 0], out[i, 1] = LEGAL[self.game][a], a
            for c, k in enumerate(TREE_FIELDS):
                out[i, 2 + c] = float(int(rows[k][i, a]))
            kept, st = carry(start[i][a], L, key[4], self.keep, self.max_visits)
            stats["truncated"] += st["truncated"]
            stats["halved"] += st["halved"]
            store.append(kept)
        stats["recut"] = int(sum(x["recut"].sum() for x in log))
        self.store, self.key = store, key
        return dict(out=out, action=np.array([LEGAL[self.game][a] for a in best], np.int32), best=best, rows=rows, log=log, stats=stats, trees=start)

    def units(self):
        """the store as the product's reader gives it: [env][k] lists of (n, v_sum, child) with 0 for a missing link"""
        return [[[(nd.n, nd.v_sum, tuple(c or 0 for c in nd.child)) for nd in tree] for tree in env] for env in self.store]


def played_differ(log_a, log_b):
    return sum(int(((x["code"] != y["code"]) | (x["depth"] != y["depth"])).sum()) for x, y in zip(log_a, log_b))


def expected_loop(lib, game, e, periods, tree, reuse, keep=0, max_visits=0, drops=None, compare=False, state=None, step=None):
    """The closed loop on the checker engine `e`, which is stepped: each period searches on a copy of e's records with counter
    t + period, picks, carries and steps e `hold` frames under the picked actions with auto-reset.  drops[period]: a mask (or
    None for all, "done" for the envs whose game ended in the step before) dropped before that period's call.  compare: every period
    is searched a second time from empty trees on the same records; `played` and `picked` count what reuse changed.  step(e, action)
    -> the envs whose game ended: the period's step where it is not the raw one (an agent step: its episode-end flags).
    -> (list of per-period dicts, the TreeActReplay)"""
    st = state or TreeActReplay(game, e.n_envs)
    st.keep, st.max_visits = keep, max_visits
    out, done = [], np.zeros(e.n_envs, bool)
    for p in range(periods):
        if drops and p in drops:
            st.drop(done if isinstance(drops[p], str) else drops[p])
        states, rngs = e.get_states(), sim_rngs(e)
        case = dict(tree, t=int(tree.get("t", 0)) + p)
        r = st.call(lib, states, rngs, case, reuse)
        r["units"] = st.units()
        if compare:
            plain = TreeActReplay(game, e.n_envs).call(lib, states, rngs, case, 0)
            r["played"], r["picked"] = played_differ(r["log"], plain["log"]), int((r["best"] != plain["best"]).sum())
        done = np.zeros(e.n_envs, bool)
        if step is not None:
            done |= np.asarray(step(e, r["action"])).astype(bool)
        else:
            for _ in range(int(tree.get("hold", 1))):
                done |= np.asarray(e.step(r["action"], auto_reset=True)[1]).astype(bool)
        r["done"] = done.copy()
        out.append(r)
    return out, st


# ---------------------------------------------------------------- the cases of tests/test_gpu_tree_act.py
PERIODS = 5
# the halving threshold that the `halve_mid` loop first crosses in its third period: below the root-child visits two carries can
# pile up, above what one carry brings (tests/test_tree_act.py asserts where it is crossed)
HALVE_MID = {"breakout": 41, "space_invaders": 61, "amidar": 61, "gridworld": 51}


def loop_tree(game, name):
    """keywords of expected_loop for the case `name`: depth 3, M = 6 L, frames = 3 periods of `hold`"""
    L, hold = len(LEGAL[game]), HOLD[game]
    base = dict(frames=3 * hold, hold=hold, depth=3, simulations=6 * L, explore=0, rest=-1, seed=77, t=5)
    if name == "reuse":
        return dict(tree=base, reuse=1)
    if name == "reuse_explore":
        return dict(tree=dict(base, explore=EXPLORE[game]), reuse=1)
    if name == "long":
        return dict(tree=dict(base, frames=12 * hold), reuse=1)
    if name == "survival":
        return dict(tree=dict(base, frames=12 * hold, objective=1, explore=EXPLORE[game]), reuse=1)
    if name == "few":
        return dict(tree=dict(base, simulations=L - 1), reuse=1)
    if name == "plain":
        return dict(tree=dict(base, explore=EXPLORE[game]), reuse=0)
    if name == "drawn":
        return dict(tree=dict(dict(base, **DRAWN_TREE), explore=EXPLORE[game], t=2 ** 32 - PERIODS), reuse=1)     # (the counter ends at 2^32 - 1)
    if name.startswith("keep"):
        return dict(tree=dict(base, explore=EXPLORE[game]), reuse=1, keep=int(name[4:]))
    if name == "halve1":
        return dict(tree=dict(base, explore=EXPLORE[game]), reuse=1, max_visits=1)
    if name == "halve_mid":
        return dict(tree=base, reuse=1, max_visits=HALVE_MID[game])
    raise KeyError(name)


LOOPS = ("reuse", "reuse_explore", "long", "few", "plain", "drawn", "keep1", "keep2", "keep5", "halve1", "halve_mid")
# dropped before period 2 of the `reuse` loops, through a host mask
DROP_MASK = np.arange(ENVS) % 3 == 0
# the ratchet of tests/test_tree_act.py: 1 used, 2 truncated, 3 recut, 4 halved, 5 start_absent, 6 flag_drops, 7 played, 8 picked
COVERAGE = ("used", "truncated", "recut", "halved", "start_absent", "flag_drops", "played", "picked")
# a condition a game cannot meet, and why in one line
ALLOWED_MISSING = {}


def missing_coverage(game, totals):
    return [k for k in COVERAGE if not totals.get(k) and k not in ALLOWED_MISSING.get(game, {})]
