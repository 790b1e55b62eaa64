"""The yardstick of the evolve tests (TBX_QUERY_LOOKAHEAD_EVOLVE, include/toybox_amd.h): CLONE AND PLAY GENERATION BY GENERATION,
built from search_replay.play_plan and plan_columns.

The words, generation 0, the ranking and the breeding are written here a second time, in Python integers, from the header's text
alone -- nothing of the product's evolve_word / evolve_generation0 is imported.  Individual i of first action a of every env is
played at once on ONE checker clone with per-env codes (up to TILE individuals side by side in a clone that holds the batch
several times over); the ranks are a numpy lexicographic sort per (env, first action) group.
Nothing of the device's slots, env ranges or scratch appears here.  Beside the rows, expected_evolve returns every generation's
population -- codes, fields, ranks, parents -- which the coverage conditions count (evolve_stats)."""
import numpy as np

from lookahead_replay import FIELDS, clone
from search_replay import NO_LOSS, SEARCH_FIELDS, plan_columns, play_plan, valid_plan_rows
from support import LEGAL

MAX_POPULATION, MAX_GENERATIONS = 256, 64
M64 = (1 << 64) - 1
# the cases of tests/test_gpu_evolve.py: (envs, frames, hold, depth, population, generations, elite, mutation, frames of synthetic
# play behind the batch); depth None: TBX_PLAN_MAX_DEPTH(game) with frames = hold x depth.  rest = the game's first legal action.
# deep: a fixed init plan in the even envs through per-env rows; wide: the population crosses the select kernel's 64-lane stride;
# full: the largest population, every digit mutated; deepest: Breakout codes run to 2^32 - 1.
EVOLVE_SHAPES = {"deep": (24, 96, 8, 8, 16, 3, 4, 64), "wide": (12, 64, 4, 4, 65, 1, 3, 128), "full": (4, 40, 4, 3, 256, 1, 2, 256),
                 "deepest": (24, None, 4, None, 8, 2, 2, 64)}
BATCH_FRAMES = {"breakout": 400, "space_invaders": 400, "amidar": 400, "gridworld": 40}
PLAN_SEED = 0x9E3779B9
# ... and one per game with drawn rest actions: the beam tests' seed above 32 bits, a counter that leaves 32 bits and an env offset
DRAWN_EVOLVE = dict(rest=-1, seed=(0xABCDE << 32) | 0x1234567, t=2 ** 32 - 3, env_offset=70000)


def case_evolve(game, name):
    """the keyword arguments of expected_evolve for the case `name` of `game`, and its batch: (evolve, n, batch_frames)"""
    from toybox_amd import _abi
    n, frames, hold, depth, P, G, E, mutation = EVOLVE_SHAPES[name]
    L = len(LEGAL[game])
    if depth is None:
        depth = _abi.PLAN_MAX_DEPTH[game]
        frames = hold * depth
    ev = dict(frames=frames, hold=hold, depth=depth, population=P, generations=G, elite=E, mutation=mutation, plan_seed=PLAN_SEED, rest=LEGAL[game][0])
    if name == "deep":                                        # a fixed plan -- digits 1, 2, 1, 2, ... -- in the even envs, none in the odd ones
        code = sum((1 + p % 2) * L ** p for p in range(depth))
        ev["init"] = np.where(np.arange(n) % 2 == 0, code, -1)
    return ev, n, BATCH_FRAMES[game]


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def base_word(plan_seed, a, env_number):
    return splitmix64(splitmix64(plan_seed ^ (a << 32)) ^ (env_number & M64))


def word(base, g, i, p):
    return splitmix64(base ^ (g << 40) ^ (i << 8) ^ p)


def generation0(L, depth, population, base, a, init=-1):
    """the codes of generation 0 of one (env, first action) group, Python ints"""
    codes = []
    for i in range(population):
        if i == 0 and init >= 0:
            codes.append(init - init % L + a)
        else:
            codes.append(a + sum(((word(base, 0, i, p) >> 32) % L) * L ** p for p in range(1, depth)))
    return codes


def breed(L, depth, population, elite, mutation, base, g, ranked):
    """generation g of one group from `ranked`, the codes of generation g - 1 in rank order -> (codes, parent ranks; -1: an elite)"""
    codes, parents = list(ranked[:elite]), [-1] * elite
    for i in range(elite, population):
        r = (word(base, g, i, 0) >> 32) % elite
        digits = [ranked[r] // L ** p % L for p in range(depth)]
        for p in range(1, depth):
            x = word(base, g, i, p)
            if (x & 0xff) < mutation:
                digits[p] = (x >> 32) % L
        codes.append(sum(d * L ** p for p, d in enumerate(digits)))
        parents.append(r)
    return codes, parents


def _keys(fields, objective):
    """the order's keys of individuals, larger is better, most significant first"""
    loss = np.where(fields["life_lost_at"] < 0, NO_LOSS, fields["life_lost_at"])
    return (fields["ret"], fields["lives"], loss) if objective == 0 else (fields["lives"], loss, fields["ret"])


def _order(fields, codes, objective):
    # np.lexsort sorts by its LAST key first: the index breaks the last tie, then the code; larger-is-better keys are negated
    return np.lexsort((np.arange(len(codes)), codes) + tuple(-np.asarray(k, np.float64) for k in reversed(_keys(fields, objective))))


def _col(n, v, default):
    return np.broadcast_to(np.asarray(default if v is None else v, np.int64), (n,)).copy()


TILE = 64


def _tiled(lib, game, states, rngs, s, copies):
    """one checker clone that holds the batch `copies` times over, and the plan columns for it: copy q of env i is env
    q * n + i of the clone and plays under env i's own number (env_offset + i, modulo 2^64 as the key takes it), so one clone
    plays `copies` individuals of every env at once -- the plays are the same, the Python loop is shorter"""
    n = len(states)
    big = (states._type_ * (n * copies)).from_buffer_copy(bytes(states) * copies)
    e = clone(lib, game, big, np.tile(np.asarray(rngs, np.uint64), (copies, 1)))
    tiled = {k: np.tile(v, copies) for k, v in s.items()}
    tiled["env_offset"] = np.tile(s["env_offset"] + np.arange(n, dtype=np.uint64), copies) - np.arange(n * copies, dtype=np.uint64)
    return e, tiled


def expected_evolve(lib, game, states, rngs, evolve, replay_elites=False):
    """evolve: frames, hold, depth, objective, rest, seed, t, env_offset, population, generations, elite, plan_seed, mutation, init
    (scalars, or one value per env) -> (rows, gens).  rows: the five fields and code, each [n, n_legal]; a refused env answers
    zeros.  gens[g]: dict of code, valid, rank, parent (the parent's rank in generation g - 1; -1: none), parent_code and the five
    fields, each [n, n_legal, P].  replay_elites: play the elites of a later generation again instead of carrying their records."""
    n, L = len(states), len(LEGAL[game])
    own = ("objective", "population", "generations", "elite", "plan_seed", "mutation", "init")
    s = plan_columns(n, **dict({k: v for k, v in evolve.items() if k not in own}, code=0))
    objective, P, G, E = (_col(n, evolve.get(k), d) for k, d in (("objective", 0), ("population", 1), ("generations", 0), ("elite", 1)))
    plan_seed, mutation, init = (_col(n, evolve.get(k), d) for k, d in (("plan_seed", 0), ("mutation", 64), ("init", -1)))
    depth = s["depth"]
    ok = valid_plan_rows(game, s) & (depth >= 1) & np.isin(objective, (0, 1)) & (P >= 1) & (P <= MAX_POPULATION) & (G >= 0) & (G <= MAX_GENERATIONS)
    ok &= (E >= 1) & (E <= P) & (plan_seed >= 0) & (plan_seed < 2 ** 32) & (mutation >= 0) & (mutation <= 256)
    ok &= np.array([bool(o) and (int(c) == -1 or 0 <= int(c) < L ** int(d)) for o, c, d in zip(ok, init, depth)], bool)
    rows = {k: np.zeros((n, L), np.float64 if k == "ret" else np.int64) for k in SEARCH_FIELDS}
    gens = []
    if not ok.any():
        return rows, gens
    top = int(P[ok].max())
    bases = [[base_word(int(plan_seed[i]), a, int(s["env_offset"][i]) + i) for a in range(L)] for i in range(n)]
    for g in range(int(G[ok].max()) + 1):
        on = ok & (G >= g)
        gen = {k: np.zeros((n, L, top), np.float64 if k == "ret" else np.int64) for k in FIELDS}
        gen.update(code=np.zeros((n, L, top), np.int64), valid=np.zeros((n, L, top), bool), rank=np.zeros((n, L, top), np.int64),
                   parent=np.full((n, L, top), -1, np.int64), parent_code=np.zeros((n, L, top), np.int64))
        play = np.zeros((n, L, top), bool)
        for i in np.flatnonzero(on):
            p = int(P[i])
            for a in range(L):
                if g == 0:
                    codes, parents, ranked = generation0(L, int(depth[i]), p, bases[i][a], a, int(init[i])), [-1] * p, None
                else:
                    prev = gens[g - 1]
                    by_rank = np.argsort(prev["rank"][i, a, :p])
                    ranked = [int(c) for c in prev["code"][i, a, by_rank]]
                    codes, parents = breed(L, int(depth[i]), p, int(E[i]), int(mutation[i]), bases[i][a], g, ranked)
                    for k in FIELDS:                           # the elites' records, carried (overwritten below where they are replayed)
                        gen[k][i, a, :E[i]] = prev[k][i, a, by_rank[:E[i]]]
                gen["code"][i, a, :p], gen["parent"][i, a, :p], gen["valid"][i, a, :p] = codes, parents, True
                gen["parent_code"][i, a, :p] = [ranked[r] if r >= 0 else 0 for r in parents]
                play[i, a, :p] = True
                if g > 0 and not replay_elites:
                    play[i, a, :E[i]] = False
        for a in range(L):
            slots = [j for j in range(top) if play[:, a, j].any()]
            for c in range(0, len(slots), TILE):
                part = slots[c:c + TILE]
                mine = np.concatenate([play[:, a, j] for j in part])
                e, tiled = _tiled(lib, game, states, rngs, s, len(part))
                tiled["code"] = np.where(mine, np.concatenate([gen["code"][:, a, j] for j in part]), 0)
                row = play_plan(e, game, tiled, ok=mine)
                e.close()
                for q, j in enumerate(part):
                    for k in FIELDS:
                        gen[k][play[:, a, j], a, j] = row[k][q * n:(q + 1) * n][play[:, a, j]]
        for i in np.flatnonzero(on):
            p = int(P[i])
            for a in range(L):
                order = _order({k: gen[k][i, a, :p] for k in FIELDS}, gen["code"][i, a, :p], int(objective[i]))
                gen["rank"][i, a, order] = np.arange(p)
                if g == G[i]:
                    for k in FIELDS:
                        rows[k][i, a] = gen[k][i, a, order[0]]
                    rows["code"][i, a] = gen["code"][i, a, order[0]]
        gens.append(gen)
    return rows, gens


def evolve_stats(game, gens, objective, depth):
    """what the coverage conditions count over the replay of a case (objective and depth: scalars, or one per env): new_winner --
    groups whose final winner is not generation 0's; code_ranks -- (group, generation) populations where two neighbours in rank
    order differ in nothing but the code; duplicates -- populations holding one code twice; mixed_children -- children that keep at
    least one and change at least one of their parent's digits 1 .. depth-1; ended_envs -- envs with an individual that ended the
    game; scored -- any ret > 0; plays -- plans played with the elites carried"""
    n, L, top = gens[0]["valid"].shape
    objective, depth = np.broadcast_to(objective, (n,)), np.broadcast_to(depth, (n,))
    new_winner = code_ranks = duplicates = mixed = plays = 0
    ended, scored = np.zeros(n, bool), False
    for g, gen in enumerate(gens):
        ended |= (gen["valid"] & (gen["lives"] <= 0) & (gen["frames_run"] > 0)).any(axis=(1, 2))
        scored = scored or bool((gen["ret"][gen["valid"]] > 0).any())
        plays += int((gen["valid"] & ((gen["parent"] >= 0) | (g == 0))).sum())
        for i in range(n):
            for a in range(L):
                p = int(gen["valid"][i, a].sum())
                if not p:
                    continue
                codes = gen["code"][i, a, :p]
                by_rank = np.argsort(gen["rank"][i, a, :p])
                keys = np.stack([np.asarray(k, np.float64) for k in _keys({k: gen[k][i, a, :p] for k in FIELDS}, int(objective[i]))])[:, by_rank]
                ranked = codes[by_rank]
                code_ranks += int(((keys[:, 1:] == keys[:, :-1]).all(axis=0) & (ranked[1:] != ranked[:-1])).any())
                duplicates += int(len(np.unique(codes)) < p)
                last = g + 1 == len(gens) or not gens[g + 1]["valid"][i, a].any()
                if last and g > 0:
                    first = gens[0]
                    new_winner += int(ranked[0] != first["code"][i, a, np.argmin(np.where(first["valid"][i, a], first["rank"][i, a], top))])
                for j in np.flatnonzero(gen["parent"][i, a, :p] >= 0):
                    mine = [int(codes[j]) // L ** q % L for q in range(1, int(depth[i]))]
                    theirs = [int(gen["parent_code"][i, a, j]) // L ** q % L for q in range(1, int(depth[i]))]
                    same = sum(x == y for x, y in zip(mine, theirs))
                    mixed += int(0 < same < len(mine))
    return dict(new_winner=new_winner, code_ranks=code_ranks, duplicates=duplicates, mixed_children=mixed, ended_envs=int(ended.sum()), scored=scored, plays=plays)


def not_worse(objective, x, y):
    """rows x are not worse than rows y under the order's keys (the code left out): bool, the shape of the rows"""
    kx, ky = _keys(x, objective), _keys(y, objective)
    better = np.zeros(np.shape(kx[0]), bool)
    equal = np.ones(np.shape(kx[0]), bool)
    for a, b in zip(kx, ky):
        better |= equal & (a > b)
        equal &= a == b
    return better | equal


COVERAGE = ("new_winner", "code_ranks", "duplicates", "mixed_children", "ended_envs")


def missing_coverage(game, totals):
    """the conditions that the summed counts of a game's cases do not meet"""
    return [k for k in COVERAGE if not totals.get(k)]
