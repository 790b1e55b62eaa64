"""Engine: thin Python view of one tbx_engine handle (N envs of one game on one MI355X).

All compute happens behind the C-ABI of include/toybox_amd.h; this class only marshals numpy
buffers and POD records.  The library is the in-tree HIP build (toybox_amd/_lib.py).  The `lib`
argument takes any bound library that exports the same ABI; product code never passes it (the
test-suite uses it to drive this host code over its CPU checker).
"""
import ctypes as C

import weakref

import numpy as np

from . import _abi
from ._lib import ToyboxAmdError, load


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _addr(a):
    """address of a C-contiguous numpy array for a descriptor struct (None -> 0)"""
    if a is None:
        return None
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("host output arrays must be C-contiguous")
    return a.ctypes.data


class HostArray:
    """One block of page-locked host memory from the engine library's tbx_host_alloc, handed out as a numpy array.  The block
    belongs to the ctypes array that is the `base` of every numpy view of it: a finaliser on that array calls tbx_host_free when
    the last view is gone -- by reference counting alone, no garbage-collector pass needed (the earlier owner
    object <-> buffer cycle kept blocks of several hundred MB alive until a full collection).  An observation a caller kept past
    env.close() stays valid."""

    @staticmethod
    def _release(lib, address):
        try:
            lib.tbx_host_free(C.c_void_p(address))
        except Exception:
            pass

    @staticmethod
    def make(lib, shape, dtype=np.uint8):
        dt = np.dtype(dtype)
        count = int(np.prod(shape))
        nbytes = max(1, count * dt.itemsize)
        p = C.c_void_p()
        rc = lib.tbx_host_alloc(C.byref(p), nbytes)
        if rc != _abi.OK or not p.value:
            msg = lib.tbx_last_error(None)
            raise ToyboxAmdError(rc, msg.decode() if msg else "tbx_host_alloc failed")
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        weakref.finalize(buf, HostArray._release, lib, p.value)      # (holds the library and the address, not the buffer)
        return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)


def checkpoint_args(n_envs, slot, rows=None, salt=None):
    """The argument rows of TBX_EDIT_CHECKPOINT_SAVE / _RESTORE and TBX_QUERY_CHECKPOINT_VALID: columns {slot[, row[, salt]]},
    trailing absent ones dropped, a salt without rows with -1 ("the env's own row") in the row column.  All scalars: a list, the
    same for every env; any column one per env: float64 [N, columns] (a scalar column broadcasts; a wrong length raises)."""
    cols = [slot]
    if rows is not None or salt is not None:
        cols.append(-1 if rows is None else rows)
    if salt is not None:
        cols.append(salt)
    if not any(np.ndim(c) for c in cols):
        return [float(c) for c in cols]
    args = np.empty((int(n_envs), len(cols)), np.float64)
    for k, c in enumerate(cols):
        c = np.asarray(c, np.float64)
        if c.ndim > 1 or (c.ndim == 1 and c.shape[0] != int(n_envs)):
            raise ValueError("checkpoint arguments are ints or one value per env (%d), got shape %r" % (n_envs, c.shape))
        args[:, k] = c
    return args


LOOKAHEAD_FIELDS = ("ret", "score", "lives", "frames_run", "life_lost_at")


def lookahead_args(n_envs, frames, hold=1, first=None, rest=None, seed=0, t=0, env_offset=0):
    """The argument rows of TBX_QUERY_LOOKAHEAD / _ALL: columns {frames, hold, first, rest, seed_lo, seed_hi, t, env_offset}.
    Returns (args, per_env): all scalars give one shared row (a list of 8 floats, per_env False); any column one value per env
    gives float64 [N, 8] (per_env True; scalar columns broadcast, a wrong length raises).  first / rest: an ALE action id or None
    = -1 = drawn by the synthetic rule; the seed (below 2**64) is split into its 32-bit halves.  Ranges are checked here where
    every env shares the value (ValueError); per-env rows are checked on the device, where a bad row answers zeros."""
    cols = [frames, hold, -1 if first is None else first, -1 if rest is None else rest, seed, t, env_offset]
    per_env = any(np.ndim(c) for c in cols)
    n = int(n_envs)
    for name, c in zip(("frames", "hold", "first", "rest", "seed", "t", "env_offset"), cols):
        if np.ndim(c) > 1 or (np.ndim(c) == 1 and len(c) != n):
            raise ValueError("lookahead %s is a scalar or one value per env (%d), got shape %r" % (name, n, np.shape(c)))
    if not np.ndim(frames) and not 1 <= int(frames) <= _abi.LOOKAHEAD_MAX_FRAMES:
        raise ValueError("lookahead frames must be 1 .. %d, got %r" % (_abi.LOOKAHEAD_MAX_FRAMES, frames))
    if not np.ndim(hold) and int(hold) < 1:
        raise ValueError("lookahead hold must be at least 1, got %r" % (hold,))
    for name, c, top in (("seed", seed, 1 << 64), ("t", t, 1 << 32), ("env_offset", env_offset, 1 << 32)):
        v = np.asarray(c, dtype=object).reshape(-1)
        if any(int(x) < 0 or int(x) >= top for x in v):
            raise ValueError("lookahead %s must be in 0 .. 2**%d - 1" % (name, 64 if name == "seed" else 32))
    sd = np.asarray(seed, dtype=np.uint64)
    cols = cols[:4] + [sd & np.uint64(0xFFFFFFFF), sd >> np.uint64(32)] + cols[5:]
    if not per_env:
        return [float(c) for c in cols], False
    args = np.empty((n, len(cols)), np.float64)
    for k, c in enumerate(cols):
        args[:, k] = np.asarray(c, np.float64)
    return args, True


SEARCH_OBJECTIVES = {"return": 0, "survival": 1}


def _game_name(game):
    return game if isinstance(game, str) else _abi.GAME_NAMES[int(game)]


def plan_code(game, actions):
    """ALE action ids [..., depth] -> plan codes [...] (uint64): code = sum of digit_p * n_legal ** p, digit_p the index of action p
    in the game's legal set, action 0 the first played.  An action outside the legal set or a depth beyond PLAN_MAX_DEPTH raises."""
    game = _game_name(game)
    legal = np.asarray(_abi.LEGAL_ACTIONS[game], np.int64)
    a = np.asarray(actions, np.int64)
    if a.ndim < 1 or a.shape[-1] > _abi.PLAN_MAX_DEPTH[game]:
        raise ValueError("a plan is [..., depth] action ids with depth 0 .. %d, got shape %r" % (_abi.PLAN_MAX_DEPTH[game], a.shape))
    if not np.isin(a, legal).all():
        raise ValueError("a plan holds an action outside the legal set %r of %s" % (tuple(legal), game))
    digits = np.searchsorted(legal, a).astype(np.uint64)
    code = np.zeros(a.shape[:-1], np.uint64)
    for p in range(a.shape[-1] - 1, -1, -1):
        code = code * np.uint64(len(legal)) + digits[..., p]
    return code


def plan_digits(n_legal, code, depth):
    """plan codes [...] -> their digits [..., depth] (int64): indices into the legal set, digit 0 first"""
    c = np.asarray(code).astype(np.uint64)
    out = np.empty(c.shape + (int(depth),), np.int64)
    for p in range(int(depth)):
        out[..., p] = (c % np.uint64(n_legal)).astype(np.int64)
        c = c // np.uint64(n_legal)
    return out


def plan_actions(game, code, depth):
    """plan codes [...] -> ALE action ids [..., depth] (int64), the inverse of plan_code"""
    game = _game_name(game)
    legal = np.asarray(_abi.LEGAL_ACTIONS[game], np.int64)
    if not 0 <= int(depth) <= _abi.PLAN_MAX_DEPTH[game]:
        raise ValueError("plan depth must be 0 .. %d, got %r" % (_abi.PLAN_MAX_DEPTH[game], depth))
    c = np.asarray(code)
    if c.size and (c.min() < 0 or int(c.max()) >= len(legal) ** int(depth)):
        raise ValueError("plan codes of depth %d are 0 .. %d" % (depth, len(legal) ** int(depth) - 1))
    return legal[plan_digits(len(legal), c, depth)]


def _plan_rows(what, game, n_envs, frames, hold, depth, col3, rest, seed, t, env_offset):
    """columns {frames, hold, depth, code | objective, rest, seed_lo, seed_hi, t, env_offset}: lookahead_args with `first` set
    aside, then depth and column 3 put in"""
    game = _game_name(game)
    for name, c in (("depth", depth), (what, col3)):
        if np.ndim(c) > 1 or (np.ndim(c) == 1 and len(c) != int(n_envs)):
            raise ValueError("lookahead %s is a scalar or one value per env (%d), got shape %r" % (name, n_envs, np.shape(c)))
    if rest is not None and not np.ndim(rest) and int(rest) != -1 and int(rest) not in _abi.LEGAL_ACTIONS[game]:
        raise ValueError("lookahead rest must be None, -1 or one of %r, got %r" % (_abi.LEGAL_ACTIONS[game], rest))
    base, per_env = lookahead_args(n_envs, frames, hold, None, rest, seed, t, env_offset)
    if not per_env and not np.ndim(depth) and not np.ndim(col3):
        return [base[0], base[1], float(depth), float(col3)] + base[3:], False
    args = np.empty((int(n_envs), 9), np.float64)
    args[:, [0, 1, 4, 5, 6, 7, 8]] = np.asarray(base, np.float64)[..., [0, 1, 3, 4, 5, 6, 7]]
    args[:, 2] = np.asarray(depth, np.float64)
    args[:, 3] = np.asarray(col3, np.float64)
    return args, True


def plan_args(game, n_envs, frames, hold=1, depth=0, code=0, rest=None, seed=0, t=0, env_offset=0):
    """The argument rows of TBX_QUERY_LOOKAHEAD_PLAN: columns {frames, hold, depth, code, rest, seed_lo, seed_hi, t, env_offset};
    (args, per_env) as lookahead_args gives them.  Shared values are range-checked here (ValueError): depth 0 .. PLAN_MAX_DEPTH,
    code 0 .. n_legal ** depth - 1, rest None / -1 / a legal action; per-env rows are left to the device (a bad row answers zeros)."""
    name = _game_name(game)
    if not np.ndim(depth):
        if not 0 <= int(depth) <= _abi.PLAN_MAX_DEPTH[name]:
            raise ValueError("plan depth must be 0 .. %d, got %r" % (_abi.PLAN_MAX_DEPTH[name], depth))
        if not np.ndim(code) and not 0 <= int(code) < len(_abi.LEGAL_ACTIONS[name]) ** int(depth):
            raise ValueError("plan code must be 0 .. n_legal ** depth - 1, got %r at depth %r" % (code, depth))
    return _plan_rows("code", name, n_envs, frames, hold, depth, code, rest, seed, t, env_offset)


def search_args(game, n_envs, frames, hold=1, depth=1, objective=0, rest=None, seed=0, t=0, env_offset=0):
    """The argument rows of TBX_QUERY_LOOKAHEAD_SEARCH: columns {frames, hold, depth, objective, rest, seed_lo, seed_hi, t,
    env_offset}; objective 0 / "return" or 1 / "survival".  Shared values are range-checked here (ValueError): depth >= 1 with
    n_legal ** depth <= LOOKAHEAD_MAX_PLANS; per-env rows are left to the device."""
    name = _game_name(game)
    if isinstance(objective, str):
        if objective not in SEARCH_OBJECTIVES:
            raise ValueError("search objective is 'return' or 'survival', got %r" % (objective,))
        objective = SEARCH_OBJECTIVES[objective]
    if not np.ndim(objective) and int(objective) not in (0, 1):
        raise ValueError("search objective is 0 (return) or 1 (survival), got %r" % (objective,))
    if not np.ndim(depth) and not (int(depth) >= 1 and len(_abi.LEGAL_ACTIONS[name]) ** int(depth) <= _abi.LOOKAHEAD_MAX_PLANS):
        raise ValueError("search depth must be at least 1 with n_legal ** depth <= %d, got %r" % (_abi.LOOKAHEAD_MAX_PLANS, depth))
    return _plan_rows("objective", name, n_envs, frames, hold, depth, objective, rest, seed, t, env_offset)


def beam_args(game, n_envs, frames, depth, width, hold=1, objective=0, rest=None, seed=0, t=0, env_offset=0):
    """The argument rows of TBX_QUERY_LOOKAHEAD_BEAM: columns {frames, hold, depth, objective, rest, seed_lo, seed_hi, t,
    env_offset, width} -- the search's with width appended; (args, per_env) as lookahead_args gives them.  Shared values are
    range-checked here (ValueError): depth 1 .. PLAN_MAX_DEPTH (no n_legal ** depth cap), width 1 .. BEAM_MAX_WIDTH, objective
    0 / "return" or 1 / "survival"; per-env rows are left to the device (a bad row answers zeros)."""
    name = _game_name(game)
    if isinstance(objective, str):
        if objective not in SEARCH_OBJECTIVES:
            raise ValueError("beam objective is 'return' or 'survival', got %r" % (objective,))
        objective = SEARCH_OBJECTIVES[objective]
    if not np.ndim(objective) and int(objective) not in (0, 1):
        raise ValueError("beam objective is 0 (return) or 1 (survival), got %r" % (objective,))
    if not np.ndim(depth) and not 1 <= int(depth) <= _abi.PLAN_MAX_DEPTH[name]:
        raise ValueError("beam depth must be 1 .. %d, got %r" % (_abi.PLAN_MAX_DEPTH[name], depth))
    if np.ndim(width) > 1 or (np.ndim(width) == 1 and len(width) != int(n_envs)):
        raise ValueError("lookahead width is a scalar or one value per env (%d), got shape %r" % (n_envs, np.shape(width)))
    if not np.ndim(width) and not 1 <= int(width) <= _abi.BEAM_MAX_WIDTH:
        raise ValueError("beam width must be 1 .. %d, got %r" % (_abi.BEAM_MAX_WIDTH, width))
    base, per_env = _plan_rows("objective", name, n_envs, frames, hold, depth, objective, rest, seed, t, env_offset)
    if not per_env and not np.ndim(width):
        return list(base) + [float(width)], False
    args = np.empty((int(n_envs), 10), np.float64)
    args[:, :9] = np.asarray(base, np.float64)
    args[:, 9] = np.asarray(width, np.float64)
    return args, True


def evolve_args(game, n_envs, frames, depth, population=1, generations=0, elite=1, plan_seed=0, mutation=64, init=-1, hold=1, objective=0, rest=None,
                seed=0, t=0, env_offset=0):
    """The argument rows of TBX_QUERY_LOOKAHEAD_EVOLVE: columns {frames, hold, depth, objective, rest, seed_lo, seed_hi, t,
    env_offset, population, generations, elite, plan_seed, mutation, init} -- the beam's first nine with the six of the evolution
    appended; (args, per_env) as lookahead_args gives them.  init: a plan code of `depth` (its digit 0 is replaced by every first
    action in turn) or -1 / None for none.  Shared values are range-checked here (ValueError): depth 1 .. PLAN_MAX_DEPTH (no
    n_legal ** depth cap), population 1 .. EVOLVE_MAX_POPULATION, generations 0 .. EVOLVE_MAX_GENERATIONS, elite 1 .. population,
    plan_seed 0 .. 2**32 - 1, mutation 0 .. 256, init -1 or 0 .. n_legal ** depth - 1, objective 0 / "return" or 1 / "survival";
    per-env rows are left to the device (a bad row answers zeros)."""
    name = _game_name(game)
    if isinstance(objective, str):
        if objective not in SEARCH_OBJECTIVES:
            raise ValueError("evolve objective is 'return' or 'survival', got %r" % (objective,))
        objective = SEARCH_OBJECTIVES[objective]
    if not np.ndim(objective) and int(objective) not in (0, 1):
        raise ValueError("evolve objective is 0 (return) or 1 (survival), got %r" % (objective,))
    if not np.ndim(depth) and not 1 <= int(depth) <= _abi.PLAN_MAX_DEPTH[name]:
        raise ValueError("evolve depth must be 1 .. %d, got %r" % (_abi.PLAN_MAX_DEPTH[name], depth))
    init = -1 if init is None else init
    own = (("population", population), ("generations", generations), ("elite", elite), ("plan_seed", plan_seed), ("mutation", mutation), ("init", init))
    for what, c in own:
        if np.ndim(c) > 1 or (np.ndim(c) == 1 and len(c) != int(n_envs)):
            raise ValueError("lookahead %s is a scalar or one value per env (%d), got shape %r" % (what, n_envs, np.shape(c)))
    for what, c, lo, hi in (("population", population, 1, _abi.EVOLVE_MAX_POPULATION), ("generations", generations, 0, _abi.EVOLVE_MAX_GENERATIONS),
                            ("plan_seed", plan_seed, 0, (1 << 32) - 1), ("mutation", mutation, 0, 256)):
        if not np.ndim(c) and not lo <= int(c) <= hi:
            raise ValueError("evolve %s must be %d .. %d, got %r" % (what, lo, hi, c))
    if not np.ndim(elite) and not np.ndim(population) and not 1 <= int(elite) <= int(population):
        raise ValueError("evolve elite must be 1 .. population (%r), got %r" % (population, elite))
    if not np.ndim(elite) and int(elite) < 1:
        raise ValueError("evolve elite must be at least 1, got %r" % (elite,))
    if not np.ndim(init) and int(init) != -1:
        if int(init) < 0 or (not np.ndim(depth) and int(init) >= len(_abi.LEGAL_ACTIONS[name]) ** int(depth)):
            raise ValueError("evolve init must be -1 or a plan code 0 .. n_legal ** depth - 1, got %r at depth %r" % (init, depth))
    base, per_env = _plan_rows("objective", name, n_envs, frames, hold, depth, objective, rest, seed, t, env_offset)
    if not per_env and not any(np.ndim(c) for _, c in own):
        return list(base) + [float(int(c)) for _, c in own], False
    args = np.empty((int(n_envs), 15), np.float64)
    args[:, :9] = np.asarray(base, np.float64)
    for k, (_, c) in enumerate(own):
        args[:, 9 + k] = np.asarray(c, np.float64)
    return args, True


def evolve_word(plan_seed, env, action_index, g, i, p):
    """The draw word w(g, i, p) of TBX_QUERY_LOOKAHEAD_EVOLVE for env number `env` (env_offset + the env's index, below 2**64) and
    first action index `action_index`: splitmix64(base ^ (g << 40) ^ (i << 8) ^ p) with
    base = splitmix64(splitmix64(plan_seed ^ (action_index << 32)) ^ env).  With it a caller reproduces every population."""
    base = _splitmix64(_splitmix64(int(plan_seed) ^ (int(action_index) << 32)) ^ (int(env) & 0xFFFFFFFFFFFFFFFF))
    return _splitmix64(base ^ (int(g) << 40) ^ (int(i) << 8) ^ int(p))


def evolve_generation0(game, depth, population, plan_seed, env, action_index, init=None):
    """The plan codes of generation 0 of TBX_QUERY_LOOKAHEAD_EVOLVE for env number `env` (env_offset + index) and first action index
    `action_index`: uint64 [population]; individual 0 takes digits 1 .. depth-1 of `init` where one is given."""
    L = len(_abi.LEGAL_ACTIONS[_game_name(game)])
    codes = np.empty(int(population), np.uint64)
    for i in range(int(population)):
        if i == 0 and init is not None and int(init) >= 0:
            codes[i] = int(init) - int(init) % L + int(action_index)
        else:
            codes[i] = int(action_index) + sum(((evolve_word(plan_seed, env, action_index, 0, i, p) >> 32) % L) * L ** p for p in range(1, int(depth)))
    return codes


ACT_PLANNERS = {"search": _abi.QUERY_LOOKAHEAD_SEARCH, "search_samples": _abi.QUERY_LOOKAHEAD_SEARCH_SAMPLES, "beam": _abi.QUERY_LOOKAHEAD_BEAM,
                "beam_samples": _abi.QUERY_LOOKAHEAD_BEAM_SAMPLES, "evolve": _abi.QUERY_LOOKAHEAD_EVOLVE}
ACT_SAMPLED = (_abi.QUERY_LOOKAHEAD_SEARCH_SAMPLES, _abi.QUERY_LOOKAHEAD_BEAM_SAMPLES)


def act_planner(planner):
    """the query id of a planner of TBX_QUERY_LOOKAHEAD_ACT: one of ACT_PLANNERS' names or ids"""
    pid = ACT_PLANNERS.get(planner) if isinstance(planner, str) else int(planner)
    if pid not in ACT_PLANNERS.values():
        raise ValueError("act planner is one of %r or their query ids, got %r" % (tuple(ACT_PLANNERS), planner))
    return pid


def act_args(game, planner, **planner_keywords):
    """The shared argument row of TBX_QUERY_LOOKAHEAD_ACT: {planner, then the planner's own columns} as search_args /
    search_samples_args / beam_args / beam_samples_args / evolve_args build them from `planner_keywords` (their n_envs is not
    asked for: the query takes shared arguments only, and a per-env value raises ValueError), range-checked there.  planner: a
    name of ACT_PLANNERS or its query id.  With the evolution init="carry" (or -2) becomes -2: every env is seeded with the
    plan the last call left in BUF_PLAN_CARRY."""
    pid = act_planner(planner)
    build = {_abi.QUERY_LOOKAHEAD_SEARCH: search_args, _abi.QUERY_LOOKAHEAD_SEARCH_SAMPLES: search_samples_args, _abi.QUERY_LOOKAHEAD_BEAM: beam_args,
             _abi.QUERY_LOOKAHEAD_BEAM_SAMPLES: beam_samples_args, _abi.QUERY_LOOKAHEAD_EVOLVE: evolve_args}[pid]
    kw = dict(planner_keywords)
    carry = False
    if pid == _abi.QUERY_LOOKAHEAD_EVOLVE and "init" in kw and not np.ndim(kw["init"]) and kw["init"] is not None:
        if isinstance(kw["init"], str) and kw["init"] != "carry":
            raise ValueError("evolve init is a plan code, -1 / None or 'carry', got %r" % (kw["init"],))
        if isinstance(kw["init"], str) or int(kw["init"]) == -2:
            carry, kw["init"] = True, -1
    if "n_envs" in kw:
        raise ValueError("act takes shared arguments only: no n_envs")
    args, per_env = build(game, 1, **kw)
    if per_env:
        raise ValueError("act takes shared arguments only, got a per-env value")
    args = [float(pid)] + [float(v) for v in args]
    if carry:
        args[15] = -2.0
    return args


def plan_pick(rows, objective=0, sampled=False):
    """The pick of TBX_QUERY_LOOKAHEAD_ACT in numpy: rows [N, n_legal, 6] of a search, a beam or an evolution ({ret, score, lives,
    frames run, life lost at, code}) or, sampled, [N, n_legal, 9] of their sampled forms (the eight sums, then the code) -> the
    winner's action index, int64 [N].  Not sampled: the search's order for `objective` (0 / "return": the larger ret, lives,
    loss; 1 / "survival": lives, loss, ret; loss = life lost at, none counting as later than any), then the smaller code.
    Sampled: the larger ret_sum, the smaller lost, the larger safe_frames_sum ("survival": lost, safe_frames_sum, ret_sum), then
    the smaller index."""
    objective = SEARCH_OBJECTIVES.get(objective, objective) if isinstance(objective, str) else int(objective)
    if objective not in (0, 1):
        raise ValueError("objective is 0 / 'return' or 1 / 'survival', got %r" % (objective,))
    r = np.asarray(rows)
    if r.ndim != 3 or r.shape[2] != (9 if sampled else 6):
        raise ValueError("rows are [N, n_legal, %d], got shape %r" % (9 if sampled else 6, r.shape))
    r = r.astype(np.int64)
    if sampled:
        ret, k1, k2 = -r[..., 1], r[..., 5], -r[..., 7]
        tie = np.broadcast_to(np.arange(r.shape[1]), r.shape[:2])
    else:
        ret, k1 = -r[..., 0], -r[..., 2]
        k2 = -np.where(r[..., 4] < 0, 1 << 30, r[..., 4])
        tie = r[..., 5]
    keys = (ret, k1, k2) if objective == 0 else (k1, k2, ret)
    # np.lexsort: the last key is the primary one, ascending
    return np.lexsort((tie,) + tuple(reversed(keys)), axis=1)[:, 0].astype(np.int64)


def plan_shift(game, code, depth):
    """A plan code shifted by one period, as TBX_QUERY_LOOKAHEAD_ACT leaves it in BUF_PLAN_CARRY: code // L + (code % L) *
    L ** (depth - 1) -- np.roll(digits, -1); an int or a uint64 array"""
    L = len(_abi.LEGAL_ACTIONS[_game_name(game)])
    if not 1 <= int(depth) <= _abi.PLAN_MAX_DEPTH[_game_name(game)]:
        raise ValueError("plan depth must be 1 .. %d, got %r" % (_abi.PLAN_MAX_DEPTH[_game_name(game)], depth))
    if not np.ndim(code):
        return int(code) // L + (int(code) % L) * L ** (int(depth) - 1)
    c = np.asarray(code).astype(np.uint64)
    return c // np.uint64(L) + (c % np.uint64(L)) * np.uint64(L ** (int(depth) - 1))


SAMPLE_FIELDS = ("samples", "ret_sum", "ret_min", "ret_max", "lives_sum", "lost", "ended", "safe_frames_sum")


def _splitmix64(x):
    x = (int(x) + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def sample_seed(seed, s):
    """The lookahead seed of future s of TBX_QUERY_LOOKAHEAD_SAMPLES: splitmix64((seed + s) mod 2**64).  Future s of a sampled
    lookahead with salt 0 is lookahead_all(..., seed=sample_seed(seed, s))."""
    return _splitmix64((int(seed) + int(s)) & 0xFFFFFFFFFFFFFFFF)


def sample_args(game, n_envs, frames, samples, hold=1, salt=0, rest=None, seed=0, t=0, env_offset=0):
    """The argument rows of TBX_QUERY_LOOKAHEAD_SAMPLES: columns {frames, hold, samples, salt, rest, seed_lo, seed_hi, t,
    env_offset}; (args, per_env) as lookahead_args gives them.  Shared values are range-checked here (ValueError): samples
    1 .. LOOKAHEAD_MAX_SAMPLES, salt 0 .. 2**32 - 1 with salt + samples - 1 below 2**32 where it is not 0; per-env rows are left
    to the device (a bad row answers zeros)."""
    if not np.ndim(samples) and not 1 <= int(samples) <= _abi.LOOKAHEAD_MAX_SAMPLES:
        raise ValueError("samples must be 1 .. %d, got %r" % (_abi.LOOKAHEAD_MAX_SAMPLES, samples))
    if not np.ndim(salt):
        if not 0 <= int(salt) < 1 << 32:
            raise ValueError("sample salt must be 0 .. 2**32 - 1, got %r" % (salt,))
        if int(salt) and not np.ndim(samples) and int(salt) + int(samples) - 1 >= 1 << 32:
            raise ValueError("sample salt + samples - 1 must stay below 2**32, got %r + %r" % (salt, samples))
    return _plan_rows("salt", game, n_envs, frames, hold, samples, salt, rest, seed, t, env_offset)


def search_samples_args(game, n_envs, frames, depth, samples, hold=1, objective=0, salt=0, rest=None, seed=0, t=0, env_offset=0):
    """The argument rows of TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES: columns {frames, hold, depth, objective, rest, seed_lo, seed_hi, t,
    env_offset, samples, salt} -- search_args with samples and salt appended; (args, per_env) as lookahead_args gives them.
    Shared values are range-checked here (ValueError): the search's, samples 1 .. LOOKAHEAD_MAX_SAMPLES,
    n_legal ** depth * samples <= LOOKAHEAD_MAX_LEAVES and the salt ranges of sample_args; per-env rows are left to the device
    (a bad row answers zeros)."""
    name = _game_name(game)
    for what, c in (("samples", samples), ("salt", salt)):
        if np.ndim(c) > 1 or (np.ndim(c) == 1 and len(c) != int(n_envs)):
            raise ValueError("lookahead %s is a scalar or one value per env (%d), got shape %r" % (what, n_envs, np.shape(c)))
    if not np.ndim(samples):
        if not 1 <= int(samples) <= _abi.LOOKAHEAD_MAX_SAMPLES:
            raise ValueError("samples must be 1 .. %d, got %r" % (_abi.LOOKAHEAD_MAX_SAMPLES, samples))
        if not np.ndim(depth) and int(depth) >= 1 and len(_abi.LEGAL_ACTIONS[name]) ** int(depth) * int(samples) > _abi.LOOKAHEAD_MAX_LEAVES:
            raise ValueError("n_legal ** depth * samples must not exceed %d, got depth %r and %r samples" % (_abi.LOOKAHEAD_MAX_LEAVES, depth, samples))
    if not np.ndim(salt):
        if not 0 <= int(salt) < 1 << 32:
            raise ValueError("sample salt must be 0 .. 2**32 - 1, got %r" % (salt,))
        if int(salt) and not np.ndim(samples) and int(salt) + int(samples) - 1 >= 1 << 32:
            raise ValueError("sample salt + samples - 1 must stay below 2**32, got %r + %r" % (salt, samples))
    base, per_env = search_args(name, n_envs, frames, hold, depth, objective, rest, seed, t, env_offset)
    if not per_env and not np.ndim(samples) and not np.ndim(salt):
        return list(base) + [float(samples), float(salt)], False
    args = np.empty((int(n_envs), 11), np.float64)
    args[:, :9] = np.asarray(base, np.float64)
    args[:, 9] = np.asarray(samples, np.float64)
    args[:, 10] = np.asarray(salt, np.float64)
    return args, True


def beam_kept(legal, width, level):
    """|B_level| of a beam: 1, then min(width, legal * the level before) (tbx_beam_kept)"""
    kept = 1
    for _ in range(2, int(level) + 1):
        kept = min(int(width), kept * int(legal))
    return kept


def beam_samples_args(game, n_envs, frames, depth, width, samples, hold=1, objective=0, salt=0, rest=None, seed=0, t=0, env_offset=0):
    """The argument rows of TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES: columns {frames, hold, depth, objective, rest, seed_lo, seed_hi, t,
    env_offset, width, samples, salt} -- beam_args with samples and salt appended; (args, per_env) as lookahead_args gives them.
    Shared values are range-checked here (ValueError): the beam's, samples 1 .. LOOKAHEAD_MAX_SAMPLES, the salt ranges of sample_args
    and the leaf cap -- the candidates of the widest level times the samples, n_legal * beam_kept(n_legal, width, depth - 1) *
    (1 if depth == 1 else n_legal) * samples, must not exceed LOOKAHEAD_MAX_LEAVES; per-env rows are left to the device (a bad
    row answers zeros)."""
    name = _game_name(game)
    for what, c in (("samples", samples), ("salt", salt)):
        if np.ndim(c) > 1 or (np.ndim(c) == 1 and len(c) != int(n_envs)):
            raise ValueError("lookahead %s is a scalar or one value per env (%d), got shape %r" % (what, n_envs, np.shape(c)))
    if not np.ndim(samples) and not 1 <= int(samples) <= _abi.LOOKAHEAD_MAX_SAMPLES:
        raise ValueError("samples must be 1 .. %d, got %r" % (_abi.LOOKAHEAD_MAX_SAMPLES, samples))
    if not np.ndim(salt):
        if not 0 <= int(salt) < 1 << 32:
            raise ValueError("sample salt must be 0 .. 2**32 - 1, got %r" % (salt,))
        if int(salt) and not np.ndim(samples) and int(salt) + int(samples) - 1 >= 1 << 32:
            raise ValueError("sample salt + samples - 1 must stay below 2**32, got %r + %r" % (salt, samples))
    base, per_env = beam_args(name, n_envs, frames, depth, width, hold, objective, rest, seed, t, env_offset)
    if not np.ndim(samples) and not np.ndim(depth) and not np.ndim(width):
        L = len(_abi.LEGAL_ACTIONS[name])
        leaves = L * beam_kept(L, width, int(depth) - 1) * (1 if int(depth) == 1 else L) * int(samples)
        if leaves > _abi.LOOKAHEAD_MAX_LEAVES:
            raise ValueError("the candidates of the last level x samples must not exceed %d, got %d (depth %r, width %r, %r samples)"
                             % (_abi.LOOKAHEAD_MAX_LEAVES, leaves, depth, width, samples))
    if not per_env and not np.ndim(samples) and not np.ndim(salt):
        return list(base) + [float(samples), float(salt)], False
    args = np.empty((int(n_envs), 12), np.float64)
    args[:, :10] = np.asarray(base, np.float64)
    args[:, 10] = np.asarray(samples, np.float64)
    args[:, 11] = np.asarray(salt, np.float64)
    return args, True


TREE_FIELDS = SAMPLE_FIELDS + ("code", "pv_depth", "pv_visits", "pv_value")


def tree_args(game, n_envs, frames, depth, simulations=1, explore=0, salt=0, hold=1, objective=0, rest=None, seed=0, t=0, env_offset=0):
    """The argument rows of TBX_QUERY_LOOKAHEAD_TREE: columns {frames, hold, depth, objective, rest, seed_lo, seed_hi, t,
    env_offset, simulations, explore, salt} -- the beam's first nine with the three of the tree appended; (args, per_env) as
    lookahead_args gives them.  Shared values are range-checked here (ValueError): depth 1 .. PLAN_MAX_DEPTH (no n_legal ** depth
    cap), simulations 1 .. TREE_MAX_SIMULATIONS, explore 0 .. TREE_MAX_EXPLORE (an integer in units of the value), the salt ranges
    of sample_args with simulations for samples, objective 0 / "return" or 1 / "survival"; per-env rows are left to the device (a
    bad row answers zeros)."""
    name = _game_name(game)
    if isinstance(objective, str):
        if objective not in SEARCH_OBJECTIVES:
            raise ValueError("tree objective is 'return' or 'survival', got %r" % (objective,))
        objective = SEARCH_OBJECTIVES[objective]
    if not np.ndim(objective) and int(objective) not in (0, 1):
        raise ValueError("tree objective is 0 (return) or 1 (survival), got %r" % (objective,))
    if not np.ndim(depth) and not 1 <= int(depth) <= _abi.PLAN_MAX_DEPTH[name]:
        raise ValueError("tree depth must be 1 .. %d, got %r" % (_abi.PLAN_MAX_DEPTH[name], depth))
    own = (("simulations", simulations), ("explore", explore), ("salt", salt))
    for what, c in own:
        if np.ndim(c) > 1 or (np.ndim(c) == 1 and len(c) != int(n_envs)):
            raise ValueError("lookahead %s is a scalar or one value per env (%d), got shape %r" % (what, n_envs, np.shape(c)))
    for what, c, lo, hi in (("simulations", simulations, 1, _abi.TREE_MAX_SIMULATIONS), ("explore", explore, 0, _abi.TREE_MAX_EXPLORE), ("salt", salt, 0, (1 << 32) - 1)):
        if not np.ndim(c) and not lo <= int(c) <= hi:
            raise ValueError("tree %s must be %d .. %d, got %r" % (what, lo, hi, c))
    if not np.ndim(salt) and int(salt) and not np.ndim(simulations) and int(salt) + int(simulations) - 1 >= 1 << 32:
        raise ValueError("tree salt + simulations - 1 must stay below 2**32, got %r + %r" % (salt, simulations))
    base, per_env = _plan_rows("objective", name, n_envs, frames, hold, depth, objective, rest, seed, t, env_offset)
    if not per_env and not any(np.ndim(c) for _, c in own):
        return list(base) + [float(int(c)) for _, c in own], False
    args = np.empty((int(n_envs), 12), np.float64)
    args[:, :9] = np.asarray(base, np.float64)
    for k, (_, c) in enumerate(own):
        args[:, 9 + k] = np.asarray(c, np.float64)
    return args, True


TREE_ACT_WIDTH = 14


def tree_act_args(game, frames, depth, simulations=1, explore=0, salt=0, reuse=False, hold=1, objective=0, rest=None, seed=0, t=0, env_offset=0):
    """The shared argument row of TBX_QUERY_LOOKAHEAD_TREE_ACT: tree_args' twelve columns, range-checked there, then reuse (False / 0
    or True / 1: start from the carried trees where they are live).  The query takes shared arguments only, so there is no
    n_envs and a per-env value raises ValueError."""
    if isinstance(reuse, (bool, np.bool_)):
        reuse = int(reuse)
    if np.ndim(reuse) or reuse not in (0, 1):
        raise ValueError("tree act reuse is False / 0 or True / 1, got %r" % (reuse,))
    args, per_env = tree_args(game, 1, frames, depth, simulations, explore, salt, hold, objective, rest, seed, t, env_offset)
    if per_env:
        raise ValueError("tree act takes shared arguments only, got a per-env value")
    return [float(v) for v in args] + [float(int(reuse))]


def tree_carry(game, nodes, a_star, simulations, keep=None, max_visits=None):
    """The carry of TBX_QUERY_LOOKAHEAD_TREE_ACT in plain Python.  nodes: the L = n_legal(game) final trees of one env, each a list
    of (n, v_sum, child) in creation order with child a sequence of L links (0 or None: no child); a_star: the picked action
    index.  Returns the L carried trees in the same form with 0 for a missing link, an empty list where the root of tree a_star has
    no child k: the subtree under child k, its nodes in ascending source id, the first `keep` (None / 0: simulations + 1; more
    than that counts as that) kept and renumbered in that order, links to nodes that were not kept cut, and -- where the new
    root's n exceeds max_visits (None / 0: TREE_CARRY_MAX_VISITS) -- n = (n + 1) // 2 and v_sum = v_sum // 2 in every kept node."""
    L = len(_abi.LEGAL_ACTIONS[_game_name(game)])
    if not 1 <= int(simulations) <= _abi.TREE_MAX_SIMULATIONS:
        raise ValueError("tree simulations must be 1 .. %d, got %r" % (_abi.TREE_MAX_SIMULATIONS, simulations))
    most = int(simulations) + 1
    keep = most if not keep else int(keep)
    if not 1 <= keep <= _abi.TREE_MAX_SIMULATIONS + 1:
        raise ValueError("tree carry keep must be 1 .. %d, got %r" % (_abi.TREE_MAX_SIMULATIONS + 1, keep))
    keep = min(keep, most)
    max_visits = _abi.TREE_CARRY_MAX_VISITS if not max_visits else int(max_visits)
    if not 1 <= max_visits <= _abi.TREE_CARRY_MAX_VISITS:
        raise ValueError("tree carry max_visits must be 1 .. %d, got %r" % (_abi.TREE_CARRY_MAX_VISITS, max_visits))
    if len(nodes) != L or not 0 <= int(a_star) < L:
        raise ValueError("tree carry takes %d trees and a_star 0 .. %d" % (L, L - 1))
    src = nodes[int(a_star)]
    owner = {}                                        # source id -> (tree k, the parent's new id or None, digit)
    out = [[] for _ in range(L)]
    halved = [False] * L
    for k in range(L):
        if src[0][2][k]:
            owner[int(src[0][2][k])] = (k, None, k)
    for i in range(1, len(src)):
        if i not in owner:
            continue
        k, parent, digit = owner[i]
        if len(out[k]) >= keep:
            continue
        n, v_sum, child = src[i]
        new = len(out[k])
        if parent is None:
            halved[k] = int(n) > max_visits
        else:
            out[k][parent][2][digit] = new
        out[k].append([(int(n) + 1) // 2 if halved[k] else int(n), int(v_sum) // 2 if halved[k] else int(v_sum), [0] * L])
        for j in range(L):
            if child[j]:
                owner[int(child[j])] = (k, new, j)
    return [[(n, v, tuple(c)) for n, v, c in tree] for tree in out]


def tree_store_units(game, raw, n_envs, simulations):
    """The bytes of BUF_PLAN_TREE (a uint8 array) as carried trees: units[env][k] a list of (n, v_sum, child) with child a tuple of
    n_legal links, empty where tree (env, k) is absent -- tree_carry's form.  Layout: include/toybox_amd.h."""
    L = len(_abi.LEGAL_ACTIONS[_game_name(game)])
    stride = (int(simulations) + 2) & ~1
    block = 64 + 32 * stride
    raw = np.ascontiguousarray(raw, np.uint8).reshape(int(n_envs), L, block)
    node = np.dtype([("v_sum", "<i8"), ("n", "<u4"), ("child", "<u2", (6,)), ("nodes", "<u4"), ("pad", "<u4")])
    units = []
    for e in range(int(n_envs)):
        row = []
        for k in range(L):
            count = int(raw[e, k, :4].view("<u4")[0])
            recs = raw[e, k, 64:64 + 32 * count].view(node)
            row.append([(int(r["n"]), int(r["v_sum"]), tuple(int(c) for c in r["child"][:L])) for r in recs])
        units.append(row)
    return units


class Engine:
    def __init__(self, game, n_envs=1, device=0, config=None, lib=None):
        self._lib = lib if lib is not None else load()
        self.game_id = _abi.GAME_IDS[game] if isinstance(game, str) else int(game)
        self.game = _abi.GAME_NAMES[self.game_id]
        self.n_envs = int(n_envs)
        self.device = int(device)
        self._h = C.c_void_p()
        self.state_type = _abi.STATE_TYPES[self.game_id]
        self.config_type = _abi.CONFIG_TYPES[self.game_id]
        cfg_ptr, cfg_size = None, 0
        if config is not None:
            if not isinstance(config, self.config_type):
                raise TypeError("config must be a %s" % self.config_type.__name__)
            cfg_ptr, cfg_size = C.cast(C.pointer(config), C.c_void_p), C.sizeof(config)
        rc = self._lib.tbx_create(self.game_id, self.n_envs, self.device, cfg_ptr, cfg_size, C.byref(self._h))
        if rc != _abi.OK:
            msg = self._lib.tbx_last_error(None)
            self._h = C.c_void_p()
            raise ToyboxAmdError(rc, msg.decode() if msg else "tbx_create failed")
        h, w = C.c_int(), C.c_int()
        self._check(self._lib.tbx_frame_dims(self.game_id, C.byref(h), C.byref(w)))
        self.height, self.width = h.value, w.value
        buf = (C.c_int32 * 18)()
        n = self._lib.tbx_legal_actions(self.game_id, buf, 18)
        self.legal_actions = [int(buf[i]) for i in range(n)]
        self._out4 = (C.c_int32 * 4)()

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != _abi.OK:
            msg = self._lib.tbx_last_error(self._h)
            raise ToyboxAmdError(rc, msg.decode() if msg else "")

    def close(self):
        if self._h:
            self._lib.tbx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------------ launch-time options (tbx_set_option)
    def set_option(self, option, value):
        self._check(self._lib.tbx_set_option(self._h, int(option), int(value)))
        return self

    def get_option(self, option):
        v = C.c_int()
        self._check(self._lib.tbx_get_option(self._h, int(option), C.byref(v)))
        return v.value

    # ------------------------------------------------------------------ seeding / RNG
    def seed(self, seed, env=-1):
        self._check(self._lib.tbx_seed(self._h, int(env), int(seed) & 0xFFFFFFFF))

    def seed_array(self, seeds):
        """env i gets seeds[i] (one upload, one launch)."""
        a = np.ascontiguousarray(seeds, dtype=np.uint32)
        if a.shape != (self.n_envs,):
            raise ValueError("seeds must have shape (%d,)" % self.n_envs)
        self._check(self._lib.tbx_seed_array(self._h, _ptr(a)))

    def get_sim_rng(self, env=0):
        out = (C.c_uint64 * 2)()
        self._check(self._lib.tbx_get_sim_rng(self._h, int(env), out))
        return int(out[0]), int(out[1])

    def set_sim_rng(self, state, env=-1):
        st = (C.c_uint64 * 2)(int(state[0]), int(state[1]))
        self._check(self._lib.tbx_set_sim_rng(self._h, int(env), st))

    # ------------------------------------------------------------------ game control
    def new_game(self, mask=None):
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            assert m.shape == (self.n_envs,)
        self._check(self._lib.tbx_new_game(self._h, _ptr(m)))

    def step(self, actions, auto_reset=False):
        """One frame for every env.  Returns (reward int32[N], done bool[N], lives int32[N], score int32[N])."""
        a = np.ascontiguousarray(actions, dtype=np.int32)
        if a.shape != (self.n_envs,):
            raise ValueError("actions must have shape (%d,)" % self.n_envs)
        n = self.n_envs
        reward, lives, score = (np.empty(n, np.int32) for _ in range(3))
        done = np.empty(n, np.uint8)
        flags = _abi.STEP_AUTO_RESET if auto_reset else 0
        self._check(self._lib.tbx_step(self._h, _ptr(a), flags, _ptr(reward), _ptr(done), _ptr(lives), _ptr(score)))
        return reward, done.astype(bool), lives, score

    def step1(self, env, ale_action, auto_reset=False):
        """One frame for one env: (reward, done, lives, score) as Python ints.  On a one-env engine this is the resident-kernel
        path of tbx_step1 (no launch, no copy)."""
        out = self._out4
        rc = self._lib.tbx_step1(self._h, env, ale_action, _abi.STEP_AUTO_RESET if auto_reset else 0, out)
        if rc != _abi.OK:
            self._check(rc)
        return out[0], out[1] != 0, out[2], out[3]

    def step1_frame(self, env, ale_action, channels=1, auto_reset=False):
        """tbx_step1_frame: one frame of one env and the picture of the state it leaves -- (reward, done, lives, score, frame)
        with frame a fresh uint8 (H, W, channels) array.  On a one-env engine the resident kernel paints into pinned host memory
        (no launch, no copy on the device side); the array returned here is a host copy of that buffer, because the buffer is
        reused by the next call and gym code keeps observations."""
        out = self._out4
        fp = C.c_void_p()
        rc = self._lib.tbx_step1_frame(self._h, env, ale_action, _abi.STEP_AUTO_RESET if auto_reset else 0, int(channels), out, C.byref(fp))
        if rc != _abi.OK:
            self._check(rc)
        if not fp.value:
            raise ToyboxAmdError(rc, "tbx_step1_frame returned no frame buffer")
        n = self.height * self.width * int(channels)
        frame = np.frombuffer((C.c_uint8 * n).from_address(fp.value), np.uint8).reshape(self.height, self.width, int(channels)).copy()
        return out[0], out[1] != 0, out[2], out[3], frame

    def apply_input(self, env, buttons):
        self._check(self._lib.tbx_apply_input(self._h, int(env), int(buttons)))

    def scalars(self):
        n = self.n_envs
        score, lives, level = (np.empty(n, np.int32) for _ in range(3))
        over = np.empty(n, np.uint8)
        self._check(self._lib.tbx_get_scalars(self._h, _ptr(score), _ptr(lives), _ptr(level), _ptr(over)))
        return score, lives, level, over.astype(bool)

    # ------------------------------------------------------------------ frames
    def render(self, channels=3, out=None):
        """Every env's frame as uint8 [N, H, W, channels] on the host.  `out`: write into this array instead of a fresh one
        (a reused, page-locked one -- toybox_amd.hip.PinnedArray -- receives the frames at the PCIe link's rate)."""
        shape = (self.n_envs, self.height, self.width, channels)
        if out is None:
            out = np.empty(shape, np.uint8)
        elif out.shape != shape or out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous uint8 array of shape %r" % (shape,))
        self._check(self._lib.tbx_render(self._h, _ptr(out), int(channels)))
        return out

    def render_env(self, env, channels=3):
        out = np.empty((self.height, self.width, channels), np.uint8)
        self._check(self._lib.tbx_render_env(self._h, int(env), _ptr(out), int(channels)))
        return out

    # ------------------------------------------------------------------ state / config records
    def get_state(self, env=0):
        st = self.state_type()
        self._check(self._lib.tbx_get_state(self._h, int(env), C.byref(st), C.sizeof(st)))
        return st

    def set_state(self, env, st):
        if not isinstance(st, self.state_type):
            raise TypeError("state must be a %s" % self.state_type.__name__)
        self._check(self._lib.tbx_set_state(self._h, int(env), C.byref(st), C.sizeof(st)))

    def get_states(self, first=0, count=None):
        """Records of envs [first, first+count) as a ctypes array (one pack launch, one copy)."""
        count = self.n_envs - first if count is None else int(count)
        arr = (self.state_type * count)()
        self._check(self._lib.tbx_get_states(self._h, int(first), count, C.cast(arr, C.c_void_p), C.sizeof(self.state_type)))
        return arr

    def set_states(self, first, arr):
        count = len(arr)
        if not isinstance(arr, C.Array) or arr._type_ is not self.state_type:
            raise TypeError("states must be a ctypes array of %s" % self.state_type.__name__)
        self._check(self._lib.tbx_set_states(self._h, int(first), count, C.cast(arr, C.c_void_p), C.sizeof(self.state_type)))

    def get_states_np(self, first=0, count=None):
        """The same records as a numpy structured array (fields named like the C struct): vectorised interventions,
        e.g. `st = e.get_states_np(); st['lives'] = 1; e.set_states_np(0, st)`."""
        arr = self.get_states(first, count)
        return np.frombuffer(arr, dtype=np.dtype(self.state_type)).copy()

    def set_states_np(self, first, records):
        rec = np.ascontiguousarray(records, dtype=np.dtype(self.state_type))
        arr = (self.state_type * len(rec)).from_buffer_copy(rec.tobytes())
        self.set_states(first, arr)

    def get_config(self):
        cfg = self.config_type()
        self._check(self._lib.tbx_get_config(self._h, C.byref(cfg), C.sizeof(cfg)))
        return cfg

    def set_config(self, cfg):
        if not isinstance(cfg, self.config_type):
            raise TypeError("config must be a %s" % self.config_type.__name__)
        self._check(self._lib.tbx_set_config(self._h, C.byref(cfg), C.sizeof(cfg)))

    # ------------------------------------------------------------------ batched interventions on the device
    def _edit_args(self, args):
        """args: a sequence of scalars (the same for every env) or an array [N, n_args] (one row per env)"""
        a = np.ascontiguousarray(args, dtype=np.float64)
        if a.ndim == 2:
            if a.shape[0] != self.n_envs:
                raise ValueError("per-env arguments need one row per env (%d), got %d" % (self.n_envs, a.shape[0]))
            return a, a.shape[1], 1
        a = a.reshape(-1)
        return a, a.shape[0], 0

    def edit(self, op, args=(), mask=None):
        """tbx_edit: one field write in every env whose mask entry is true (mask None: all) -- a kernel over the state in HBM,
        no state record crosses PCIe.  args as in _edit_args."""
        a, n, per_env = self._edit_args(args)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask).astype(bool), dtype=np.uint8)
            if m.shape != (self.n_envs,):
                raise ValueError("mask must have one entry per env")
        self._check(self._lib.tbx_edit(self._h, int(op), _ptr(a) if n else None, n, per_env, _ptr(m) if m is not None else None))

    def fork(self, src, mask=None, salt=None):
        """TBX_EDIT_COPY_ENV: every env whose mask entry is true (None: all) becomes a copy of env src (an int: one source fanned
        out; int[N]: env i copies env src[i]) as it was before the call -- game state, simulator RNG, prev_score and, after
        agent_init, the wrapper stack's state and the observation.  salt (None, an int below 2**32 or int[N]): the copy's RNG
        words become splitmix64(word ^ salt), 0 meaning none."""
        cols = [src] if salt is None else [src, salt]
        if any(np.ndim(c) for c in cols):
            args = np.empty((self.n_envs, len(cols)), np.float64)
            for k, c in enumerate(cols):
                args[:, k] = np.asarray(c, np.float64)      # (a scalar column broadcasts; a wrong length raises)
        else:
            args = [float(c) for c in cols]
        self.edit(_abi.EDIT_COPY_ENV, args, mask)

    def checkpoint_slots(self, slots):
        """TBX_EDIT_CHECKPOINT_SLOTS: a fresh, empty checkpoint store of `slots` planes of N cells on the device (an existing one
        is released first; 0 releases it).  The store belongs to the per-env arrays the engine has now: call this after agent_init."""
        self.edit(_abi.EDIT_CHECKPOINT_SLOTS, [int(slots)])

    def checkpoint_save(self, slot, mask=None):
        """TBX_EDIT_CHECKPOINT_SAVE: every env whose mask entry is true (None: all) is written into cell (slot, its own row) --
        everything fork() copies; slot an int or int[N].  Nothing in the live engine changes."""
        self.edit(_abi.EDIT_CHECKPOINT_SAVE, checkpoint_args(self.n_envs, slot), mask)

    def checkpoint_restore(self, slot, rows=None, mask=None, salt=None):
        """TBX_EDIT_CHECKPOINT_RESTORE: every selected env i becomes the env saved in cell (slot, rows[i]) (rows None: its own row);
        slot, rows, salt each an int or one per env; salt as in fork()."""
        self.edit(_abi.EDIT_CHECKPOINT_RESTORE, checkpoint_args(self.n_envs, slot, rows, salt), mask)

    def checkpoint_valid(self, slot, rows=None):
        """TBX_QUERY_CHECKPOINT_VALID as int8[N]: 1 cell (slot, rows[i] or i) holds an env, 0 it is empty, -1 no such cell or no store"""
        return self.reduce(_abi.QUERY_CHECKPOINT_VALID, checkpoint_args(self.n_envs, slot, rows))[:, 0].astype(np.int8)

    def lookahead(self, frames, hold=1, first=None, rest=None, seed=0, t=0, env_offset=0):
        """TBX_QUERY_LOOKAHEAD: what the next `frames` raw frames bring every env under the schedule `first` for the first `hold`
        frames, `rest` after them (ALE action ids; None: drawn by the rule of step_synthetic(seed, t + period, env_offset)) --
        computed on the device from the state as it stands and thrown away: the engine is untouched.  Every argument a scalar
        or one per env.  Returns a dict of [N] arrays: ret (float64: the sum of the positive score steps), score, lives, frames_run
        (shorter than `frames` where the game ended) and life_lost_at (the first frame that cost a life, -1: none), int64."""
        args, _ = lookahead_args(self.n_envs, frames, hold, first, rest, seed, t, env_offset)
        return self._lookahead_dict(self.reduce(_abi.QUERY_LOOKAHEAD, args))

    def lookahead_all(self, frames, hold=1, rest=None, seed=0, t=0, env_offset=0):
        """TBX_QUERY_LOOKAHEAD_ALL: lookahead() once per legal action a (self.legal_actions order) as the first action; the same dict,
        arrays shaped [N, n_legal]."""
        args, _ = lookahead_args(self.n_envs, frames, hold, None, rest, seed, t, env_offset)
        return self._lookahead_dict(self.reduce(_abi.QUERY_LOOKAHEAD_ALL, args).reshape(self.n_envs, len(self.legal_actions), 5))

    def lookahead_plan(self, frames, plan, hold=1, rest=None, seed=0, t=0, env_offset=0):
        """TBX_QUERY_LOOKAHEAD_PLAN: lookahead() under an action sequence -- plan: ALE action ids [depth] (shared) or [N, depth],
        action p held for period p (`hold` frames), `rest` after the last.  The same dict of five [N] arrays."""
        plan = np.asarray(plan, np.int64)
        if plan.ndim not in (1, 2) or (plan.ndim == 2 and plan.shape[0] != self.n_envs):
            raise ValueError("plan is [depth] or [%d, depth] action ids, got shape %r" % (self.n_envs, plan.shape))
        code = plan_code(self.game, plan)
        args, _ = plan_args(self.game, self.n_envs, frames, hold, plan.shape[-1], code if plan.ndim == 2 else int(code), rest, seed, t, env_offset)
        return self._lookahead_dict(self.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args))

    def lookahead_search(self, frames, depth, hold=1, objective="return", rest=None, seed=0, t=0, env_offset=0):
        """TBX_QUERY_LOOKAHEAD_SEARCH: all n_legal ** depth plans of every env played on the device; for each first action a
        (self.legal_actions order) the best plan that begins with it under `objective` ("return": ret, lives, the later first
        life loss; "survival": lives, the later loss, ret; ties to the smaller code).  The five lookahead() fields [N, n_legal]
        plus code [N, n_legal] (uint64) and plan [N, n_legal, depth] (ALE ids; per-env depths: the largest, unused periods -1)."""
        args, _ = search_args(self.game, self.n_envs, frames, hold, depth, objective, rest, seed, t, env_offset)
        return self._best_plans_dict(self.reduce(_abi.QUERY_LOOKAHEAD_SEARCH, args), depth)

    def lookahead_beam(self, frames, depth, width, hold=1, objective="return", rest=None, seed=0, t=0, env_offset=0):
        """TBX_QUERY_LOOKAHEAD_BEAM: beam search on the device, for plans deeper than lookahead_search can enumerate (depth up to
        PLAN_MAX_DEPTH).  For each first action a, level d keeps the `width` (1 .. BEAM_MAX_WIDTH; 1 is greedy search) best
        prefixes of depth d under `objective`, every kept prefix is extended by every action and every extension is played over
        the whole horizon with `rest` behind it.  The dict of lookahead_search: the five fields and code [N, n_legal] of the
        best plan found, plan [N, n_legal, depth].  With width >= n_legal ** (depth - 2) it is lookahead_search."""
        args, _ = beam_args(self.game, self.n_envs, frames, depth, width, hold, objective, rest, seed, t, env_offset)
        return self._best_plans_dict(self.reduce(_abi.QUERY_LOOKAHEAD_BEAM, args), depth)

    @property
    def beam_ranges(self):
        """into how many env ranges the last lookahead_beam was cut (0: none yet)"""
        return self.get_option(_abi.OPT_BEAM_RANGES)

    @property
    def beam_range_envs(self):
        """at most this many envs per range of a lookahead_beam, on top of the engine's budgets (0: the engine's choice)"""
        return self.get_option(_abi.OPT_BEAM_RANGE_ENVS)

    @beam_range_envs.setter
    def beam_range_envs(self, envs):
        self.set_option(_abi.OPT_BEAM_RANGE_ENVS, envs)

    def lookahead_evolve(self, frames, depth, population, generations, elite=None, mutation=None, plan_seed=0, init=None, hold=1, objective="return",
                         rest=None, seed=0, t=0, env_offset=0):
        """TBX_QUERY_LOOKAHEAD_EVOLVE: evolutionary search over WHOLE plans of `depth` periods on the device, with a budget the
        caller chooses and an optional warm start.  Per env and first action a population of `population` plans (generation 0:
        drawn from plan_seed; individual 0 the plan code `init`, its first action replaced, where one is given) is played, ranked
        under `objective` and bred `generations` times: the `elite` best persist, every other individual copies a drawn elite and
        redraws each later digit with probability mutation / 256.  Defaults: elite max(1, population // 4), mutation
        max(1, round(256 / max(depth - 1, 1))) -- about one digit per child.  The dict of lookahead_beam: the five fields and code
        [N, n_legal] of the best plan of the last generation, plan [N, n_legal, depth].  More generations are never worse; the
        returned code fed to lookahead_plan gives the row.  Nothing in the engine is written."""
        if elite is None:
            elite = np.maximum(1, np.asarray(population) // 4) if np.ndim(population) else max(1, int(population) // 4)
        if mutation is None:
            mutation = np.maximum(1, np.round(256 / np.maximum(np.asarray(depth) - 1, 1))) if np.ndim(depth) else max(1, round(256 / max(int(depth) - 1, 1)))
        args, _ = evolve_args(self.game, self.n_envs, frames, depth, population, generations, elite, plan_seed, mutation, init, hold, objective, rest, seed, t, env_offset)
        return self._best_plans_dict(self.reduce(_abi.QUERY_LOOKAHEAD_EVOLVE, args), depth)

    @property
    def evolve_ranges(self):
        """into how many env ranges the last lookahead_evolve was cut (0: none yet)"""
        return self.get_option(_abi.OPT_EVOLVE_RANGES)

    def lookahead_tree(self, frames, depth, simulations, explore=0, salt=0, hold=1, objective="return", rest=None, seed=0, t=0, env_offset=0):
        """TBX_QUERY_LOOKAHEAD_TREE: open-loop Monte-Carlo tree search on the device -- per env and first action a tree of action
        prefixes up to `depth` periods deep, grown by `simulations` (1 .. TREE_MAX_SIMULATIONS) futures spent adaptively: every
        simulation walks down by the priority Q + U (Q the mean value of a child in 1/256ths, U = explore x sqrt(visits of the
        parent) / (1 + visits of the child), in integers), adds at most one node and plays its prefix, `rest` behind it, on future
        m (seed sample_seed(seed, m), the game RNG salted by salt + m where salt is not 0: the futures of lookahead_samples, the
        same for all first actions).  The value is ret ("return") or the frames before the first lost life ("survival").  Returns
        a dict of [N, n_legal] arrays: the eight lookahead_samples() sums of the root (samples 0: the row was refused), then the
        principal variation -- the most visited path -- as code (uint64), pv_depth, pv_visits and pv_value (the sum of the values
        through its last node), int64.  With depth 1 the sums are lookahead_samples'.  Nothing in the engine is written."""
        args, _ = tree_args(self.game, self.n_envs, frames, depth, simulations, explore, salt, hold, objective, rest, seed, t, env_offset)
        return self._tree_dict(self.reduce(_abi.QUERY_LOOKAHEAD_TREE, args))

    def _tree_dict(self, out):
        out = np.asarray(out).reshape(self.n_envs, len(self.legal_actions), 12)
        return {k: out[..., i].astype(np.uint64 if k == "code" else np.int64) for i, k in enumerate(TREE_FIELDS)}

    @property
    def tree_ranges(self):
        """into how many env ranges the last lookahead_tree was cut (0: none yet)"""
        return self.get_option(_abi.OPT_TREE_RANGES)

    @property
    def tree_launch_simulations(self):
        """at most this many simulations per launch of a lookahead_tree, on top of the engine's budget (0: the engine's choice)"""
        return self.get_option(_abi.OPT_TREE_LAUNCH_SIMULATIONS)

    @tree_launch_simulations.setter
    def tree_launch_simulations(self, simulations):
        self.set_option(_abi.OPT_TREE_LAUNCH_SIMULATIONS, simulations)

    def lookahead_tree_act(self, frames, depth, simulations, explore=0, salt=0, reuse=False, hold=1, objective="return", rest=None, seed=0, t=0, env_offset=0):
        """TBX_QUERY_LOOKAHEAD_TREE_ACT: lookahead_tree with every env's winner picked on the device (plan_pick's sampled rule on
        the root sums) and the subtree under the winner kept in BUF_PLAN_TREE (tree_carry's rule); reuse=True starts the trees
        from what the last call kept, where the call's frames, hold, depth, objective and simulations are the same and tree_drop
        has not named the env.  Returns a dict of [N] arrays: action (the ALE id, also left in BUF_PLAN_ACTION for step_device /
        agent_step_device), action_index and the winner's TREE_FIELDS (samples = simulations; pv_visits counts carried visits
        too).  Nothing else in the engine is written."""
        args = tree_act_args(self.game, frames, depth, simulations, explore, salt, reuse, hold, objective, rest, seed, t, env_offset)
        return self._tree_act_dict(self.reduce(_abi.QUERY_LOOKAHEAD_TREE_ACT, args))

    def lookahead_tree_act_device(self, out_ptr, frames, depth, simulations, stream=0, **keywords):
        """lookahead_tree_act, asynchronous on `stream`: rows float64[N][14] = {action, action_index, the winner's tree row} into
        the device buffer at out_ptr; a step_device(plan_action_ptr, stream=stream) queued behind it reads the finished actions"""
        self.reduce_device(_abi.QUERY_LOOKAHEAD_TREE_ACT, out_ptr, tree_act_args(self.game, frames, depth, simulations, **keywords), stream=stream)

    def _tree_act_dict(self, out):
        out = np.asarray(out).reshape(self.n_envs, TREE_ACT_WIDTH)
        res = {"action": out[:, 0].astype(np.int64), "action_index": out[:, 1].astype(np.int64)}
        res.update({k: out[:, 2 + i].astype(np.uint64 if k == "code" else np.int64) for i, k in enumerate(TREE_FIELDS)})
        return res

    def tree_drop(self, mask=None):
        """TBX_EDIT_TREE_DROP, the host form: the carried trees of the masked envs (a bool array [N]; None: all) are dead for the
        next lookahead_tree_act.  Raises ToyboxAmdError(E_INVALID) before the first lookahead_tree_act."""
        self.edit(_abi.EDIT_TREE_DROP, (), mask)

    def tree_drop_device(self, mask_ptr=0, stream=0):
        """TBX_EDIT_TREE_DROP, asynchronous on `stream`: mask_ptr = device address of uint8[N] (0: every env) -- a step's done
        buffer, so that a queued loop forgets the trees of games that ended"""
        self.edit_device(_abi.EDIT_TREE_DROP, (), mask_ptr=mask_ptr, stream=stream)

    def plan_trees(self, simulations):
        """BUF_PLAN_TREE on the host after everything queued has finished, as tree_store_units gives it: [env][k] lists of
        (n, v_sum, child).  simulations: that of the call that wrote the store."""
        from . import hip
        ptr, nbytes = self.device_buffer(_abi.BUF_PLAN_TREE)
        raw = np.empty(nbytes, np.uint8)
        self.sync()
        hip.memcpy_dtoh(raw, ptr, nbytes)
        return tree_store_units(self.game, raw, self.n_envs, simulations)

    def lookahead_act(self, planner, **planner_keywords):
        """TBX_QUERY_LOOKAHEAD_ACT: the planner's query (a name of ACT_PLANNERS or its id; keywords as act_args takes them) with
        every env's winner picked on the device (plan_pick's rule).  Returns a dict of [N] arrays: action (the ALE id, also left
        in BUF_PLAN_ACTION for step_device / agent_step_device), action_index, the winner's fields (LOOKAHEAD_FIELDS, or
        SAMPLE_FIELDS for the sampled planners), code (uint64) and plan [N, depth] (digits: indices into legal_actions, the first
        being action_index).  BUF_PLAN_CARRY keeps plan_shift(code) for the evolution's init="carry" of the next call.  Nothing else
        in the engine is written."""
        args = act_args(self.game, planner, **planner_keywords)
        return self._act_dict(self.reduce(_abi.QUERY_LOOKAHEAD_ACT, args), act_planner(planner), planner_keywords.get("depth", 1))

    def lookahead_act_device(self, planner, out_ptr, stream=0, **planner_keywords):
        """lookahead_act, asynchronous on `stream`: rows float64[N][11] = {action, action_index, the winner's planner row
        zero-padded to 9} into the device buffer at out_ptr; a step_device(plan_action_ptr, stream=stream) queued behind it reads
        the finished actions"""
        self.reduce_device(_abi.QUERY_LOOKAHEAD_ACT, out_ptr, act_args(self.game, planner, **planner_keywords), stream=stream)

    @property
    def plan_action_ptr(self):
        """device address of BUF_PLAN_ACTION, int32[N]; it exists from the engine's first lookahead_act / lookahead_act_device on"""
        return self.device_buffer(_abi.BUF_PLAN_ACTION)[0]

    def plan_buffers(self):
        """(BUF_PLAN_ACTION int32[N], BUF_PLAN_CARRY uint32[N]) on the host, after everything queued has finished"""
        from . import hip
        action, carry = np.empty(self.n_envs, np.int32), np.empty(self.n_envs, np.uint32)
        pa, pc = self.device_buffer(_abi.BUF_PLAN_ACTION)[0], self.device_buffer(_abi.BUF_PLAN_CARRY)[0]
        self.sync()
        hip.memcpy_dtoh(action, pa, action.nbytes)
        hip.memcpy_dtoh(carry, pc, carry.nbytes)
        return action, carry

    def _act_dict(self, out, planner, depth):
        out = np.asarray(out).reshape(self.n_envs, 11)
        res = {"action": out[:, 0].astype(np.int64), "action_index": out[:, 1].astype(np.int64)}
        if planner in ACT_SAMPLED:
            res.update(self._samples_dict(out[:, 2:10]))
            res["code"] = out[:, 10].astype(np.uint64)
        else:
            res.update(self._lookahead_dict(out[:, 2:7]))
            res["code"] = out[:, 7].astype(np.uint64)
        res["plan"] = plan_digits(len(self.legal_actions), res["code"], int(depth))
        return res

    def _best_plans_dict(self, out, depth):
        L = len(self.legal_actions)
        out = out.reshape(self.n_envs, L, 6)
        res = self._lookahead_dict(out[..., :5])
        res["code"] = out[..., 5].astype(np.uint64)
        d = np.broadcast_to(np.clip(np.asarray(depth, np.int64), 0, _abi.PLAN_MAX_DEPTH[self.game]), (self.n_envs,))
        width = int(d.max()) if self.n_envs else 0
        plan = np.asarray(self.legal_actions, np.int64)[plan_digits(L, res["code"], width)]
        plan[np.broadcast_to(np.arange(width) >= d[:, None, None], plan.shape)] = -1
        res["plan"] = plan
        return res

    def lookahead_samples(self, frames, samples, hold=1, salt=0, rest=None, seed=0, t=0, env_offset=0):
        """TBX_QUERY_LOOKAHEAD_SAMPLES: for every env and every first action (self.legal_actions order) `samples` futures of
        `frames` raw frames, summed on the device.  Future s is lookahead_all() under seed sample_seed(seed, s) -- with rest None
        every future draws its own action stream -- and, with a salt that is not 0, with the env's game RNG salted by salt + s as
        fork(salt=...) would salt it (in registers: nothing is written).  Returns a dict of int64 [N, n_legal] arrays: samples
        (0: the row was refused), ret_sum, ret_min, ret_max, lives_sum, lost (futures that lost a life), ended (futures whose
        game ended) and safe_frames_sum (frames before the first lost life, summed)."""
        args, _ = sample_args(self.game, self.n_envs, frames, samples, hold, salt, rest, seed, t, env_offset)
        out = self.reduce(_abi.QUERY_LOOKAHEAD_SAMPLES, args).reshape(self.n_envs, len(self.legal_actions), 8)
        return self._samples_dict(out)

    @staticmethod
    def _samples_dict(out):
        return {k: out[..., i].astype(np.int64) for i, k in enumerate(SAMPLE_FIELDS)}

    def lookahead_search_samples(self, frames, depth, samples, hold=1, objective="return", salt=0, rest=None, seed=0, t=0, env_offset=0):
        """TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES: all n_legal ** depth plans of every env, each played on the SAME `samples` futures
        (future s: seed sample_seed(seed, s) and, with a salt that is not 0, the game RNG salted by salt + s, as in
        lookahead_samples); for each first action a (self.legal_actions order) the best plan that begins with it by the summed
        outcome -- "return": the larger ret_sum, then the smaller lost, then the larger safe_frames_sum; "survival": the smaller
        lost, the larger safe_frames_sum, the larger ret_sum; ties to the smaller code.  The eight lookahead_samples() fields of
        that plan, int64 [N, n_legal] (samples 0: the row was refused), plus code [N, n_legal] (uint64) and plan
        [N, n_legal, depth] (ALE ids; per-env depths: the largest, unused periods -1).  Nothing in the engine is written."""
        args, _ = search_samples_args(self.game, self.n_envs, frames, depth, samples, hold, objective, salt, rest, seed, t, env_offset)
        L = len(self.legal_actions)
        out = self.reduce(_abi.QUERY_LOOKAHEAD_SEARCH_SAMPLES, args).reshape(self.n_envs, L, 9)
        return self._search_samples_dict(out, depth)

    def lookahead_beam_samples(self, frames, depth, width, samples, hold=1, objective="return", salt=0, rest=None, seed=0, t=0, env_offset=0):
        """TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES: lookahead_beam with every candidate judged on the SAME `samples` futures (future s:
        seed sample_seed(seed, s) and, with a salt that is not 0, the game RNG salted by salt + s, as in lookahead_samples) -- plans
        up to PLAN_MAX_DEPTH deep by their summed outcome.  Level d keeps the `width` best prefixes of depth d under the order of
        lookahead_search_samples ("return": the larger ret_sum, the smaller lost, the larger safe_frames_sum; "survival": the smaller
        lost, the larger safe_frames_sum, the larger ret_sum; ties to the smaller code).  The dict of lookahead_search_samples: the
        eight sums, int64 [N, n_legal] (samples 0: the row was refused), code (uint64) and plan [N, n_legal, depth].  With depth 1
        the sums are lookahead_samples'; with width >= n_legal ** (depth - 2) it is lookahead_search_samples where that accepts
        the depth.  Nothing in the engine is written."""
        args, _ = beam_samples_args(self.game, self.n_envs, frames, depth, width, samples, hold, objective, salt, rest, seed, t, env_offset)
        L = len(self.legal_actions)
        out = self.reduce(_abi.QUERY_LOOKAHEAD_BEAM_SAMPLES, args).reshape(self.n_envs, L, 9)
        return self._search_samples_dict(out, depth)

    @property
    def beam_samples_ranges(self):
        """into how many env ranges the last lookahead_beam_samples was cut (0: none yet)"""
        return self.get_option(_abi.OPT_BEAM_SAMPLES_RANGES)

    @property
    def beam_samples_chunks(self):
        """the largest number of sample chunks any level of the last lookahead_beam_samples used (0: none yet)"""
        return self.get_option(_abi.OPT_BEAM_SAMPLES_CHUNKS)

    def _search_samples_dict(self, out, depth):
        L = len(self.legal_actions)
        res = self._samples_dict(out[..., :8])
        res["code"] = out[..., 8].astype(np.uint64)
        d = np.broadcast_to(np.clip(np.asarray(depth, np.int64), 0, _abi.PLAN_MAX_DEPTH[self.game]), (self.n_envs,))
        width = int(d.max()) if self.n_envs else 0
        plan = np.asarray(self.legal_actions, np.int64)[plan_digits(L, res["code"], width)]
        plan[np.broadcast_to(np.arange(width) >= d[:, None, None], plan.shape)] = -1
        res["plan"] = plan
        return res

    @property
    def search_samples_chunks(self):
        """into how many chunks the last lookahead_search_samples cut every (env, first action) group of plans (0: none yet)"""
        return self.get_option(_abi.OPT_SEARCH_SAMPLES_CHUNKS)

    @property
    def search_samples_launches(self):
        """into how many launches over env ranges the last lookahead_search_samples was cut (0: none yet)"""
        return self.get_option(_abi.OPT_SEARCH_SAMPLES_LAUNCHES)

    @property
    def sample_chunks(self):
        """into how many chunks the last lookahead_samples cut the samples of every (env, first action) group (0: none yet)"""
        return self.get_option(_abi.OPT_SAMPLE_CHUNKS)

    @property
    def search_chunks(self):
        """into how many chunks the last lookahead_search cut every (env, first action) group of plans (0: none yet)"""
        return self.get_option(_abi.OPT_SEARCH_CHUNKS)

    @staticmethod
    def _lookahead_dict(out):
        return {k: (out[..., i].copy() if i == 0 else out[..., i].astype(np.int64)) for i, k in enumerate(LOOKAHEAD_FIELDS)}

    def reduce(self, query, args=()):
        """tbx_reduce: a per-env feature as float64 [N, width] (integers are exact; missing entries read -1)"""
        width = self._lib.tbx_reduce_width(_abi.GAME_IDS[self.game], int(query))
        if width < 0:
            raise ToyboxAmdError(width, "unknown query %d for %s" % (query, self.game))
        a, n, per_env = self._edit_args(args)
        out = np.empty((self.n_envs, width), np.float64)
        self._check(self._lib.tbx_reduce(self._h, int(query), _ptr(a) if n else None, n, per_env, _ptr(out)))
        return out

    def edit_device(self, op, args=(), mask_ptr=0, stream=0, per_env_ptr=0, n_args=0):
        """tbx_edit_device, asynchronous on `stream`: mask_ptr = device address of uint8[N] (0: every env); arguments either
        `args` (scalars, the same for every env) or per_env_ptr = device address of float64[N][n_args]"""
        if per_env_ptr:
            self._check(self._lib.tbx_edit_device(self._h, int(op), C.c_void_p(int(per_env_ptr)), int(n_args), 1,
                                                  C.c_void_p(int(mask_ptr)) if mask_ptr else None, C.c_void_p(int(stream))))
            return
        a, n, _ = self._edit_args(args)
        self._check(self._lib.tbx_edit_device(self._h, int(op), _ptr(a) if n else None, n, 0, C.c_void_p(int(mask_ptr)) if mask_ptr else None,
                                              C.c_void_p(int(stream))))

    def reduce_device(self, query, out_ptr, args=(), stream=0, per_env_ptr=0, n_args=0):
        """tbx_reduce_device: float64[N][width] into the device buffer at out_ptr, asynchronous on `stream`"""
        if per_env_ptr:
            self._check(self._lib.tbx_reduce_device(self._h, int(query), C.c_void_p(int(per_env_ptr)), int(n_args), 1, C.c_void_p(int(out_ptr)),
                                                    C.c_void_p(int(stream))))
            return
        a, n, _ = self._edit_args(args)
        self._check(self._lib.tbx_reduce_device(self._h, int(query), _ptr(a) if n else None, n, 0, C.c_void_p(int(out_ptr)), C.c_void_p(int(stream))))

    def reduce_width(self, query):
        return self._lib.tbx_reduce_width(_abi.GAME_IDS[self.game], int(query))

    def query(self, env, query_id, args, n_out=2):
        a = (C.c_int32 * len(args))(*[int(v) for v in args])
        out = (C.c_int32 * n_out)()
        self._check(self._lib.tbx_query(self._h, int(env), int(query_id), a, len(args), out, n_out))
        return [int(v) for v in out]

    # ------------------------------------------------------------------ agent-side preprocessing (fused wrapper stack)
    def agent_init(self, skip=4, out_h=84, out_w=84, stack=4, clip_reward=True, episodic_life=False, fire_reset=False,
                   noop_max=0, noop_seed=0, env_offset=0, stack_fill=0, new_plane=False):
        """stack_fill: what a reset leaves in the older stack slots -- 0 zeros (VecFrameStack), 1 the reset observation (the
        per-env FrameStack of wrap_deepmind(frame_stack=True)).  new_plane = 1 / True: the device also keeps every stack's newest
        plane alone (TBX_BUF_AGENT_PLANE) -- what a host-side frame stack receives per step.  new_plane = 2: the plane INSTEAD
        of the stack -- a ring of the last `stack` planes (TBX_BUF_AGENT_RING, agent_ring_head()); agent_reset / agent_step
        return None for the observation, agent_fetch / agent_step_begin deliver plane= only."""
        cfg = _abi.AgentConfig(int(skip), int(out_h), int(out_w), int(stack), int(bool(clip_reward)), int(bool(episodic_life)),
                               int(bool(fire_reset)), int(noop_max), int(noop_seed), int(env_offset), int(stack_fill), int(new_plane))
        self._check(self._lib.tbx_agent_init(self._h, C.byref(cfg)))
        self._agent_shape = (self.n_envs, int(out_h), int(out_w), int(stack))
        self._agent_ring = int(new_plane) == 2

    def agent_ring_head(self):
        """new_plane = 2: the slot of TBX_BUF_AGENT_RING (uint8[stack][N][h][w]) that holds the newest plane; env i's stack, oldest
        first, is ring[(head + 1 + c) % stack][i], c = 0 .. stack - 1"""
        h = C.c_int32()
        self._check(self._lib.tbx_agent_ring_head(self._h, C.byref(h)))
        return int(h.value)

    def agent_set_noops(self, counts):
        """NoopResetEnv.override_num_noops per env (counts[i] > 0 overrides, 0 keeps the default rule); None removes it."""
        if counts is None:
            self._check(self._lib.tbx_agent_set_noops(self._h, None))
            return
        a = np.ascontiguousarray(counts, dtype=np.int32)
        if a.shape != (self.n_envs,):
            raise ValueError("counts must have shape (%d,)" % self.n_envs)
        self._check(self._lib.tbx_agent_set_noops(self._h, _ptr(a)))

    def _agent_obs_array(self, out):
        if out is None:
            return np.empty(self._agent_shape, np.uint8)
        if out.shape != tuple(self._agent_shape) or out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous uint8 array of shape %r" % (tuple(self._agent_shape),))
        return out

    def agent_reset(self, out=None):
        obs = None if self._agent_ring else self._agent_obs_array(out)
        self._check(self._lib.tbx_agent_reset(self._h, _ptr(obs)))
        return obs

    def agent_step(self, actions, tolerate_needs_reset=False, out=None):
        """actions: ALE ids.  Returns (obs uint8[N,oh,ow,stack], reward float32[N], done bool[N]); `out`: the array the
        observations go into (a reused page-locked one takes them at the PCIe link's rate).
        TBX_E_NEEDS_RESET (where bench.Monitor raises) is raised like every other error unless tolerate_needs_reset: the step
        has been carried out either way and the outputs are valid."""
        a = np.ascontiguousarray(actions, dtype=np.int32)
        if a.shape != (self.n_envs,):
            raise ValueError("actions must have shape (%d,)" % self.n_envs)
        obs = None if self._agent_ring else self._agent_obs_array(out)
        reward = np.empty(self.n_envs, np.float32)
        done = np.empty(self.n_envs, np.uint8)
        rc = self._lib.tbx_agent_step(self._h, _ptr(a), _ptr(reward), _ptr(done), _ptr(obs))
        if not (tolerate_needs_reset and rc == _abi.E_NEEDS_RESET):
            self._check(rc)
        return obs, reward, done.astype(bool)

    def agent_episodes(self):
        """Episode monitor of the last agent step: (ended bool[N], return float32[N], length int32[N])."""
        n = self.n_envs
        ended, ret, length = np.empty(n, np.uint8), np.empty(n, np.float32), np.empty(n, np.int32)
        self._check(self._lib.tbx_agent_episodes(self._h, _ptr(ended), _ptr(ret), _ptr(length)))
        return ended.astype(bool), ret, length

    # ------------------------------------------------------------------ host delivery: step_async / step_wait
    def host_array(self, shape, dtype=np.uint8):
        """A numpy array over page-locked host memory of the engine's library (tbx_host_alloc): the destination of the
        asynchronous copies of step_begin / agent_step_begin.  The memory lives as long as the array or any view of it."""
        return HostArray.make(self._lib, shape, dtype)

    def host_stack_push(self, dst, src, plane, done=None, reset=False, fill_repeat=False, threads=0):
        """tbx_host_stack_push: dst = VecFrameStack's next stackedobs (uint8[N, h, w, stack]) from src (may be dst itself), the
        newly received plane uint8[N, h, w] and the done flags -- the roll of vec_frame_stack.py:17-27 as threaded host code"""
        n, h, w, k = dst.shape
        if src.shape != dst.shape or plane.shape != (n, h, w) or dst.dtype != np.uint8 or src.dtype != np.uint8 or plane.dtype != np.uint8:
            raise ValueError("host_stack_push: uint8 stacks [N, h, w, stack] and a uint8 plane [N, h, w] are needed")
        d = None
        if done is not None:
            d = np.ascontiguousarray(done, dtype=np.uint8)
            if d.shape != (n,):
                raise ValueError("done must have one entry per env")
        rc = self._lib.tbx_host_stack_push(_addr(dst), _addr(src), _addr(plane), _ptr(d), int(bool(reset)), n, h * w, k,
                                           int(bool(fill_repeat)), int(threads))
        if rc != _abi.OK:
            msg = self._lib.tbx_last_error(None)
            raise ToyboxAmdError(rc, msg.decode() if msg else "tbx_host_stack_push failed")
        return dst

    def agent_step_begin(self, actions, reward=None, done=None, obs=None, plane=None, ep_done=None, ep_return=None, ep_length=None):
        """tbx_agent_step_begin: queues actions -> device, the agent step and the copies of the requested outputs into the given
        host arrays (C-contiguous, of the documented dtypes; page-locked ones from host_array() keep the call asynchronous);
        returns at once.  agent_step_end() waits."""
        a = np.ascontiguousarray(actions, dtype=np.int32)
        if a.shape != (self.n_envs,):
            raise ValueError("actions must have shape (%d,)" % self.n_envs)
        out = _abi.AgentHostOut(*[_addr(x) for x in (reward, done, obs, plane, ep_done, ep_return, ep_length)])
        self._host_keep = (a, reward, done, obs, plane, ep_done, ep_return, ep_length)     # alive until the step has ended
        self._check(self._lib.tbx_agent_step_begin(self._h, _ptr(a), C.byref(out)))

    def agent_step_end(self, tolerate_needs_reset=False):
        rc = self._lib.tbx_agent_step_end(self._h)
        self._host_keep = None
        if not (tolerate_needs_reset and rc == _abi.E_NEEDS_RESET):
            self._check(rc)

    def agent_fetch(self, reward=None, done=None, obs=None, plane=None, ep_done=None, ep_return=None, ep_length=None):
        """the current contents of the agent layer's output buffers (after agent_reset or a step), synchronous"""
        out = _abi.AgentHostOut(*[_addr(x) for x in (reward, done, obs, plane, ep_done, ep_return, ep_length)])
        self._check(self._lib.tbx_agent_fetch(self._h, C.byref(out)))

    def step_begin(self, actions, auto_reset=False, reward=None, done=None, lives=None, score=None, frame=None, channels=3):
        """tbx_step_begin: one frame for every env plus (frame given) the picture of the state it leaves, queued; step_end() waits.
        reward / lives / score int32[N], done uint8[N], frame uint8[N, H, W, channels]."""
        a = np.ascontiguousarray(actions, dtype=np.int32)
        if a.shape != (self.n_envs,):
            raise ValueError("actions must have shape (%d,)" % self.n_envs)
        out = _abi.StepHostOut(_addr(reward), _addr(done), _addr(lives), _addr(score), _addr(frame), int(channels), 0)
        self._host_keep = (a, reward, done, lives, score, frame)
        self._check(self._lib.tbx_step_begin(self._h, _ptr(a), _abi.STEP_AUTO_RESET if auto_reset else 0, C.byref(out)))

    def step_end(self):
        rc = self._lib.tbx_step_end(self._h)
        self._host_keep = None
        self._check(rc)

    def agent_step_synthetic(self, action_seed, t, env_offset=0, stream=0):
        self._check(self._lib.tbx_agent_step_synthetic(self._h, int(action_seed), int(t), int(env_offset), C.c_void_p(int(stream))))

    def agent_step_device(self, actions_ptr, stream=0):
        self._check(self._lib.tbx_agent_step_device(self._h, C.c_void_p(int(actions_ptr)), C.c_void_p(int(stream))))

    # ------------------------------------------------------------------ device-resident path
    def step_device(self, actions_ptr, auto_reset=False, stream=0):
        flags = _abi.STEP_AUTO_RESET if auto_reset else 0
        self._check(self._lib.tbx_step_device(self._h, C.c_void_p(int(actions_ptr)), flags, C.c_void_p(int(stream))))

    def step_synthetic(self, action_seed, t, env_offset=0, auto_reset=True, stream=0):
        flags = _abi.STEP_AUTO_RESET if auto_reset else 0
        self._check(self._lib.tbx_step_synthetic(self._h, int(action_seed), int(t), int(env_offset), flags,
                                                 C.c_void_p(int(stream))))

    def render_device(self, out_ptr=0, channels=3, stream=0):
        self._check(self._lib.tbx_render_device(self._h, C.c_void_p(int(out_ptr)) if out_ptr else None,
                                                int(channels), C.c_void_p(int(stream))))

    def render_step_synthetic(self, action_seed, t, out_ptr=0, channels=3, env_offset=0, auto_reset=True, stream=0):
        """tbx_render_step_synthetic: the frame of the current state into out_ptr (0: TBX_BUF_FRAME) and one step with
        device-generated actions, one launch where the rasteriser reads step-written records (random-rollout loops only)."""
        flags = _abi.STEP_AUTO_RESET if auto_reset else 0
        self._check(self._lib.tbx_render_step_synthetic(self._h, C.c_void_p(int(out_ptr)) if out_ptr else None, int(channels),
                                                        int(action_seed), int(t), int(env_offset), flags, C.c_void_p(int(stream))))

    def device_identity(self):
        """tbx_device_identity: which device this engine drives -- {"ordinal", "pci" ("dddd:bb:dd"), "arch", "name", "total_memory",
        "compute_units"}; the CPU checker reports ordinal -1 and arch "cpu-oracle"."""
        d = _abi.DeviceIdentity()
        self._check(self._lib.tbx_device_identity(self._h, C.byref(d)))
        return {"ordinal": int(d.ordinal), "pci": "%04x:%02x:%02x" % (d.pci_domain & 0xFFFF, d.pci_bus & 0xFF, d.pci_device & 0xFF) if d.ordinal >= 0 else None,
                "arch": d.arch.decode(), "name": d.name.decode(), "total_memory": int(d.total_memory), "compute_units": int(d.compute_units)}

    def rollout_synthetic(self, action_seed, t0, k, channels=3, env_offset=0, auto_reset=True, stream=0):
        """tbx_rollout_synthetic: k consecutive render_step_synthetic calls (each followed by gather() under a K-step record ring, K = k)
        as one -- frames in BUF_ROLLOUT_FRAMES [k, N, H, W, C], step records in BUF_ROLLOUT_PACKED [k, stride].  Where the engine can
        (Breakout, SpaceInvaders; RGB / RGBA) the chunk's steps on an internal stream + its rasteriser launches on others (OPT_ROLLOUT_CHUNKS)."""
        flags = _abi.STEP_AUTO_RESET if auto_reset else 0
        self._check(self._lib.tbx_rollout_synthetic(self._h, int(channels), int(action_seed), int(t0), int(k), int(env_offset), flags,
                                                    C.c_void_p(int(stream))))

    def device_buffer(self, which):
        p, b = C.c_void_p(), C.c_size_t()
        self._check(self._lib.tbx_device_buffer(self._h, int(which), C.byref(p), C.byref(b)))
        return (p.value or 0), b.value

    # ------------------------------------------------------------------ multi-GPU record gather (RCCL behind the C-ABI)
    def gather_unique_id(self):
        """rank 0: bytes of a fresh communicator id, to be handed to every rank out of band."""
        buf = (C.c_uint8 * _abi.GATHER_ID_BYTES)()
        rc = self._lib.tbx_gather_unique_id(buf, _abi.GATHER_ID_BYTES)
        if rc != _abi.OK:
            msg = self._lib.tbx_last_error(None)
            raise ToyboxAmdError(rc, msg.decode() if msg else "tbx_gather_unique_id failed")
        return bytes(buf)

    def gather_init(self, nranks, rank, unique_id, records_per_rank=None):
        width = self.n_envs if records_per_rank is None else int(records_per_rank)
        buf = (C.c_uint8 * _abi.GATHER_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._check(self._lib.tbx_gather_init(self._h, int(nranks), int(rank), width, buf, _abi.GATHER_ID_BYTES))
        k = self._lib.tbx_gather_every(self._h)
        self._gather_shape = (int(nranks), width) if k <= 1 else (int(nranks), k, width)

    def gather(self, out_ptr=0, stream=0):
        self._check(self._lib.tbx_gather(self._h, C.c_void_p(int(out_ptr)) if out_ptr else None, C.c_void_p(int(stream))))

    def gather_wait(self, stream=0):
        self._check(self._lib.tbx_gather_wait(self._h, C.c_void_p(int(stream))))

    def gather_every(self):
        """K of the record ring the communicator was initialised with (OPT_GATHER_EVERY at gather_init)"""
        return self._lib.tbx_gather_every(self._h)

    def gather_fill(self):
        """steps whose records wait in the ring for the next collective"""
        return self._lib.tbx_gather_fill(self._h)

    def gather_host(self):
        """uint64[nranks, records_per_rank] -- [nranks, K, records_per_rank] with a K-step ring -- of the last queued gather
        (blocks until it has finished)."""
        out = np.empty(self._gather_shape, np.uint64)
        self._check(self._lib.tbx_gather_host(self._h, _ptr(out)))
        return out

    def gather_nranks(self):
        """ranks the communicator spans, as the collective library itself reports it"""
        n = self._lib.tbx_gather_nranks(self._h)
        if n < 0:
            self._check(n)
        return n

    def gather_library(self):
        return (self._lib.tbx_gather_library(self._h) or b"").decode()

    def gather_reduce_max(self, value):
        v = C.c_double(float(value))
        self._check(self._lib.tbx_gather_reduce_max(self._h, C.byref(v)))
        return v.value

    def sync(self):
        self._check(self._lib.tbx_sync(self._h))
