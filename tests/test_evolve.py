"""Evolutionary plan search (TBX_QUERY_LOOKAHEAD_EVOLVE), the part that needs no GPU: the constants, the argument shaping, the words
and generation 0 of the product against the replay's own, and the yardstick of tests/test_gpu_evolve.py under test itself over the
CPU checker alone (tests/evolve_replay.py): the six consequences the header states, elites carried or replayed, refused rows, and
that the GPU module's cases cover what they must (the counts and replay times of each case are printed)."""
import functools
import os
import re
import time

import numpy as np
import pytest

from conftest import ROOT
from evolve_replay import (EVOLVE_SHAPES, MAX_GENERATIONS, MAX_POPULATION, base_word, case_evolve, evolve_stats, expected_evolve, generation0, missing_coverage,
                           not_worse, word)
from fork_replay import sim_rngs
from lookahead_replay import FIELDS, batch
from search_replay import SEARCH_FIELDS, assert_search_equal, expected_plan, expected_search
from support import LEGAL
from toybox_amd import Engine, ToyboxAmdError, _abi
from toybox_amd.engine import beam_args, evolve_args, evolve_generation0, evolve_word

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
HEADER = open(os.path.join(ROOT, "include", "toybox_amd.h")).read()


def test_header_and_python_agree_on_the_constants():
    want = {"TBX_QUERY_LOOKAHEAD_EVOLVE": (_abi.QUERY_LOOKAHEAD_EVOLVE, 158), "TBX_EVOLVE_MAX_POPULATION": (_abi.EVOLVE_MAX_POPULATION, 256),
            "TBX_EVOLVE_MAX_GENERATIONS": (_abi.EVOLVE_MAX_GENERATIONS, 64), "TBX_OPT_EVOLVE_RANGES": (_abi.OPT_EVOLVE_RANGES, 114)}
    for name, (py, value) in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, HEADER)
        assert m and int(m.group(1)) == py == value, name
    assert re.search(r"#define\s+TBX_QUERY_LOOKAHEAD_EVOLVE\s+158\s*/\*.*env_offset,\s*population, generations, elite, plan_seed, mutation, init\}\s*->\s*6\s*\*\s*n_legal",
                     HEADER), "columns and width stand on the #define line"
    assert (MAX_POPULATION, MAX_GENERATIONS) == (_abi.EVOLVE_MAX_POPULATION, _abi.EVOLVE_MAX_GENERATIONS)
    assert re.search(r"#define\s+TBX_ABI_VERSION\s+1\b", HEADER)
    for consequence in ("(i) ", "(ii) ", "(iii) ", "(iv) ", "(v) ", "(vi) "):
        assert consequence in HEADER, "the header states consequence %s" % consequence


def test_the_checker_has_no_evolve(oracle_lib):
    """the expected values cannot come from the checker's own: it answers "unknown query\""""
    with Engine("breakout", 4, lib=oracle_lib) as e:
        for call in (lambda: e.lookahead_evolve(8, 2, 2, 1), lambda: e.reduce(158, [8])):
            with pytest.raises(ToyboxAmdError) as ei:
                call()
            assert ei.value.code == _abi.E_INVALID


# ---------------------------------------------------------------- the argument shaping

def test_evolve_args_columns():
    assert evolve_args("breakout", 8, 16, 1) == ([16.0, 1.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 64.0, -1.0], False)
    seed = (0xDEADBEEF << 32) | 0x12345678
    args, per_env = evolve_args("space_invaders", 8, 300, 12, 256, 64, 256, 2 ** 32 - 1, 256, 6 ** 12 - 1, hold=4, objective="survival", rest=11, seed=seed, t=77,
                                env_offset=4096)
    assert per_env is False and args == [300.0, 4.0, 12.0, 1.0, 11.0, float(0x12345678), float(0xDEADBEEF), 77.0, 4096.0, 256.0, 64.0, 256.0, float(2 ** 32 - 1), 256.0,
                                         float(6 ** 12 - 1)]
    assert len(args) == 15 < _abi.EDIT_MAX_ARGS
    # columns 0 .. 8 are the beam's; the largest Breakout code is exact in binary64
    assert evolve_args("amidar", 8, 64, 4, 3, hold=4, objective=1, rest=0, seed=5)[0][:9] == beam_args("amidar", 8, 64, 4, 3, hold=4, objective=1, rest=0, seed=5)[0][:9]
    assert evolve_args("breakout", 2, 64, 16, init=2 ** 32 - 1)[0][14] == 4294967295.0 and evolve_args("breakout", 2, 64, 16, init=None)[0][14] == -1.0
    for game in GAMES:
        assert evolve_args(game, 2, 8, _abi.PLAN_MAX_DEPTH[game], 2)[0][2] == float(_abi.PLAN_MAX_DEPTH[game])
    n = 6
    args, per_env = evolve_args("gridworld", n, 8, np.array([0, 1, 5, 13, 99, -3]), np.array([1, 256, 0, 257, 2, 3]), elite=np.array([1, 2, 3, 4, 5, 6]),
                                init=np.array([-1, 0, 7, -2, 5 ** 13, 1]), objective=np.array([0, 1, 2, 0, 0, 0]), rest=np.full(n, 17))
    assert per_env is True and args.shape == (n, 15) and args.dtype == np.float64      # per-env rows are checked on the device, not here
    assert args[:, 2].tolist() == [0, 1, 5, 13, 99, -3] and args[:, 9].tolist() == [1, 256, 0, 257, 2, 3] and args[:, 11].tolist() == [1, 2, 3, 4, 5, 6]
    assert args[:, 10].tolist() == [0] * n and args[:, 13].tolist() == [64] * n and args[:, 14].tolist() == [-1, 0, 7, -2, 5 ** 13, 1]
    args, per_env = evolve_args("breakout", n, np.arange(1, n + 1), 3, 4, 2, 2)
    assert per_env is True and args[:, 9].tolist() == [4] * n and args[:, 10].tolist() == [2] * n and args[:, 11].tolist() == [2] * n


@pytest.mark.parametrize("bad", [dict(frames=0), dict(frames=1025), dict(hold=0), dict(depth=0), dict(depth=17), dict(population=0), dict(population=257),
                                 dict(generations=-1), dict(generations=65), dict(elite=0), dict(elite=5), dict(plan_seed=-1), dict(plan_seed=2 ** 32),
                                 dict(mutation=-1), dict(mutation=257), dict(init=-2), dict(init=16), dict(objective=2), dict(objective="score"), dict(rest=2),
                                 dict(depth=np.ones(5)), dict(population=np.ones(5)), dict(elite=np.ones((6, 1))), dict(init=np.zeros(7)),
                                 dict(objective=np.zeros(7)), dict(env_offset=-3), dict(seed=2 ** 64), dict(t=2 ** 32)])
def test_evolve_args_range_and_shape_errors(bad):
    kw = dict(frames=8, depth=2, population=4, generations=2, elite=2)
    kw.update(bad)
    with pytest.raises(ValueError):
        evolve_args("breakout", 6, **kw)


def test_the_products_words_and_generation_0_are_the_replays():
    rng = np.random.default_rng(5)
    for _ in range(200):
        plan_seed, env, a = int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 33)), int(rng.integers(0, 6))
        g, i, p = int(rng.integers(0, 65)), int(rng.integers(0, 256)), int(rng.integers(0, 16))
        assert evolve_word(plan_seed, env, a, g, i, p) == word(base_word(plan_seed, a, env), g, i, p)
    # the text of the header, once more, on one word
    from evolve_replay import splitmix64
    assert evolve_word(7, 70003, 2, 3, 9, 4) == splitmix64(splitmix64(splitmix64(7 ^ (2 << 32)) ^ 70003) ^ (3 << 40) ^ (9 << 8) ^ 4)
    for game in GAMES:
        L, depth = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
        for a in range(L):
            for init in (None, L ** depth - 1):
                got = evolve_generation0(game, depth, 9, 123, 70001, a, init=init)
                want = generation0(L, depth, 9, base_word(123, a, 70001), a, -1 if init is None else init)
                assert got.dtype == np.uint64 and [int(c) for c in got] == want and all(c % L == a and c < L ** depth for c in want)
                assert init is None or want[0] == L ** depth - L + a
        assert len(set(generation0(L, depth, 64, base_word(1, 0, 0), 0))) > 32, "the draws are not one value"


# ---------------------------------------------------------------- the yardstick, on the checker alone

N = 8


@pytest.fixture(scope="module")
def batches(oracle_lib):
    out = {}
    for game in GAMES:
        e = batch(oracle_lib, game, N)
        out[game] = (e.get_states(), sim_rngs(e))
        e.close()
    return out


def _equal(x, y):
    return all(np.array_equal(np.asarray(x[k], np.float64), np.asarray(y[k], np.float64)) for k in SEARCH_FIELDS)


@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("game", GAMES)
def test_the_consequences_hold_for_the_replay(game, objective, batches, oracle_lib):
    states, rngs = batches[game]
    L, depth = len(LEGAL[game]), 3
    sched = dict(frames=28, hold=4, rest=LEGAL[game][1], seed=3, t=9)
    ev = dict(sched, depth=depth, objective=objective, population=6, elite=2, mutation=128, plan_seed=11)
    # (i) one individual, no generation, an init: the plan query's row for the init with its first digit replaced
    c = np.arange(N) * 7 % L ** depth
    one, _ = expected_evolve(oracle_lib, game, states, rngs, dict(sched, depth=depth, objective=objective, init=c))
    for a in range(L):
        plan = expected_plan(oracle_lib, game, states, rngs, dict(sched, depth=depth, code=c - c % L + a))
        assert np.array_equal(one["code"][:, a], c - c % L + a) and all(np.array_equal(one[k][:, a], plan[k]) for k in FIELDS), (game, a)
    # (ii) more generations are not worse, and generations 0 .. G are the same populations; carried elites = replayed elites
    rows, gens = zip(*[expected_evolve(oracle_lib, game, states, rngs, dict(ev, generations=G)) for G in range(4)])
    for G in range(3):
        assert not_worse(objective, rows[G + 1], rows[G]).all(), (game, G)
        assert all(np.array_equal(gens[G + 1][g][k], gens[G][g][k]) for g in range(G + 1) for k in ("code", "rank") + FIELDS)
    replayed, _ = expected_evolve(oracle_lib, game, states, rngs, dict(ev, generations=3), replay_elites=True)
    assert _equal(replayed, rows[3]), "the rows depend on whether elites are replayed or carried"
    # (iii) the returned code reproduces the row
    for a in range(L):
        plan = expected_plan(oracle_lib, game, states, rngs, dict(sched, depth=depth, code=rows[3]["code"][:, a]))
        assert all(np.array_equal(rows[3][k][:, a], plan[k]) for k in FIELDS) and (rows[3]["code"][:, a] % L == a).all()
    # (iv) the exhaustive search is not worse
    search = expected_search(oracle_lib, game, states, rngs, dict(sched, depth=depth, objective=objective))
    assert not_worse(objective, search, rows[3]).all() and (rows[3]["frames_run"] > 0).all()
    # (v) elite = population, or no mutation: generation 0's winner whatever G is
    for still in (dict(elite=6), dict(mutation=0)):
        assert _equal(expected_evolve(oracle_lib, game, states, rngs, dict(ev, generations=2, **still))[0], rows[0]), (game, still)
    # (vi) depth 1: the plan query's row for code a
    flat, _ = expected_evolve(oracle_lib, game, states, rngs, dict(ev, depth=1, generations=2))
    for a in range(L):
        plan = expected_plan(oracle_lib, game, states, rngs, dict(sched, depth=1, code=a))
        assert (flat["code"][:, a] == a).all() and all(np.array_equal(flat[k][:, a], plan[k]) for k in FIELDS)


def test_refused_evolve_rows_are_zero_and_leave_the_others(batches, oracle_lib):
    game = "breakout"
    states, rngs = batches[game]
    cols = dict(depth=np.full(N, 3), population=np.full(N, 4), generations=np.full(N, 1), elite=np.full(N, 2), init=np.full(N, -1), frames=np.full(N, 24))
    cols["depth"][0], cols["population"][1], cols["population"][2], cols["elite"][3], cols["init"][4], cols["generations"][5] = 17, 0, 257, 5, 64, 65
    got, _ = expected_evolve(oracle_lib, game, states, rngs, dict(cols, hold=4, rest=0))
    plain, _ = expected_evolve(oracle_lib, game, states, rngs, dict(frames=24, hold=4, depth=3, population=4, generations=1, elite=2, rest=0))
    bad = np.isin(np.arange(N), [0, 1, 2, 3, 4, 5])
    for k in SEARCH_FIELDS:
        assert (got[k][bad] == 0).all() and np.array_equal(got[k][~bad], plain[k][~bad]), k
    assert (plain["frames_run"] > 0).all()


# ---------------------------------------------------------------- the GPU module's cases cover what they must

@functools.lru_cache(maxsize=None)
def case_counts(oracle_lib, game, name):
    ev, n, batch_frames = case_evolve(game, name)
    e = batch(oracle_lib, game, n, frames=batch_frames)
    states, rngs = e.get_states(), sim_rngs(e)
    e.close()
    counts = {}
    t0 = time.perf_counter()
    for o in (0, 1):
        _, gens = expected_evolve(oracle_lib, game, states, rngs, dict(ev, objective=o))
        for k, v in evolve_stats(game, gens, o, ev["depth"]).items():
            counts[k] = counts.get(k, 0) + int(v)
    print(game, name, EVOLVE_SHAPES[name], "replay of both objectives %.1f s" % (time.perf_counter() - t0), counts)
    return counts


@pytest.mark.parametrize("game", GAMES)
def test_the_cases_cover_what_they_must(game, oracle_lib):
    """over a game's evolve cases (tests/evolve_replay.py, EVOLVE_SHAPES), on the replay alone: a group whose final winner is not
    generation 0's, a rank decided by the code alone, a population holding a duplicate code, a child that keeps at least one and
    changes at least one of its parent's digits, and an env with an ended individual"""
    totals = {}
    for name in EVOLVE_SHAPES:
        for k, v in case_counts(oracle_lib, game, name).items():
            totals[k] = totals.get(k, 0) + int(v)
    missing = missing_coverage(game, totals)
    assert not missing, "%s: the evolve cases together never show: %s" % (game, ", ".join(missing))


# ---------------------------------------------------------------- the adapters

def test_the_adapters_map_action_indices_steps_and_the_init_plan(monkeypatch):
    """ToyboxVecEnv.evolve_search: frames = steps, hold = 1; ToyboxPreprocVecEnv: frames = steps x skip, hold = skip; `rest` and
    init_plan action indices going in, plans action indices coming out; best_action / best_plan as search() picks them; a pending
    step ends first"""
    from toybox_amd.envs import vec_env
    lut = np.asarray(LEGAL["space_invaders"], np.int32)
    L = len(lut)

    class FakeEngine:
        legal_actions = list(lut)

        def lookahead_evolve(self, frames, depth, population, generations, **kw):
            self.call = (frames, depth, population, generations, kw)
            ret = np.zeros((2, L))
            ret[0, 4], ret[1, [2, 5]] = 30.0, 10.0                # env 1: a tie between actions 2 and 5 -> the smaller CODE: action 5
            code = np.tile(np.arange(L, dtype=np.uint64), (2, 1)) + np.uint64(L) * np.array([[5, 4, 3, 2, 1, 0]] * 2, np.uint64)
            code[1, 2], code[1, 5] = 2 + L * 4, 5 + L * 1
            return dict(ret=ret, score=ret.astype(np.int64), lives=np.ones((2, L), np.int64), frames_run=np.full((2, L), frames),
                        life_lost_at=np.full((2, L), -1, np.int64), code=code, plan=np.zeros((2, L, depth), np.int64))

    for cls, skip in ((vec_env.ToyboxVecEnv, 1), (vec_env.ToyboxPreprocVecEnv, 4)):
        v = object.__new__(cls)
        v.num_envs, v._in_flight, v._pending, v.engine, v._lut, v._action_set, v._skip = 2, None, None, FakeEngine(), lut, list(lut), 4
        waited = []
        monkeypatch.setattr(cls, "step_wait", lambda self: waited.append(1) or setattr(self, "_in_flight", None))
        out = v.evolve_search(5, 2, 8, 3, elite=2, mutation=99, plan_seed=6, init_plan=[3, 5], objective="survival", rest=4, seed=8, t=2)
        frames, depth, population, generations, kw = v.engine.call
        assert (frames, depth, population, generations, kw["hold"], kw["objective"], kw["rest"], kw["seed"], kw["t"]) == (5 * skip, 2, 8, 3, skip, "survival", 11, 8, 2)
        assert (kw["elite"], kw["mutation"], kw["plan_seed"], kw["init"]) == (2, 99, 6, 3 + L * 5)
        assert out["plan"][0].tolist() == [[0, 5], [1, 4], [2, 3], [3, 2], [4, 1], [5, 0]]      # action INDICES
        out = v.evolve_search(5, 2, 4, 1, init_plan=[[0, 1], [2, 3]])
        assert v.engine.call[4]["init"].tolist() == [0 + L * 1, 2 + L * 3] and v.engine.call[4]["elite"] is None and v.engine.call[4]["mutation"] is None
        assert out["best_action"].tolist() == [4, 5] and out["best_plan"].tolist() == [[4, 1], [5, 1]]
        assert not waited
        v._in_flight = object()
        v.evolve_search(1, 1, 1, 0)
        assert waited == [1]
        with pytest.raises(AssertionError):
            v.evolve_search(1, 1, 1, 0, rest=6)
        for bad in ([1, 2, 3], [[0, 1]] * 3, [0, 6]):
            with pytest.raises((ValueError, AssertionError)):
                v.evolve_search(5, 2, 4, 1, init_plan=bad)


def test_engine_defaults_and_the_batch_intervention_window():
    """Engine.lookahead_evolve's default elite and mutation, and BatchIntervention.lookahead_evolve: per-env rows always, the envs
    outside the window asking for one individual and no generation"""
    from toybox_amd.interventions import BatchIntervention
    seen = []

    class Probe(Engine):
        def __init__(self):
            self.game, self.n_envs, self.legal_actions = "breakout", 6, list(LEGAL["breakout"])

        def reduce(self, query, args):
            seen.append((query, args))
            return np.zeros((6, 24))

    e = Probe()
    out = e.lookahead_evolve(32, 9, 16, 2)
    (query, args), = seen
    assert query == _abi.QUERY_LOOKAHEAD_EVOLVE and args[9:] == [16.0, 2.0, 4.0, 0.0, 32.0, -1.0] and out["plan"].shape == (6, 4, 9)
    e.lookahead_evolve(32, 1, 3, 0)
    assert seen[-1][1][9:] == [3.0, 0.0, 1.0, 0.0, 256.0, -1.0]
    bi = object.__new__(BatchIntervention)
    bi.engine, bi.first, bi.count, bi._flush = e, 2, 3, lambda: None
    part = bi.lookahead_evolve(32, 5, 8, 2, init=np.array([5, -1, 9]), plan_seed=4)
    rows = seen[-1][1]
    assert rows.shape == (6, 15) and rows[:, 9].tolist() == [1, 1, 8, 8, 8, 1] and rows[:, 10].tolist() == [0, 0, 2, 2, 2, 0]
    assert rows[:, 11].tolist() == [1, 1, 2, 2, 2, 1] and rows[:, 14].tolist() == [-1, -1, 5, -1, 9, -1] and rows[:, 12].tolist() == [4] * 6
    assert part["ret"].shape == (3, 4)
