"""Tree search (TBX_QUERY_LOOKAHEAD_TREE), the part that needs no GPU: the constants, the argument shaping, and the yardstick of
tests/test_gpu_tree.py under test itself over the CPU checker alone (tests/tree_replay.py): the consequences the header states
against sample_replay / search_replay, refused rows, and that the GPU module's cases cover what they must (the counts and replay
times of each case are printed)."""
import functools
import os
import re
import time

import numpy as np
import pytest

from conftest import ROOT
from fork_replay import sim_rngs
from lookahead_replay import batch
from sample_replay import assert_samples_equal, expected_samples
from search_replay import expected_plan
from support import LEGAL
from toybox_amd import Engine, ToyboxAmdError, _abi
from toybox_amd.engine import SAMPLE_FIELDS, TREE_FIELDS, beam_args, tree_args
from tree_replay import (BATCH_FRAMES, CASES, ENVS, MAX_EXPLORE, MAX_SIMULATIONS, OPT_LAUNCH_SIMULATIONS, OPT_RANGES, QUERY, case_tree, expected_tree,
                         missing_coverage, played_codes_differ, splitmix64, tree_stats)
import tree_replay

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
HEADER = open(os.path.join(ROOT, "include", "toybox_amd.h")).read()


def test_header_python_and_replay_agree_on_the_constants():
    want = {"TBX_QUERY_LOOKAHEAD_TREE": (_abi.QUERY_LOOKAHEAD_TREE, QUERY, 160), "TBX_TREE_MAX_SIMULATIONS": (_abi.TREE_MAX_SIMULATIONS, MAX_SIMULATIONS, 1024),
            "TBX_TREE_MAX_EXPLORE": (_abi.TREE_MAX_EXPLORE, MAX_EXPLORE, 1048576), "TBX_OPT_TREE_RANGES": (_abi.OPT_TREE_RANGES, OPT_RANGES, 115),
            "TBX_OPT_TREE_LAUNCH_SIMULATIONS": (_abi.OPT_TREE_LAUNCH_SIMULATIONS, OPT_LAUNCH_SIMULATIONS, 116)}
    for name, (py, replay, value) in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, HEADER)
        assert m and int(m.group(1)) == py == replay == value, name
    assert re.search(r"#define\s+TBX_QUERY_LOOKAHEAD_TREE\s+160\s*/\*.*env_offset,\s*simulations, explore, salt\}\s*->\s*12\s*\*\s*n_legal", HEADER), \
        "columns and width stand on the #define line"
    assert re.search(r"#define\s+TBX_ABI_VERSION\s+1\b", HEADER)
    text = HEADER[HEADER.index("Tree search: open-loop"):HEADER.index("#define TBX_TREE_MAX_SIMULATIONS")]
    for consequence in ("(i) ", "(ii) ", "(iii) ", "(iv) ", "(v) "):
        assert consequence in text, "the header states consequence %s" % consequence
    assert TREE_FIELDS == tree_replay.TREE_FIELDS and TREE_FIELDS[:8] == SAMPLE_FIELDS and len(TREE_FIELDS) == 12
    assert _abi.EDIT_MAX_ARGS == 16 and sorted(__import__("toybox_amd.engine").engine.ACT_PLANNERS.values()) == [153, 155, 156, 157, 158]


def test_the_checker_has_no_tree(oracle_lib):
    """the expected values cannot come from the checker's own: it answers "unknown query\""""
    with Engine("breakout", 4, lib=oracle_lib) as e:
        for call in (lambda: e.lookahead_tree(8, 2, 2), lambda: e.reduce(160, [8])):
            with pytest.raises(ToyboxAmdError) as ei:
                call()
            assert ei.value.code == _abi.E_INVALID


# ---------------------------------------------------------------- the argument shaping

def test_tree_args_columns():
    assert tree_args("breakout", 8, 16, 1) == ([16.0, 1.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0], False)
    seed = (0xDEADBEEF << 32) | 0x12345678
    args, per_env = tree_args("space_invaders", 8, 300, 12, 1024, 1048576, 2 ** 32 - 1024, hold=4, objective="survival", rest=11, seed=seed, t=77, env_offset=4096)
    assert per_env is False and args == [300.0, 4.0, 12.0, 1.0, 11.0, float(0x12345678), float(0xDEADBEEF), 77.0, 4096.0, 1024.0, 1048576.0, float(2 ** 32 - 1024)]
    assert len(args) == 12 < _abi.EDIT_MAX_ARGS
    # columns 0 .. 8 are the beam's
    assert tree_args("amidar", 8, 64, 4, 3, hold=4, objective=1, rest=0, seed=5)[0][:9] == beam_args("amidar", 8, 64, 4, 3, hold=4, objective=1, rest=0, seed=5)[0][:9]
    for game in GAMES:
        assert tree_args(game, 2, 8, _abi.PLAN_MAX_DEPTH[game], 2)[0][2] == float(_abi.PLAN_MAX_DEPTH[game])
    n = 6
    args, per_env = tree_args("gridworld", n, 8, np.array([0, 1, 5, 13, 99, -3]), np.array([1, 1024, 0, 1025, 2, 3]), explore=np.array([0, 1, -1, 2 ** 20 + 1, 5, 6]),
                              salt=np.array([0, 2 ** 32 - 1, 7, -2, 2 ** 32, 1]), objective=np.array([0, 1, 2, 0, 0, 0]), rest=np.full(n, 17))
    assert per_env is True and args.shape == (n, 12) and args.dtype == np.float64      # per-env rows are checked on the device, not here
    assert args[:, 2].tolist() == [0, 1, 5, 13, 99, -3] and args[:, 9].tolist() == [1, 1024, 0, 1025, 2, 3] and args[:, 10].tolist() == [0, 1, -1, 2 ** 20 + 1, 5, 6]
    assert args[:, 11].tolist() == [0, 2 ** 32 - 1, 7, -2, 2 ** 32, 1] and args[:, 3].tolist() == [0, 1, 2, 0, 0, 0]
    args, per_env = tree_args("breakout", n, np.arange(1, n + 1), 3, 4, 2, 9)
    assert per_env is True and args[:, 9].tolist() == [4] * n and args[:, 10].tolist() == [2] * n and args[:, 11].tolist() == [9] * n


@pytest.mark.parametrize("bad", [dict(frames=0), dict(frames=1025), dict(hold=0), dict(depth=0), dict(depth=17), dict(simulations=0), dict(simulations=1025),
                                 dict(explore=-1), dict(explore=2 ** 20 + 1), dict(salt=-1), dict(salt=2 ** 32), dict(salt=2 ** 32 - 3, simulations=4),
                                 dict(objective=2), dict(objective="score"), dict(rest=2), dict(depth=np.ones(5)), dict(simulations=np.ones(5)),
                                 dict(explore=np.ones((6, 1))), dict(salt=np.zeros(7)), dict(objective=np.zeros(7)), dict(env_offset=-3), dict(seed=2 ** 64),
                                 dict(t=2 ** 32)])
def test_tree_args_range_and_shape_errors(bad):
    kw = dict(frames=8, depth=2, simulations=4, explore=2)
    kw.update(bad)
    with pytest.raises(ValueError):
        tree_args("breakout", 6, **kw)
    tree_args("breakout", 6, 8, 2, 4, salt=2 ** 32 - 4)          # the largest salt of four simulations


def test_the_replays_words_are_the_headers():
    from toybox_amd.engine import sample_seed
    for seed, m in ((0, 0), (77, 5), (2 ** 64 - 1, 3), ((0xABCDE << 32) | 0x1234567, 1023)):
        assert splitmix64((seed + m) & (2 ** 64 - 1)) == sample_seed(seed, m)


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


@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("game", GAMES)
def test_the_consequences_hold_for_the_replay(game, objective, batches, oracle_lib):
    states, rngs = batches[game]
    L, hold = len(LEGAL[game]), tree_replay.HOLD[game]
    sched = dict(frames=hold * 8, hold=hold, rest=-1, seed=(5 << 33) | 3, t=9, env_offset=11)
    # (i) depth 1: the row of the sampled lookahead, and [8 .. 10] = a, 1, M
    M = 5
    rows, log, _ = expected_tree(oracle_lib, game, states, rngs, dict(sched, depth=1, objective=objective, simulations=M, explore=7, salt=1000))
    assert_samples_equal(rows, expected_samples(oracle_lib, game, states, rngs, dict(sched, samples=M, salt=1000)), "%s (i)" % game)
    assert np.array_equal(rows["code"], np.tile(np.arange(L), (N, 1))) and (rows["pv_depth"] == 1).all() and (rows["pv_visits"] == M).all()
    value = rows["ret_sum"] if objective == 0 else rows["safe_frames_sum"]
    assert np.array_equal(rows["pv_value"], value), "the root's v_sum is the sum its objective names"
    # (ii) depth >= 2 and M <= L: simulation m plays code a + m L at depth 2 on future m
    rows, log, _ = expected_tree(oracle_lib, game, states, rngs, dict(sched, depth=3, objective=objective, simulations=L, explore=7))
    for m in range(L):
        assert np.array_equal(log[m]["code"], np.tile(np.arange(L) + m * L, (N, 1))) and (log[m]["depth"] == 2).all() and log[m]["absent"].all()
        for a in range(L):
            plan = expected_plan(oracle_lib, game, states, rngs, dict(sched, depth=2, code=a + m * L, seed=splitmix64(sched["seed"] + m)))
            v = plan["ret"] if objective == 0 else np.where(plan["life_lost_at"] < 0, plan["frames_run"], plan["life_lost_at"])
            assert np.array_equal(log[m]["value"][:, a], np.asarray(v, np.int64)), (game, m, a)
    # (iii) depth >= 2: the n of the root's children sum to M, and pv_depth >= 2
    M = 3 * L + 2
    rows, log, trees = expected_tree(oracle_lib, game, states, rngs, dict(sched, depth=3, objective=objective, simulations=M, explore=7, salt=5))
    for i in range(N):
        for a in range(L):
            nodes = trees[i][a]
            assert sum(nodes[c].n for c in nodes[0].child if c is not None) == M == nodes[0].n == rows["samples"][i, a]
            assert len(nodes) <= M + 1 and all(c is None or 0 < c < len(nodes) for nd in nodes for c in nd.child)
    assert (rows["pv_depth"] >= 2).all() and (rows["pv_depth"] <= 3).all() and (rows["code"] % L == np.arange(L)).all()
    assert (rows["ret_min"] <= rows["ret_max"]).all() and (rows["pv_visits"] >= 1).all() and (rows["pv_visits"] < M).all()
    # (v) two equal replays give equal rows
    again, _, _ = expected_tree(oracle_lib, game, states, rngs, dict(sched, depth=3, objective=objective, simulations=M, explore=7, salt=5))
    assert all(np.array_equal(again[k], rows[k]) for k in TREE_FIELDS)


def test_refused_tree_rows_are_zero_and_leave_the_others(batches, oracle_lib):
    game = "breakout"
    states, rngs = batches[game]
    cols = dict(depth=np.full(N, 3), simulations=np.full(N, 6), explore=np.full(N, 3), salt=np.full(N, 0), objective=np.full(N, 0), frames=np.full(N, 24))
    cols["depth"][0], cols["simulations"][1], cols["simulations"][2], cols["explore"][3], cols["salt"][4], cols["objective"][5] = 17, 0, 1025, 2 ** 20 + 1, 2 ** 32 - 5, 2
    got, _, _ = expected_tree(oracle_lib, game, states, rngs, dict(cols, hold=4, rest=0))
    plain, _, _ = expected_tree(oracle_lib, game, states, rngs, dict(frames=24, hold=4, depth=3, simulations=6, explore=3, rest=0))
    bad = np.isin(np.arange(N), [0, 1, 2, 3, 4, 5])
    for k in TREE_FIELDS:
        assert (got[k][bad] == 0).all() and np.array_equal(got[k][~bad], plain[k][~bad]), k
    assert (plain["samples"] == 6).all()


# ---------------------------------------------------------------- the GPU module's cases cover what they must

@functools.lru_cache(maxsize=None)
def case_replay(oracle_lib, game, name):
    e = batch(oracle_lib, game, ENVS, frames=BATCH_FRAMES[game])
    states, rngs = e.get_states(), sim_rngs(e)
    e.close()
    tree = case_tree(game, name)
    t0 = time.perf_counter()
    rows, log, trees = expected_tree(oracle_lib, game, states, rngs, tree)
    counts = tree_stats(game, rows, log, trees, tree["depth"])
    print(game, name, {k: tree[k] for k in ("frames", "hold", "depth", "simulations", "explore")}, "replay %.1f s" % (time.perf_counter() - t0), counts)
    return rows, log, counts


@pytest.mark.parametrize("game", GAMES)
def test_the_cases_cover_what_they_must(game, oracle_lib):
    """over a game's tree cases (tests/tree_replay.py, case_tree), on the replay alone: the eight coverage conditions"""
    totals = {}
    for name in CASES:
        for k, v in case_replay(oracle_lib, game, name)[2].items():
            if k != "pv_full":
                totals[k] = totals.get(k, 0) + int(v)
    totals["pv_full"] = case_replay(oracle_lib, game, "deepest")[2]["pv_full"]
    totals["explore_changes"] = played_codes_differ(case_replay(oracle_lib, game, "tree")[1], case_replay(oracle_lib, game, "tree_explore")[1])
    print(game, totals)
    missing = missing_coverage(game, totals)
    assert not missing, "%s: the tree cases together never show: %s" % (game, ", ".join(missing))


@pytest.mark.parametrize("game", GAMES)
def test_explore_changes_a_played_code(game, oracle_lib):
    """the `tree` case under explore 0 and under tree_replay.EXPLORE: the same batch, the same futures, another code played"""
    assert case_tree(game, "tree")["explore"] == 0 < case_tree(game, "tree_explore")["explore"]
    assert played_codes_differ(case_replay(oracle_lib, game, "tree")[1], case_replay(oracle_lib, game, "tree_explore")[1]) > 0


# ---------------------------------------------------------------- the adapters

def test_the_adapters_map_action_indices_and_steps(monkeypatch):
    """ToyboxVecEnv.tree_search: frames = steps, hold = 1; ToyboxPreprocVecEnv: frames = steps x skip, hold = skip; `rest` an action
    index going in; best_action by sample_best_action on the root sums, best_plan the winner's digits with -1 beyond pv_depth; a
    pending step ends first"""
    from toybox_amd.envs import vec_env
    lut = np.asarray(LEGAL["space_invaders"], np.int32)
    L = len(lut)

    class FakeEngine:
        legal_actions = list(lut)

        def lookahead_tree(self, frames, depth, simulations, **kw):
            self.call = (frames, depth, simulations, kw)
            out = {k: np.zeros((2, L), np.int64) for k in TREE_FIELDS}
            out["samples"][:] = simulations
            out["ret_sum"][0, 4], out["ret_sum"][1, [2, 5]] = 30, 10                # env 1: a tie between actions 2 and 5 -> the smaller index
            out["code"] = (np.tile(np.arange(L), (2, 1)) + L * np.array([[5, 4, 3, 2, 1, 0]] * 2) + L * L * 3).astype(np.uint64)
            out["pv_depth"][:] = 3
            out["pv_depth"][1, 2] = 2
            return out

    for cls, skip in ((vec_env.ToyboxVecEnv, 1), (vec_env.ToyboxPreprocVecEnv, 4)):
        v = object.__new__(cls)
        v.num_envs, v._in_flight, v._pending, v.engine, v._lut, v._action_set, v._skip = 2, None, None, FakeEngine(), lut, list(lut), 4
        waited = []
        monkeypatch.setattr(cls, "step_wait", lambda self: waited.append(1) or setattr(self, "_in_flight", None))
        out = v.tree_search(5, 4, 9, explore=6, objective="survival", rest=4, seed=8, t=2, salt=3)
        frames, depth, simulations, kw = v.engine.call
        assert (frames, depth, simulations, kw["hold"], kw["objective"], kw["rest"], kw["seed"], kw["t"], kw["explore"], kw["salt"]) == (5 * skip, 4, 9, skip, "survival", 11, 8, 2, 6, 3)
        out = v.tree_search(5, 4, 9)
        assert v.engine.call[3]["rest"] is None and v.engine.call[3]["explore"] == 0
        assert out["best_action"].tolist() == [4, 2] and out["best_plan"].tolist() == [[4, 1, 3, -1], [2, 3, -1, -1]]
        assert not waited
        v._in_flight = object()
        v.tree_search(1, 1, 1)
        assert waited == [1]
        with pytest.raises(AssertionError):
            v.tree_search(1, 1, 1, rest=6)
        with pytest.raises(ValueError):
            v.tree_search(1, 1, 1, objective="score")


def test_engine_rows_become_the_dict():
    class Probe(Engine):
        def __init__(self):
            self.game, self.n_envs, self.legal_actions = "breakout", 3, list(LEGAL["breakout"])

        def reduce(self, query, args):
            self.seen = (query, args)
            return np.arange(3 * 48, dtype=np.float64).reshape(3, 48)

    e = Probe()
    out = e.lookahead_tree(32, 9, 16, explore=5, salt=2, hold=4)
    assert e.seen == (_abi.QUERY_LOOKAHEAD_TREE, [32.0, 4.0, 9.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 16.0, 5.0, 2.0])
    assert tuple(out) == TREE_FIELDS and all(v.shape == (3, 4) for v in out.values()) and out["code"].dtype == np.uint64 and out["samples"].dtype == np.int64
    assert out["samples"][1, 2] == 48 + 24 and out["pv_value"][2, 3] == 143
