"""Plans and the search (TBX_QUERY_LOOKAHEAD_PLAN / _SEARCH), the part that needs no GPU: the constants, plan codes, the argument
shaping, the adapters' mapping, and the yardstick of tests/test_gpu_search.py under test itself over the CPU checker alone
(tests/search_replay.py): play_plan at depth 0 and 1 is the lookahead's own replay, a plan split in time composes, a depth-1 search
is the all-actions lookahead, and the GPU module's cases cover what they must."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from fork_replay import sim_rngs
from lookahead_replay import FIELDS, assert_fields_equal, batch, clone, expected, play, schedule_columns
from search_replay import (DRAWN_CASE, SEARCH_CASES, SEARCH_FIELDS, case_search, expected_plan, expected_search, group_stats, pick, plan_columns,
                           play_all_codes, play_plan)
from support import LEGAL
from toybox_amd import Engine, ToyboxAmdError, _abi
from toybox_amd.engine import plan_actions, plan_args, plan_code, search_args

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
HEADER = open(os.path.join(ROOT, "include", "toybox_amd.h")).read()
MAX_DEPTH = {"breakout": 16, "space_invaders": 12, "amidar": 12, "gridworld": 13}
SEARCH_DEPTH = {"breakout": 6, "space_invaders": 4, "amidar": 4, "gridworld": 5}


def test_header_and_python_agree_on_the_constants():
    want = {"TBX_QUERY_LOOKAHEAD_PLAN": (_abi.QUERY_LOOKAHEAD_PLAN, 152), "TBX_QUERY_LOOKAHEAD_SEARCH": (_abi.QUERY_LOOKAHEAD_SEARCH, 153),
            "TBX_LOOKAHEAD_MAX_PLANS": (_abi.LOOKAHEAD_MAX_PLANS, 4096), "TBX_OPT_SEARCH_CHUNKS": (_abi.OPT_SEARCH_CHUNKS, 105)}
    for name, (py, value) in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, HEADER)
        assert m and int(m.group(1)) == py == value, name
    assert re.search(r"#define\s+TBX_QUERY_LOOKAHEAD_PLAN\s+152\s*/\*.*->\s*5\s*\*/", HEADER), "the width stands on the #define line"
    assert re.search(r"#define\s+TBX_QUERY_LOOKAHEAD_SEARCH\s+153\s*/\*.*->\s*6\s*\*\s*n_legal", HEADER)
    m = re.search(r"#define\s+TBX_PLAN_MAX_DEPTH\(game\)\s+(.*)", HEADER)
    assert m and [int(x) for x in re.findall(r"\?\s*(\d+)|:\s*(\d+)\)", m.group(1))[0] if x] == [16]
    assert re.search(r"TBX_GAME_BREAKOUT \? 16 : \(game\) == TBX_GAME_GRIDWORLD \? 13 : 12", m.group(1))
    for game in GAMES:
        L = len(LEGAL[game])
        assert tuple(LEGAL[game]) == _abi.LEGAL_ACTIONS[game]
        assert _abi.PLAN_MAX_DEPTH[game] == MAX_DEPTH[game] and L ** MAX_DEPTH[game] <= 2 ** 32 < L ** (MAX_DEPTH[game] + 1)
        assert L ** SEARCH_DEPTH[game] <= _abi.LOOKAHEAD_MAX_PLANS < L ** (SEARCH_DEPTH[game] + 1)


def test_the_abi_has_no_new_symbols_and_keeps_its_version():
    assert len(re.findall(r"\btbx_\w*lookahead\w*\s*\(", HEADER)) == 0, "plans and the search go through tbx_reduce"
    assert re.search(r"#define\s+TBX_ABI_VERSION\s+1\b", HEADER)


def test_the_checker_has_neither_query(oracle_lib):
    """the expected values cannot come from the checker's own: it answers "unknown query" to both ids"""
    with Engine("breakout", 4, lib=oracle_lib) as e:
        for call in (lambda: e.lookahead_plan(8, [1, 3]), lambda: e.lookahead_search(8, 2), lambda: e.reduce(152, [8]), lambda: e.reduce(153, [8])):
            with pytest.raises(ToyboxAmdError) as ei:
                call()
            assert ei.value.code == _abi.E_INVALID


# ---------------------------------------------------------------- plan codes

@pytest.mark.parametrize("game", GAMES)
def test_plan_codes_round_trip(game):
    legal, L = np.asarray(LEGAL[game]), len(LEGAL[game])
    assert plan_code(game, []) == 0 and plan_actions(game, 0, 0).shape == (0,)
    assert int(plan_code(game, [legal[2], legal[0], legal[L - 1]])) == 2 + 0 * L + (L - 1) * L * L      # digit 0 is the first action
    assert plan_actions(game, 2 + (L - 1) * L * L, 3).tolist() == [legal[2], legal[0], legal[L - 1]]
    rng = np.random.default_rng(3)
    for depth in (1, 5, MAX_DEPTH[game]):
        a = legal[rng.integers(0, L, (7, 3, depth))]
        a[0, 0] = legal[L - 1]                                    # the largest code of the depth: L ** depth - 1
        code = plan_code(game, a)
        assert code.shape == (7, 3) and code.dtype == np.uint64 and int(code[0, 0]) == L ** depth - 1
        assert np.array_equal(plan_actions(game, code, depth), a)
        assert np.array_equal(plan_code(game_id(game), a), code)
    for bad in ([2 if game == "breakout" else 17], np.zeros(MAX_DEPTH[game] + 1, int)):
        with pytest.raises(ValueError):
            plan_code(game, bad)
    for code, depth in ((L ** 2, 2), (-1, 2), (0, MAX_DEPTH[game] + 1), (1, 0)):
        with pytest.raises(ValueError):
            plan_actions(game, code, depth)


def game_id(game):
    return _abi.GAME_IDS[game]


# ---------------------------------------------------------------- the argument shaping

def test_args_defaults_and_scalars():
    assert plan_args("breakout", 8, 16) == ([16.0, 1.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0], False)
    assert search_args("breakout", 8, 16) == ([16.0, 1.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0], False)
    seed = (0xDEADBEEF << 32) | 0x12345678
    args, per_env = plan_args("space_invaders", 8, 300, hold=4, depth=3, code=215, rest=11, seed=seed, t=77, env_offset=4096)
    assert per_env is False and args == [300.0, 4.0, 3.0, 215.0, 11.0, float(0x12345678), float(0xDEADBEEF), 77.0, 4096.0]
    args, per_env = search_args("amidar", 8, 64, hold=4, depth=4, objective="survival", rest=0, seed=5)
    assert per_env is False and args == [64.0, 4.0, 4.0, 1.0, 0.0, 5.0, 0.0, 0.0, 0.0]
    assert plan_args("breakout", 2, 8, depth=16, code=4 ** 16 - 1)[0][3] == float(4 ** 16 - 1)


def test_args_per_env_rows():
    n = 6
    code = np.array([0, 1, 63, 64, -1, 5])
    args, per_env = plan_args("breakout", n, np.array([1, 2, 4, 299, 0, 1024]), hold=7, depth=3, code=code, seed=np.arange(n, dtype=np.uint64) << np.uint64(33), t=5)
    assert per_env is True and args.shape == (n, 9) and args.dtype == np.float64
    assert args[:, 0].tolist() == [1, 2, 4, 299, 0, 1024] and args[:, 1].tolist() == [7] * n and args[:, 2].tolist() == [3] * n
    assert args[:, 3].tolist() == code.tolist() and args[:, 4].tolist() == [-1] * n
    assert args[:, 5].tolist() == [0] * n and args[:, 6].tolist() == [2.0 * i for i in range(n)] and args[:, 7].tolist() == [5] * n
    # per-env rows are checked on the device (a bad row answers zeros), not here
    args, per_env = search_args("gridworld", n, 8, depth=np.array([0, 1, 5, 6, 99, -3]), objective=np.array([0, 1, 2, 0, 0, 0]), rest=np.full(n, 17))
    assert per_env is True and args[:, 2].tolist() == [0, 1, 5, 6, 99, -3] and args[:, 3].tolist() == [0, 1, 2, 0, 0, 0] and args[:, 4].tolist() == [17] * n


@pytest.mark.parametrize("bad", [dict(frames=0), dict(frames=1025), dict(frames=8, hold=0), dict(frames=8, seed=2 ** 64), dict(frames=8, t=2 ** 32),
                                 dict(frames=8, depth=-1), dict(frames=8, depth=17), dict(frames=8, depth=2, code=16), dict(frames=8, depth=0, code=1),
                                 dict(frames=8, depth=2, code=-1), dict(frames=8, rest=2), dict(frames=8, depth=np.ones(5)), dict(frames=8, depth=2, code=np.zeros((6, 1))),
                                 dict(frames=np.ones(5))])
def test_plan_args_range_and_shape_errors(bad):
    with pytest.raises(ValueError):
        plan_args("breakout", 6, **bad)


@pytest.mark.parametrize("bad", [dict(frames=0), dict(frames=1025), dict(frames=8, hold=0), dict(frames=8, depth=0), dict(frames=8, depth=7), dict(frames=8, objective=2),
                                 dict(frames=8, objective="score"), dict(frames=8, rest=2), dict(frames=8, depth=np.ones(5)), dict(frames=8, objective=np.zeros(7)),
                                 dict(frames=8, env_offset=-3)])
def test_search_args_range_and_shape_errors(bad):
    with pytest.raises(ValueError):
        search_args("breakout", 6, **bad)
    assert search_args("breakout", 6, 8, depth=6)[0][2] == 6.0
    for game in ("space_invaders", "amidar"):
        with pytest.raises(ValueError):
            search_args(game, 6, 8, depth=5)
    with pytest.raises(ValueError):
        search_args("gridworld", 6, 8, depth=6)


def test_the_adapters_map_action_indices_and_steps(monkeypatch):
    """ToyboxVecEnv.search / lookahead_plan: frames = steps, hold = 1; ToyboxPreprocVecEnv: frames = steps x skip, hold = skip;
    action indices become ALE ids going in, plans come back as action indices; best_action / best_plan pick the winner of an env's
    rows under the same objective, ties to the smaller code; a pending step ends first"""
    from toybox_amd.envs import vec_env
    lut = np.asarray(LEGAL["space_invaders"], np.int32)
    L = len(lut)

    class FakeEngine:
        legal_actions = list(lut)

        def lookahead_plan(self, frames, plan, **kw):
            self.call = ("plan", frames, plan, kw)

        def lookahead_search(self, frames, depth, **kw):
            self.call = ("search", frames, depth, kw)
            ret = np.zeros((3, L))
            lives = np.ones((3, L), np.int64)
            lost = np.full((3, L), -1, np.int64)
            ret[0, 4] = 30.0                                      # env 0: return picks action 4, survival action 2 (4 loses a life)
            lives[0, 4], lost[0, 4] = 0, 7
            lost[0, [0, 1, 3, 5]] = 3
            ret[1, [2, 5]] = 10.0                                 # env 1: a tie between actions 2 and 5 -> the smaller CODE wins: action 5
            code = np.tile(np.arange(L, dtype=np.uint64), (3, 1)) + np.uint64(L) * np.array([[5, 4, 3, 2, 1, 0]] * 3, np.uint64)
            code[1, 2], code[1, 5] = 2 + L * 4, 5 + L * 1
            return dict(ret=ret, score=ret.astype(np.int64), lives=lives, frames_run=np.full((3, L), frames), life_lost_at=lost, code=code,
                        plan=np.zeros((3, L, depth), np.int64))

    for cls, skip in ((vec_env.ToyboxVecEnv, 1), (vec_env.ToyboxPreprocVecEnv, 4)):
        v = object.__new__(cls)
        v.num_envs, v._in_flight, v._pending, v.engine, v._lut, v._action_set, v._skip = 3, None, None, FakeEngine(), lut, list(lut), 4
        waited = []
        monkeypatch.setattr(cls, "step_wait", lambda self: waited.append(1) or setattr(self, "_in_flight", None))
        v.lookahead_plan(5, [4, 0, 5], rest=np.array([0, 5, 2]), seed=9, t=3)
        kind, frames, plan, kw = v.engine.call
        assert (kind, frames, kw["hold"], kw["seed"], kw["t"]) == ("plan", 5 * skip, skip, 9, 3)
        assert np.array_equal(plan, [11, 0, 12]) and np.array_equal(kw["rest"], [0, 12, 3])
        v.lookahead_plan(2, np.array([[0, 1], [2, 3], [4, 5]]))
        assert np.array_equal(v.engine.call[2], [[0, 1], [3, 4], [11, 12]]) and v.engine.call[3]["rest"] is None
        out = v.search(5, 2, rest=4, seed=8, t=2)
        kind, frames, depth, kw = v.engine.call
        assert (kind, frames, depth, kw["hold"], kw["objective"], kw["rest"], kw["seed"], kw["t"]) == ("search", 5 * skip, 2, skip, "return", 11, 8, 2)
        assert out["plan"].shape == (3, L, 2) and out["plan"][0].tolist() == [[0, 5], [1, 4], [2, 3], [3, 2], [4, 1], [5, 0]]      # action INDICES
        assert out["best_action"].tolist() == [4, 5, 5] and out["best_plan"].tolist() == [[4, 1], [5, 1], [5, 0]]
        out = v.search(5, 2, objective="survival")
        assert out["best_action"].tolist() == [2, 5, 5] and out["best_plan"][0].tolist() == [2, 3]
        assert not waited
        v._in_flight = object()
        v.search(1, 1)
        v._in_flight = object()
        v.lookahead_plan(1, [0])
        assert waited == [1, 1]
        with pytest.raises(AssertionError):
            v.lookahead_plan(1, [6])
        with pytest.raises(AssertionError):
            v.search(1, 1, rest=6)


# ---------------------------------------------------------------- the yardstick, on the checker alone

N = 24


@pytest.fixture(scope="module")
def batches(oracle_lib):
    out = {}
    for game in GAMES:
        e = batch(oracle_lib, game, N)
        out[game] = (e.get_states(), sim_rngs(e))
        e.close()
    return out


@pytest.mark.parametrize("game", GAMES)
def test_play_plan_at_depth_0_and_1_is_the_lookahead_replay(game, batches, oracle_lib):
    states, rngs = batches[game]
    sched = dict(frames=90, hold=4, rest=LEGAL[game][1], seed=77, t=5, env_offset=1000)
    want = expected(oracle_lib, game, states, rngs, dict(sched, first=sched["rest"]))
    assert_fields_equal(expected_plan(oracle_lib, game, states, rngs, dict(sched, depth=0)), want, "%s depth 0 = first is rest" % game)
    digit = np.resize(np.arange(len(LEGAL[game])), N)
    want = expected(oracle_lib, game, states, rngs, dict(sched, rest=-1, first=np.asarray(LEGAL[game])[digit]))
    assert_fields_equal(expected_plan(oracle_lib, game, states, rngs, dict(sched, rest=-1, depth=1, code=digit)), want, "%s depth 1 = first is legal[code]" % game)


@pytest.mark.parametrize("game", GAMES)
def test_a_plan_split_in_time_composes(game, batches, oracle_lib):
    """a depth-5 plan = its first k periods, then from the stepped clone the other periods with the counter moved on"""
    states, rngs = batches[game]
    L, hold, k, depth, tail = len(LEGAL[game]), 6, 2, 5, 20
    rng = np.random.default_rng(5)
    digits = rng.integers(0, L, (N, depth))
    code = (digits * L ** np.arange(depth)).sum(axis=1)
    sched = dict(hold=hold, rest=-1, seed=9, t=40, env_offset=3)
    whole = expected_plan(oracle_lib, game, states, rngs, dict(sched, frames=depth * hold + tail, depth=depth, code=code))
    e = clone(oracle_lib, game, states, rngs)
    a = play_plan(e, game, plan_columns(N, frames=k * hold, depth=k, code=code % L ** k, **sched))
    b = play_plan(e, game, plan_columns(N, frames=(depth - k) * hold + tail, depth=depth - k, code=code // L ** k, **dict(sched, t=40 + k)))
    e.close()
    going = a["lives"] > 0
    assert going.any()
    assert np.array_equal(whole["ret"][going], (a["ret"] + b["ret"])[going])
    for f in ("score", "lives"):
        assert np.array_equal(whole[f][going], b[f][going])
    assert np.array_equal(whole["frames_run"][going], (k * hold + b["frames_run"])[going])
    lost = np.where(a["life_lost_at"] >= 0, a["life_lost_at"], np.where(b["life_lost_at"] >= 0, k * hold + b["life_lost_at"], -1))
    assert np.array_equal(whole["life_lost_at"][going], lost[going])
    for f in FIELDS:
        assert np.array_equal(whole[f][~going], a[f][~going]), f


@pytest.mark.parametrize("game", GAMES)
def test_a_search_of_depth_1_is_the_all_actions_lookahead(game, batches, oracle_lib):
    states, rngs = batches[game]
    sched = dict(frames=80, hold=4, rest=-1, seed=3, t=9)
    want = expected(oracle_lib, game, states, rngs, sched, all_actions=True)
    for objective in (0, 1):
        got = expected_search(oracle_lib, game, states, rngs, dict(sched, depth=1, objective=objective))
        assert_fields_equal(got, want, "%s depth-1 search" % game)
        assert np.array_equal(got["code"], np.tile(np.arange(len(LEGAL[game])), (N, 1)))


def test_refused_search_rows_are_zero_and_leave_the_others(batches, oracle_lib):
    game = "breakout"
    states, rngs = batches[game]
    depth, objective, frames = np.full(N, 2), np.zeros(N, np.int64), np.full(N, 24)
    depth[3], depth[4], objective[6], frames[8] = 0, 7, 2, 1025
    got = expected_search(oracle_lib, game, states, rngs, dict(frames=frames, hold=4, depth=depth, objective=objective, rest=0))
    plain = expected_search(oracle_lib, game, states, rngs, dict(frames=24, hold=4, depth=2, rest=0))
    bad = np.isin(np.arange(N), [3, 4, 6, 8])
    for k in SEARCH_FIELDS:
        assert (got[k][bad] == 0).all() and np.array_equal(got[k][~bad], plain[k][~bad]), k


# ---------------------------------------------------------------- the GPU module's cases cover what they must

@functools.lru_cache(maxsize=None)
def case_leaves(oracle_lib, game, case):
    n, _, _, _, batch_frames = case
    e = batch(oracle_lib, game, n, frames=batch_frames)
    states, rngs = e.get_states(), sim_rngs(e)
    e.close()
    return play_all_codes(oracle_lib, game, states, rngs, case_search(game, case))


@pytest.mark.parametrize("game", GAMES)
def test_the_cases_cover_what_they_must(game, oracle_lib):
    """over a game's search cases (tests/search_replay.py, SEARCH_CASES): a group whose winner is not its smallest code, a group won
    on the tie-break, a positive ret and -- not GridWorld, which has no lives to lose -- a leaf that ended the game and a group where
    the two objectives choose different plans"""
    total = {}
    for case in SEARCH_CASES[game]:
        st = group_stats(game, *case_leaves(oracle_lib, game, case))
        print(game, case, st)
        for k, v in st.items():
            total[k] = total.get(k, 0) + int(v)
    need = ["winner_not_first", "ties", "scored"] + ([] if game == "gridworld" else ["disagree", "ended_envs"])
    missing = [k for k in need if not total[k]]
    assert not missing, "%s: the search cases together never show: %s" % (game, ", ".join(missing))
