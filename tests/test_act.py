"""Closed-loop planning (TBX_QUERY_LOOKAHEAD_ACT), the part that needs no GPU: the constants, the argument shaping, the product's
plan_pick and plan_shift against the replay's own pick and carry (tests/act_replay.py), and the replay's closed loop under test
itself over the CPU checker alone."""
import os
import re

import numpy as np
import pytest

import act_replay
from act_replay import BATCH_FRAMES, EVOLVE, MOST_COLUMNS, PLANNERS, expected_rollout, pick, shift
from conftest import ROOT
from lookahead_replay import FIELDS, batch, clone_of
from search_samples_replay import SAMPLE_FIELDS
from support import LEGAL
from toybox_amd import Engine, ToyboxAmdError, _abi
from toybox_amd.engine import ACT_PLANNERS, act_args, beam_args, beam_samples_args, evolve_args, plan_digits, plan_pick, plan_shift, search_args, search_samples_args

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
HEADER = open(os.path.join(ROOT, "include", "toybox_amd.h")).read()


def test_header_and_python_agree_on_the_constants():
    want = {"TBX_QUERY_LOOKAHEAD_ACT": (_abi.QUERY_LOOKAHEAD_ACT, act_replay.ACT, 159), "TBX_BUF_PLAN_ACTION": (_abi.BUF_PLAN_ACTION, act_replay.BUF_PLAN_ACTION, 17),
            "TBX_BUF_PLAN_CARRY": (_abi.BUF_PLAN_CARRY, act_replay.BUF_PLAN_CARRY, 18), "TBX_EDIT_MAX_ARGS": (_abi.EDIT_MAX_ARGS, 1 + MOST_COLUMNS[EVOLVE], 16)}
    for name, (py, replay, value) in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, HEADER) or re.search(r"^\s+%s = (\d+),?\s+/\*" % name, HEADER, re.M)     # (the two ids: an enum)
        assert m and int(m.group(1)) == py == replay == value, name
    assert re.search(r"#define\s+TBX_ABI_VERSION\s+1\b", HEADER) and _abi.ABI_VERSION == 1
    assert sorted(ACT_PLANNERS.values()) == sorted(PLANNERS) == [153, 155, 156, 157, 158]
    assert act_replay.PLAN_MAX_DEPTH == _abi.PLAN_MAX_DEPTH
    for consequence in ("(i) ", "(ii) ", "(iii) ", "(iv) "):
        assert consequence in HEADER[HEADER.index("Closed-loop planning"):HEADER.index("#define TBX_QUERY_LOOKAHEAD_ACT")]


def test_no_new_symbol():
    """the query and the two buffers go through what is there: the header declares what the parent commit declared"""
    declared = set(re.findall(r"\b(tbx_[a-z_0-9]+)\s*\(", HEADER))
    assert declared == set(_abi.PROTOTYPES) and not [s for s in declared if "act" in s.split("_") or "plan" in s.split("_") or "carry" in s]


def test_the_checker_has_no_act(oracle_lib):
    """the expected values cannot come from the checker's own"""
    with Engine("breakout", 4, lib=oracle_lib) as e:
        assert oracle_lib.tbx_reduce_width(_abi.GAME_BREAKOUT, 159) == _abi.E_INVALID
        for call in (lambda: e.reduce(159, [153, 8]), lambda: e.lookahead_act("search", frames=8), lambda: e.device_buffer(17), lambda: e.device_buffer(18)):
            with pytest.raises(ToyboxAmdError) as ei:
                call()
            assert ei.value.code == _abi.E_INVALID


# ---------------------------------------------------------------- the argument shaping

def test_act_args_are_the_planners_rows_behind_the_planner():
    sched = dict(hold=4, objective="survival", rest=1, seed=(7 << 32) | 9, t=5, env_offset=3)
    cases = {"search": (search_args, dict(frames=16, depth=2, **sched)), "search_samples": (search_samples_args, dict(frames=16, depth=2, samples=3, salt=11, **sched)),
             "beam": (beam_args, dict(frames=64, depth=8, width=3, **sched)), "beam_samples": (beam_samples_args, dict(frames=64, depth=6, width=2, samples=4, salt=1, **sched)),
             "evolve": (evolve_args, dict(frames=64, depth=8, population=16, generations=2, elite=4, plan_seed=2 ** 32 - 1, mutation=256, init=4 ** 8 - 1, **sched))}
    for name, (build, kw) in cases.items():
        own, per_env = build("breakout", 1, **kw)
        got = act_args("breakout", name, **kw)
        assert not per_env and got == [float(ACT_PLANNERS[name])] + list(own) and got == act_args("breakout", ACT_PLANNERS[name], **kw)
        assert len(got) == 1 + MOST_COLUMNS[ACT_PLANNERS[name]] <= _abi.EDIT_MAX_ARGS and all(isinstance(v, float) for v in got)
    assert len(act_args("breakout", "evolve", frames=64, depth=8)) == 16 == _abi.EDIT_MAX_ARGS
    # the defaults are the planners' own
    assert act_args("amidar", "search", frames=8) == [153.0, 8.0, 1.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0]
    assert act_args("amidar", 155, frames=8, depth=1, samples=2)[-2:] == [2.0, 0.0]
    assert act_args("amidar", "evolve", frames=8, depth=1)[10:] == [1.0, 0.0, 1.0, 0.0, 64.0, -1.0]


def test_act_args_init_from_the_carry():
    for init in ("carry", -2):
        got = act_args("space_invaders", "evolve", frames=48, depth=12, population=8, generations=1, elite=2, init=init)
        assert got[15] == -2.0 and got[:15] == act_args("space_invaders", "evolve", frames=48, depth=12, population=8, generations=1, elite=2)[:15]
    assert act_args("space_invaders", "evolve", frames=48, depth=12, init=None)[15] == -1.0
    assert act_args("space_invaders", "evolve", frames=48, depth=12, init=6 ** 12 - 1)[15] == float(6 ** 12 - 1)
    with pytest.raises(ValueError):
        evolve_args("space_invaders", 1, 48, 12, init=-2)                  # the plain query keeps refusing it
    for bad in ("last", -3, 6 ** 12):
        with pytest.raises(ValueError):
            act_args("space_invaders", "evolve", frames=48, depth=12, init=bad)


def test_act_args_range_errors():
    for planner in (150, 151, 152, 154, 159, 0, "lookahead"):
        with pytest.raises(ValueError):
            act_args("breakout", planner, frames=8)
    bad = {"search": [dict(depth=7), dict(depth=0), dict(objective=2), dict(rest=2)],
           "search_samples": [dict(depth=2, samples=0), dict(depth=2, samples=4097), dict(depth=6, samples=17), dict(depth=1, samples=1, salt=-1)],
           "beam": [dict(depth=17, width=1), dict(depth=2, width=0), dict(depth=2, width=65)],
           "beam_samples": [dict(depth=2, width=1, samples=0), dict(depth=16, width=64, samples=4096), dict(depth=2, width=1, samples=2, salt=2 ** 32 - 1)],
           "evolve": [dict(depth=17), dict(depth=2, population=257), dict(depth=2, generations=65), dict(depth=2, population=4, elite=5), dict(depth=2, plan_seed=2 ** 32),
                      dict(depth=2, mutation=257), dict(depth=2, init=16)]}
    for planner, rows in bad.items():
        for kw in rows:
            with pytest.raises(ValueError):
                act_args("breakout", planner, frames=8, **kw)
    # shared arguments only
    for kw in (dict(frames=np.array([8])), dict(frames=8, depth=np.array([1])), dict(frames=8, n_envs=4)):
        with pytest.raises(ValueError):
            act_args("breakout", "search", **kw)
    with pytest.raises(ValueError):
        act_args("breakout", "evolve", frames=8, depth=2, init=np.array([3]))


# ---------------------------------------------------------------- the pick and the shift

def _random_rows(rng, n, L, sampled):
    """integer rows with forced ties: keys drawn from two values, so many envs tie on every key; codes of first action a end in
    digit a and come in both orders"""
    names = SAMPLE_FIELDS if sampled else FIELDS
    rows = {k: rng.integers(0, 2, (n, L)).astype(np.int64) for k in names}
    if not sampled:
        rows["life_lost_at"] = rng.choice(np.array([-1, 3, 900]), (n, L))
        rows["ret"] = rows["ret"].astype(np.float64) * 2.0 ** 40
    else:
        rows["ret_sum"] = rows["ret_sum"] * (1 << 40)
    rows["code"] = rng.integers(0, L ** 3, (n, L)) * L + np.arange(L)
    rows["code"][::2] = rows["code"][::2, ::-1] // L * L + np.arange(L)             # larger codes first in every other env
    rows["code"][:8] = np.arange(L)                                                 # ... and the depth-1 codes
    for k in names:
        rows[k][:8] = rows[k][:8, :1]                                               # every key equal in the first envs
    return rows


@pytest.mark.parametrize("sampled", [False, True])
def test_plan_pick_matches_the_replays_pick(sampled):
    rng = np.random.default_rng(159)
    planner = 157 if sampled else 158
    for L in (4, 5, 6):
        rows = _random_rows(rng, 400, L, sampled)
        names = (SAMPLE_FIELDS if sampled else FIELDS) + ("code",)
        packed = np.stack([np.asarray(rows[k], np.float64) for k in names], axis=-1)
        for objective in (0, 1):
            want = pick(rows, planner, objective)
            got = plan_pick(packed, objective, sampled)
            assert got.dtype == np.int64 and np.array_equal(got, want), (L, objective)
            assert np.array_equal(plan_pick(packed, ("return", "survival")[objective], sampled), want)
            tied = act_replay.all_keys_tied(rows, planner, objective)
            assert tied[:8].all() and tied.sum() >= 40 and (want[:8] == 0).all(), "ties on every key, decided by the tie-break"
            if not sampled:
                assert (want[tied] != 0).any(), "a tie that the first index does not win"
    with pytest.raises(ValueError):
        plan_pick(np.zeros((2, 4, 9)), 0, False)
    with pytest.raises(ValueError):
        plan_pick(np.zeros((2, 4, 6)), 2, False)


@pytest.mark.parametrize("game", GAMES)
def test_plan_shift_is_a_roll_of_the_digits(game):
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    rng = np.random.default_rng(7)
    for depth in (1, 2, top):
        codes = [0, L ** depth - 1, L ** (depth - 1), (L ** depth - 1) // 2] + [int(c) for c in rng.integers(0, L ** depth, 50)]
        for code in codes:
            want = int(sum(int(d) * L ** p for p, d in enumerate(np.roll(plan_digits(L, np.uint64(code), depth), -1))))
            assert plan_shift(game, code, depth) == shift(L, code, depth) == want < L ** depth <= 2 ** 32
        arr = plan_shift(game, np.array(codes, np.uint64), depth)
        assert arr.dtype == np.uint64 and [int(c) for c in arr] == [shift(L, c, depth) for c in codes]
    assert plan_shift(game, L ** top - 1, top) == L ** top - 1 and plan_shift(game, 3, 1) == 3
    for depth in (0, top + 1):
        with pytest.raises(ValueError):
            plan_shift(game, 0, depth)


@pytest.mark.parametrize("game", GAMES)
def test_a_carry_is_cut_to_a_shallower_depth(game):
    """init = carry % L ** depth: the first `depth` digits of the carried plan, a valid code of the depth at hand"""
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    rng = np.random.default_rng(11)
    for code in [L ** top - 1] + [int(c) for c in rng.integers(0, L ** top, 20)]:
        carry = shift(L, code, top)
        for depth in (1, 3, top - 1, top):
            init = carry % L ** depth
            assert 0 <= init < L ** depth
            assert list(plan_digits(L, np.uint64(init), depth)) == list(np.roll(plan_digits(L, np.uint64(code), top), -1)[:depth])


# ---------------------------------------------------------------- the replay's closed loop

@pytest.mark.parametrize("game", ["breakout", "gridworld"])
def test_the_replays_closed_loop_is_deterministic(game, oracle_lib):
    """two runs from one batch agree in every period and leave the same records; the rows have the header's layout"""
    n, k = 6, 3
    case = dict(frames=16, hold=4, depth=4, objective=0, rest=LEGAL[game][0], population=4, generations=1, elite=2, mutation=128, plan_seed=3, init=-2)
    start = batch(oracle_lib, game, n, frames=BATCH_FRAMES[game])
    runs = []
    for _ in range(2):
        e = clone_of(oracle_lib, start)
        runs.append((expected_rollout(oracle_lib, game, e, EVOLVE, k, case), e.get_states(), e.scalars()))
        e.close()
    for a, b in zip(runs[0][0], runs[1][0]):
        assert all(np.array_equal(a[key], b[key]) for key in ("out", "action", "carry", "lives"))
    assert bytes(runs[0][1]) == bytes(runs[1][1])
    L = len(LEGAL[game])
    for p in runs[0][0]:
        assert p["out"].shape == (n, 11) and (p["out"][:, 8:] == 0).all() and np.array_equal(p["out"][:, 0], np.asarray(LEGAL[game])[p["out"][:, 1].astype(int)])
        assert np.array_equal(p["out"][:, 7].astype(np.int64) % L, p["out"][:, 1].astype(np.int64)), "the winner's code begins with the winner"
        assert [int(c) for c in p["carry"]] == [shift(L, int(c), 4) for c in p["out"][:, 7]]
    start.close()
