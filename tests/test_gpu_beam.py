"""Beam search on the device (TBX_QUERY_LOOKAHEAD_BEAM, include/toybox_amd.h) against CLONE AND PLAY LEVEL BY LEVEL on the CPU
checker (tests/beam_replay.py; its own checks are in tests/test_beam.py).  Every comparison is exact, on every field of every row.

The worlds are those of tests/test_gpu_search.py (_world): made by the input recipe of tests/lookahead_replay.py and held to their
checker twins byte for byte before any query; the expected rows are played on clones of the records the DEVICE engine reports.
Measured on the checker (tests/test_beam.py prints them), replay of both objectives together and, summed over the objectives,
groups strictly worse than the exhaustive search / equal to it / (group, level) cuts decided by the code / kept sets that are not
the first `width` codes / final winners that are not the smallest code / groups where the objectives disagree / envs with an
ended candidate:
  Breakout (24, 96, 8, 8, 3) 7.3 s - / - / 1298 / 78 / 6 / 0 / 34; (96, 200, 8, 3, 1) 1.9 s 84 / 682 / 1392 / 144 / 8 / 2 / 160;
  (24, 64, 4, 4, 8) 3.5 s - / - / 384 / 98 / 46 / 0 / 26;  Amidar (24, 96, 4, 6, 3) 8.3 s - / - / 1394 / 130 / 4 / 0 / 6;
  (96, 128, 8, 3, 1, batch 900) 2.4 s 89 / 1063 / 2136 / 168 / 55 / 5 / 8;  GridWorld (24, 40, 2, 7, 4) 4.9 s - / - / 1440 / 22 / 0 / 0 / 0;
  (96, 40, 2, 3, 1, batch 80) 0.6 s 81 / 879 / 1874 / 46 / 1 / 6 / 6;  SpaceInvaders (12, 96, 8, 6, 3) 7.0 s - / - / 666 / 319 / 48 / 11 / 10;
  (24, 96, 8, 3, 1) 1.3 s 78 / 202 / 469 / 157 / 97 / 7 / 18.  Those times are of an 8-core host; the GPU host replays every deep case
  in 0.8 to 1.6 s per objective (the module's slowest test, 2.4 s, is Amidar's coverage test)."""
import functools

import numpy as np
import pytest

from beam_replay import BEAM_CASES, DRAWN_BEAM, case_beam, case_coverage, expected_beam, missing_coverage, not_worse
from fork_replay import sim_rngs
from lookahead_replay import FIELDS, assert_fields_equal, batch
from search_replay import SEARCH_FIELDS, assert_search_equal, expected_search
from support import LEGAL
from test_gpu_custom_states import _engines, _write_all, fuzz_seed, generate  # noqa: F401  (fuzz_seed: the fixture)
from test_gpu_search import _assert_same_snapshot, _device_reduce, _held_to_twin, _search_dict, _snapshot, _world, pick_rows
from toybox_amd import ToyboxAmdError, _abi
from toybox_amd.engine import Engine, beam_args, plan_actions, plan_args

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
OBJECTIVES = ["return", "survival"]
CASES = [(game, case) for game in GAMES for case in BEAM_CASES[game]]
SEARCH_DEPTH = {"breakout": 6, "space_invaders": 4, "amidar": 4, "gridworld": 5}      # the deepest the exhaustive search accepts


@functools.lru_cache(maxsize=None)
def _replay(game, case, objective, drawn, hip_lib, oracle_lib):
    """(rows, levels) of the case replayed on the checker, made once, shared and left unchanged"""
    _, states, rngs = _world(game, case[0], case[5], hip_lib, oracle_lib)
    rows, levels = expected_beam(oracle_lib, game, states, rngs, dict(case_beam(game, case), objective=objective, **(DRAWN_BEAM if drawn else {})))
    for v in rows.values():
        v.flags.writeable = False
    return rows, levels


# ---------------------------------------------------------------- 1. rows equal the replay

@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("game,case", CASES, ids=["%s-%d-%d-%d-%d-%d" % ((g,) + c[:5]) for g, c in CASES])
def test_beam_equals_replay(game, case, objective, hip_lib, oracle_lib):
    n, frames, hold, depth, width, batch_frames = case
    L = len(LEGAL[game])
    g, _, _ = _world(game, n, batch_frames, hip_lib, oracle_lib)
    want, _ = _replay(game, case, OBJECTIVES.index(objective), False, hip_lib, oracle_lib)
    got = g.lookahead_beam(frames, depth, width, hold=hold, objective=objective, rest=LEGAL[game][0])
    assert got["ret"].shape == (n, L) and got["ret"].dtype == np.float64 and got["code"].dtype == np.uint64 and got["plan"].shape == (n, L, depth)
    assert_search_equal(got, want, "%s %r %s" % (game, case, objective))
    assert np.array_equal(got["plan"], plan_actions(game, want["code"], depth)) and np.array_equal(got["plan"][:, :, 0], np.tile(LEGAL[game], (n, 1)))
    assert g.beam_ranges == 1
    if case is BEAM_CASES[game][0]:
        assert L ** depth > _abi.LOOKAHEAD_MAX_PLANS, "the deep case is one no enumeration reaches"


@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("game", GAMES)
def test_beam_with_drawn_rest_actions(game, objective, hip_lib, oracle_lib):
    """the deep case with rest = -1: the synthetic rule with a seed above 32 bits, a counter that leaves 32 bits and an env offset"""
    case = BEAM_CASES[game][0]
    n, frames, hold, depth, width, batch_frames = case
    g, _, _ = _world(game, n, batch_frames, hip_lib, oracle_lib)
    want, _ = _replay(game, case, OBJECTIVES.index(objective), True, hip_lib, oracle_lib)
    kw = dict(hold=hold, objective=objective, rest=None, t=DRAWN_BEAM["t"], env_offset=DRAWN_BEAM["env_offset"])
    got = g.lookahead_beam(frames, depth, width, seed=DRAWN_BEAM["seed"], **kw)
    assert_search_equal(got, want, "%s drawn rest, %s" % (game, objective))
    other = g.lookahead_beam(frames, depth, width, seed=DRAWN_BEAM["seed"] ^ (1 << 40), **kw)
    assert any(not np.array_equal(other[k], got[k]) for k in SEARCH_FIELDS), "the upper half of the seed is not read"


# ---------------------------------------------------------------- 2. the cases cover what they must

@pytest.mark.parametrize("game", GAMES)
def test_the_cases_cover_what_they_must(game, hip_lib, oracle_lib):
    """asserted on the expected arrays, so no test passes by avoiding the hard rows"""
    totals = {}
    for case in BEAM_CASES[game]:
        n, frames, hold, depth, width, batch_frames = case
        beam = {o: _replay(game, case, o, False, hip_lib, oracle_lib) for o in (0, 1)}
        search = None
        if width == 1 and len(LEGAL[game]) ** depth <= _abi.LOOKAHEAD_MAX_PLANS:
            _, states, rngs = _world(game, n, batch_frames, hip_lib, oracle_lib)
            search = {o: expected_search(oracle_lib, game, states, rngs, dict(frames=frames, hold=hold, depth=depth, objective=o, rest=LEGAL[game][0])) for o in (0, 1)}
        for k, v in case_coverage(game, case, beam, search).items():
            totals[k] = totals.get(k, 0) + int(v)
    missing = missing_coverage(game, totals)
    assert not missing, "%s: the beam cases together never show: %s" % (game, ", ".join(missing))


# ---------------------------------------------------------------- 3. the device equals itself

@pytest.mark.parametrize("game", GAMES)
def test_a_beam_wide_enough_is_the_search(game, hip_lib, oracle_lib):
    """width = n_legal ** (depth - 2) and width = 64 at the deepest depth the search accepts at which 64 is still wide enough
    (Breakout 5, where 4 ** 3 is 64 itself; GridWorld 4; SpaceInvaders and Amidar 4, their deepest), and depth 1"""
    n, L = 24, len(LEGAL[game])
    depth = max(d for d in range(2, SEARCH_DEPTH[game] + 1) if L ** (d - 2) <= _abi.BEAM_MAX_WIDTH)
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    kw = dict(hold=4, rest=LEGAL[game][1])
    for objective in OBJECTIVES:
        for d, width in ((3, L), (depth, L ** (depth - 2)), (depth, 64), (1, 1), (1, 7)):
            a = g.lookahead_beam(40, d, width, objective=objective, **kw)
            b = g.lookahead_search(40, d, objective=objective, **kw)
            for k in SEARCH_FIELDS + ("plan",):
                assert np.array_equal(a[k], b[k]), (game, objective, d, width, k)
        # the deepest depth the search accepts (Breakout 6, GridWorld 5: 64 is narrower than n_legal ** (depth - 2) there, so equality
        # is not promised): the search's row is the optimum, no beam row beats it
        a = g.lookahead_beam(40, SEARCH_DEPTH[game], 64, objective=objective, **kw)
        b = g.lookahead_search(40, SEARCH_DEPTH[game], objective=objective, **kw)
        assert not_worse(OBJECTIVES.index(objective), b, a).all() and (a["frames_run"] > 0).all(), (game, objective)


@pytest.mark.parametrize("game", GAMES)
def test_every_code_of_the_deepest_beam_reproduces_its_row(game, hip_lib, oracle_lib):
    """depth = TBX_PLAN_MAX_DEPTH, width 2, frames = hold * depth: every period plays a digit; Breakout codes run up to 2^32 - 1"""
    n, L, top, hold = 24, len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game], 4
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    for objective in OBJECTIVES:
        res = g.lookahead_beam(hold * top, top, 2, hold=hold, objective=objective, rest=LEGAL[game][0])
        assert (res["frames_run"] > 0).all() and res["plan"].shape == (n, L, top)
        for a in range(L):
            assert (res["code"][:, a] % np.uint64(L) == a).all()
            args, _ = plan_args(game, n, hold * top, hold=hold, depth=top, code=res["code"][:, a], rest=LEGAL[game][0])
            again = Engine._lookahead_dict(g.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args))
            assert_fields_equal(again, {k: res[k][:, a] for k in FIELDS}, "%s %s first action %d" % (game, objective, a))


@pytest.mark.parametrize("game", GAMES)
def test_a_deeper_beam_is_not_worse_under_a_fixed_rest(game, hip_lib, oracle_lib):
    """the child that repeats `rest` replays its parent, so the best of level d is at least the best of level d - 1"""
    g, _, _ = _world(game, 24, 400, hip_lib, oracle_lib)
    for o, objective in enumerate(OBJECTIVES):
        rows = [g.lookahead_beam(64, d, 3, hold=4, objective=objective, rest=LEGAL[game][1]) for d in range(1, 8)]
        for shallow, deep in zip(rows, rows[1:]):
            assert not_worse(o, deep, shallow).all(), (game, objective)


@pytest.mark.parametrize("game", GAMES)
def test_env_ranges_change_no_bit(game, hip_lib, oracle_lib):
    """TBX_OPT_BEAM_RANGE_ENVS = 5 on 24 envs: five ranges, the last of four envs, and the one-range answer"""
    g, _, _ = _world(game, 24, 400, hip_lib, oracle_lib)
    kw = dict(hold=4, objective="survival", rest=LEGAL[game][0])
    one = g.lookahead_beam(56, 7, 3, **kw)
    assert g.beam_ranges == 1 and g.beam_range_envs == 0
    g.beam_range_envs = 5
    try:
        cut = g.lookahead_beam(56, 7, 3, **kw)
        assert g.beam_range_envs == 5 and g.beam_ranges == 5
    finally:
        g.beam_range_envs = 0
    for k in SEARCH_FIELDS + ("plan",):
        assert np.array_equal(one[k], cut[k]), k
    assert (one["frames_run"] > 0).all() and len(np.unique(one["code"])) > len(LEGAL[game])


# ---------------------------------------------------------------- 4. per-env rows with bad rows among them

@pytest.mark.parametrize("game", GAMES)
def test_per_env_rows_with_bad_rows_among_them(game, hip_lib, oracle_lib):
    """mixed depths (one above the enumeration cap), widths, objectives and holds, one row per refusal reason; the host form and
    the device form on a caller's stream: refused rows are zeros, the others the replay's and those of shared arguments"""
    n = 24
    g, states, rngs = _world(game, n, 400, hip_lib, oracle_lib)
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    illegal = 2 if game == "breakout" else 17
    s = dict(frames=np.full(n, 32), hold=np.resize([4, 2, 8], n), depth=np.resize([1, 2, 3, SEARCH_DEPTH[game] + 1], n), objective=np.resize([0, 1], n),
             rest=np.full(n, LEGAL[game][0]), width=np.resize([1, 2, 3, 7, 2], n))
    s["depth"][[1, 2]] = [0, top + 1]
    s["objective"][5] = 2
    s["rest"][8] = illegal
    s["frames"][[10, 11]] = [0, 1025]
    s["hold"][13] = 0
    s["width"][[14, 16]] = [0, 65]
    bad = [1, 2, 5, 8, 10, 11, 13, 14, 16]
    good = np.setdiff1d(np.arange(n), bad)
    want, _ = expected_beam(oracle_lib, game, states, rngs, s)
    assert all((want[k][bad] == 0).all() for k in SEARCH_FIELDS) and (want["frames_run"][good] > 0).all()
    assert (s["depth"][good] > SEARCH_DEPTH[game]).any()
    args, per_env = beam_args(game, n, s["frames"], s["depth"], s["width"], hold=s["hold"], objective=s["objective"], rest=s["rest"])
    assert per_env and args.shape == (n, 10)
    before = _snapshot(g)
    assert_search_equal(_search_dict(g.reduce(_abi.QUERY_LOOKAHEAD_BEAM, args), n, L), want, "%s beam rows (host form)" % game)
    assert_search_equal(_search_dict(_device_reduce(g, _abi.QUERY_LOOKAHEAD_BEAM, args, 6 * L), n, L), want, "%s beam rows (device form)" % game)
    _assert_same_snapshot(_snapshot(g), before, "%s per-env rows" % game)
    seen = set()
    for i in good:                                            # the same envs asked with shared arguments
        key = tuple(int(s[k][i]) for k in ("frames", "hold", "depth", "objective", "width"))
        if key in seen:
            continue
        seen.add(key)
        shared = g.lookahead_beam(key[0], key[2], key[4], hold=key[1], objective=key[3], rest=LEGAL[game][0])
        same = [j for j in good if tuple(int(s[k][j]) for k in ("frames", "hold", "depth", "objective", "width")) == key]
        for k in SEARCH_FIELDS:
            assert np.array_equal(np.asarray(shared[k][same], np.float64), np.asarray(want[k][same], np.float64)), (game, key, k)


# ---------------------------------------------------------------- 5. forms

def _beam_against_replay(g, game, oracle_lib, what, frames=48, hold=4, depth=4, width=2):
    states, rngs = g.get_states(), sim_rngs(g)
    rest = LEGAL[game][2]
    for o, objective in enumerate(OBJECTIVES):
        want, levels = expected_beam(oracle_lib, game, states, rngs, dict(frames=frames, hold=hold, depth=depth, width=width, objective=o, rest=rest))
        got = g.lookahead_beam(frames, depth, width, hold=hold, objective=objective, rest=rest)
        assert_search_equal(got, want, "%s beam %s" % (what, objective))
    return levels


@pytest.mark.parametrize("game", ["breakout", "space_invaders"])
def test_written_states(game, fuzz_seed, hip_lib, oracle_lib):
    """a Breakout batch that has left the canonical wall (the wave form with per-env brick tables) and a SpaceInvaders batch off the
    formation grid (the full load), built the way tests/test_gpu_custom_states.py builds them"""
    n = 24
    es = g, o = _engines(game, n, (hip_lib, oracle_lib))
    _write_all(es, generate(game, o, np.random.default_rng(fuzz_seed)))
    for e in es:
        for t in range(20):
            e.step_synthetic(1337, t, auto_reset=True)
    _held_to_twin(g, o, "%s written states" % game)
    levels = _beam_against_replay(g, game, oracle_lib, "%s written states" % game)
    assert any((lv["ret"] > 0).any() for lv in levels)
    _held_to_twin(g, o, "%s written states after the queries" % game)
    g.close(); o.close()


def test_breakout_wave_per_env_step_form(hip_lib, oracle_lib):
    """TBX_OPT_STEP_FORM = 2: the canonical wall through the wave form"""
    n = 24
    g = Engine("breakout", n, lib=hip_lib)
    g.set_option(_abi.OPT_STEP_FORM, _abi.STEP_FORM_WAVE_PER_ENV)
    o = batch(oracle_lib, "breakout", n)
    g.set_states(0, o.get_states())
    for i, r in enumerate(sim_rngs(o)):
        g.set_sim_rng((int(r[0]), int(r[1])), env=i)
    _held_to_twin(g, o, "breakout, wave per env")
    _beam_against_replay(g, "breakout", oracle_lib, "breakout, wave per env")
    g.close(); o.close()


def test_the_adapter_after_agent_init(hip_lib, oracle_lib):
    """ToyboxPreprocVecEnv.beam_search: agent steps, action indices, the engine's rows and the winner among an env's rows"""
    from toybox_amd.envs import ToyboxPreprocVecEnv
    game, n = "space_invaders", 24
    L = len(LEGAL[game])
    v = ToyboxPreprocVecEnv(game, n, seed=3, engine=Engine(game, n, lib=hip_lib))
    v.reset()
    rng = np.random.default_rng(0)
    for _ in range(20):
        v.step(rng.integers(0, v.action_space.n, n))
    v.step_async(rng.integers(0, v.action_space.n, n))        # a pending step ends first
    for o, objective in enumerate(OBJECTIVES):
        got = v.beam_search(steps=12, depth=5, width=2, objective=objective, rest=0)
        assert v._in_flight is None
        rows = v.engine.lookahead_beam(48, 5, 2, hold=4, objective=objective, rest=LEGAL[game][0])
        want, _ = expected_beam(oracle_lib, game, v.engine.get_states(), sim_rngs(v.engine), dict(frames=48, hold=4, depth=5, width=2, objective=o, rest=LEGAL[game][0]))
        assert_search_equal(got, rows, "ToyboxPreprocVecEnv.beam_search %s against the engine" % objective)
        assert_search_equal(got, want, "ToyboxPreprocVecEnv.beam_search %s" % objective)
        digits = np.stack([want["code"] // L ** p % L for p in range(5)], axis=-1)
        assert np.array_equal(got["plan"], digits) and np.array_equal(np.asarray(LEGAL[game])[got["plan"]], rows["plan"])
        best = pick_rows(want, o)
        assert np.array_equal(got["best_action"], best) and np.array_equal(got["best_plan"], got["plan"][np.arange(n), best])
        assert np.array_equal(got["best_plan"][:, 0], got["best_action"]), "the first digit of the best plan is the best action"
    v.close()


def test_batch_intervention_mirrors_the_engine(hip_lib, oracle_lib):
    from toybox_amd.interventions import BatchIntervention
    game, n, first, count = "breakout", 24, 5, 11
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    depth, width = np.resize([7, 2, 5], n), np.resize([2, 3], n)
    whole = g.lookahead_beam(48, depth, width, hold=4, objective="survival", rest=0)
    with BatchIntervention(g, first, count) as bi:
        part = bi.lookahead_beam(48, depth[first:first + count], width[first:first + count], hold=4, objective="survival", rest=0)
    for k in SEARCH_FIELDS:
        assert np.array_equal(part[k], whole[k][first:first + count]), k
    assert (whole["frames_run"] > 0).all()


# ---------------------------------------------------------------- 6. nothing written

@pytest.mark.parametrize("game", GAMES)
def test_the_query_leaves_the_engine_untouched(game, hip_lib, oracle_lib):
    """state records, simulator RNGs, step outputs and scalars are byte-equal before and after a query of several ranges and levels,
    and the next synthetic step gives what an untouched twin gives"""
    n = 24
    g, twin = batch(hip_lib, game, n), batch(hip_lib, game, n)
    before = _snapshot(g)
    g.beam_range_envs = 7
    g.lookahead_beam(40, 7, 3, hold=4, objective="survival", rest=LEGAL[game][0])
    assert g.beam_ranges == 4
    _assert_same_snapshot(_snapshot(g), before, game)
    for e in (g, twin):
        e.step_synthetic(1337, 400, auto_reset=True)
    _assert_same_snapshot(_snapshot(g), _snapshot(twin), "%s: the step after the query" % game)
    g.close(); twin.close()


# ---------------------------------------------------------------- 7. shared refusals

@pytest.mark.parametrize("game", GAMES)
def test_shared_refusals(game, hip_lib, oracle_lib):
    g, _, _ = _world(game, 24, 400, hip_lib, oracle_lib)
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    illegal = 2 if game == "breakout" else 17
    g.lookahead_beam(8, 2, 2)
    ranges, before = g.beam_ranges, _snapshot(g)
    g.beam_range_envs = 5
    bad = {"depth": [[8, 1, 0], [8, 1, top + 1]], "objective": [[8, 1, 2, 2]], "rest": [[8, 1, 2, 0, illegal]], "frames": [[0], [1025]], "hold": [[8, 0]],
           "width": [[8, 1, 2, 0, -1, 0, 0, 0, 0, 0], [8, 1, 2, 0, -1, 0, 0, 0, 0, 65]], "beam takes": [[8, 1, 1, 0, -1, 0, 0, 0, 0, 1, 0], []]}
    try:
        for name, rows in bad.items():
            for args in rows:
                with pytest.raises(ToyboxAmdError) as ei:
                    g.reduce(_abi.QUERY_LOOKAHEAD_BEAM, args)
                assert ei.value.code == _abi.E_INVALID and name in str(ei.value), (name, args, str(ei.value))
                assert g.beam_ranges == ranges, "a refusal leaves TBX_OPT_BEAM_RANGES standing"
    finally:
        g.beam_range_envs = 0
    _assert_same_snapshot(_snapshot(g), before, "%s after the refusals" % game)
    assert g.reduce(_abi.QUERY_LOOKAHEAD_BEAM, [8, 1, top, 1, -1, 0, 0, 0, 0, 64]).shape == (24, 6 * L)       # the deepest, widest beam
    with pytest.raises(ToyboxAmdError):
        g.set_option(_abi.OPT_BEAM_RANGE_ENVS, -1)
    with pytest.raises(ToyboxAmdError):
        g.set_option(_abi.OPT_BEAM_RANGES, 1)
    for name in GAMES:
        assert hip_lib.tbx_reduce_width(_abi.GAME_IDS[name], _abi.QUERY_LOOKAHEAD_BEAM) == 6 * len(LEGAL[name])
