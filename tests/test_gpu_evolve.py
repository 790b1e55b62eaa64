"""Evolutionary plan search on the device (TBX_QUERY_LOOKAHEAD_EVOLVE, include/toybox_amd.h) against CLONE AND PLAY GENERATION BY
GENERATION on the CPU checker (tests/evolve_replay.py; its own checks are in tests/test_evolve.py).  Every comparison is exact, on
every field of every row.

The worlds are those of tests/test_gpu_search.py (_world): made by the input recipe of tests/lookahead_replay.py and held to their
checker twins byte for byte before any query; the expected rows are played on clones of the records the DEVICE engine reports.
The shapes (envs, frames, hold, depth, population, generations, elite, mutation): deep (24, 96, 8, 8, 16, 3, 4, 64) with a fixed
init plan in the even envs through per-env rows; wide (12, 64, 4, 4, 65, 1, 3, 128); full (4, 40, 4, 3, 256, 1, 2, 256); deepest
(24, hold x depth, 4, TBX_PLAN_MAX_DEPTH, 8, 2, 2, 64).  Batches: 400 frames of synthetic play, GridWorld 40.
Measured on the checker (tests/test_evolve.py prints them), summed over the two objectives, per case deep / wide / full / deepest --
groups whose final winner is not generation 0's; populations with a rank decided by the code alone; populations holding a duplicate
code; children that keep at least one and change at least one of their parent's digits; envs with an ended individual; plans played:
  Breakout      188 / 42 / 0 / 186;  768 / 192 / 64 / 576;   562 / 192 / 64 / 104;  5306 / 4166 / 3054 / 2194;  34 / 10 / 4 / 26;  9984 / 12192 / 16320 / 3840
  SpaceInvaders 266 / 84 / 0 / 248;  1152 / 288 / 96 / 864;  813 / 288 / 96 / 212;  8375 / 6594 / 3394 / 3222;  20 / 6 / 0 / 4;    14976 / 18288 / 24480 / 5760
  Amidar        268 / 112 / 0 / 258; 1152 / 288 / 96 / 864;  810 / 288 / 96 / 218;  8314 / 6568 / 3414 / 3214;  6 / 4 / 0 / 8;     14976 / 18288 / 24480 / 5760
  GridWorld     227 / 34 / 0 / 214;  960 / 240 / 80 / 720;   694 / 240 / 80 / 176;  6876 / 5312 / 3356 / 2666;  10 / 0 / 0 / 12;   12480 / 15240 / 20400 / 4800
The replay of a case takes 0.3 to 2.4 s per objective on an 8-core host (the individuals of a first action are played side by side
in one checker clone)."""
import functools

import numpy as np
import pytest

from evolve_replay import DRAWN_EVOLVE, EVOLVE_SHAPES, PLAN_SEED, case_evolve, evolve_stats, expected_evolve, missing_coverage, not_worse
from fork_replay import Agent, sim_rngs
from lookahead_replay import FIELDS, assert_fields_equal, batch
from search_replay import SEARCH_FIELDS, assert_search_equal
from support import LEGAL, read_buffer
from test_gpu_custom_states import _engines, _write_all, fuzz_seed, generate  # noqa: F401  (fuzz_seed: the fixture)
from test_gpu_search import _assert_same_snapshot, _device_reduce, _held_to_twin, _search_dict, _snapshot, _world, pick_rows
from toybox_amd import ToyboxAmdError, _abi
from toybox_amd.engine import Engine, evolve_args, plan_actions, plan_args

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
OBJECTIVES = ["return", "survival"]
CASES = [(game, name) for game in GAMES for name in EVOLVE_SHAPES]
SEARCH_DEPTH = {"breakout": 6, "space_invaders": 4, "amidar": 4, "gridworld": 5}      # the deepest the exhaustive search accepts
EVOLVE = _abi.QUERY_LOOKAHEAD_EVOLVE


@functools.lru_cache(maxsize=None)
def _replay(game, name, objective, drawn, hip_lib, oracle_lib):
    """(rows, gens) of the case replayed on the checker, made once, shared and left unchanged"""
    ev, n, batch_frames = case_evolve(game, name)
    _, states, rngs = _world(game, n, batch_frames, hip_lib, oracle_lib)
    rows, gens = expected_evolve(oracle_lib, game, states, rngs, dict(ev, objective=objective, **(DRAWN_EVOLVE if drawn else {})))
    for v in rows.values():
        v.flags.writeable = False
    return rows, gens


def _ask(g, ev, **more):
    """Engine.lookahead_evolve with the keyword arguments of expected_evolve"""
    kw = dict(ev, **more)
    rest = kw.pop("rest", -1)
    return g.lookahead_evolve(kw.pop("frames"), kw.pop("depth"), kw.pop("population"), kw.pop("generations"), rest=None if np.ndim(rest) == 0 and rest == -1 else rest, **kw)


def _plan_rows(g, game, ev, code):
    """TBX_QUERY_LOOKAHEAD_PLAN on the device for per-env codes under the schedule of `ev`"""
    sched = {k: ev[k] for k in ("hold", "seed", "t", "env_offset") if k in ev}
    rest = ev.get("rest", -1)
    args, _ = plan_args(game, g.n_envs, ev["frames"], depth=ev["depth"], code=code, rest=None if rest == -1 else rest, **sched)
    return Engine._lookahead_dict(g.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args))


# ---------------------------------------------------------------- 1. rows equal the replay

@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("game,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_evolve_equals_replay(game, name, objective, hip_lib, oracle_lib):
    ev, n, batch_frames = case_evolve(game, name)
    L, depth = len(LEGAL[game]), ev["depth"]
    g, _, _ = _world(game, n, batch_frames, hip_lib, oracle_lib)
    want, _ = _replay(game, name, OBJECTIVES.index(objective), False, hip_lib, oracle_lib)
    got = _ask(g, ev, objective=objective)
    assert got["ret"].shape == (n, L) and got["ret"].dtype == np.float64 and got["code"].dtype == np.uint64 and got["plan"].shape == (n, L, depth)
    assert_search_equal(got, want, "%s %s %s" % (game, name, objective))
    assert np.array_equal(got["plan"], plan_actions(game, want["code"], depth)) and np.array_equal(got["plan"][:, :, 0], np.tile(LEGAL[game], (n, 1)))
    assert g.evolve_ranges == 1 and (want["frames_run"] > 0).all()
    if name == "deepest":
        assert depth == _abi.PLAN_MAX_DEPTH[game] and int(want["code"].max()) >= L ** (depth - 1), "the top digit is played"
    if name == "deep":
        assert np.ndim(ev["init"]) == 1 and (ev["init"] >= 0).sum() == n // 2, "an init in half of the envs, through per-env rows"


@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("game", GAMES)
def test_evolve_with_drawn_rest_actions(game, objective, hip_lib, oracle_lib):
    """the deep case with rest = -1: the synthetic rule with a seed above 32 bits, a counter that leaves 32 bits and an env offset
    (which the base word reads too)"""
    ev, n, batch_frames = case_evolve(game, "deep")
    g, _, _ = _world(game, n, batch_frames, hip_lib, oracle_lib)
    want, _ = _replay(game, "deep", OBJECTIVES.index(objective), True, hip_lib, oracle_lib)
    got = _ask(g, ev, objective=objective, **DRAWN_EVOLVE)
    assert_search_equal(got, want, "%s drawn rest, %s" % (game, objective))
    other = _ask(g, ev, objective=objective, **dict(DRAWN_EVOLVE, seed=DRAWN_EVOLVE["seed"] ^ (1 << 40)))
    assert any(not np.array_equal(other[k], got[k]) for k in SEARCH_FIELDS), "the upper half of the seed is not read"


# ---------------------------------------------------------------- 2. the cases cover what they must

@pytest.mark.parametrize("game", GAMES)
def test_the_cases_cover_what_they_must(game, hip_lib, oracle_lib):
    """asserted on the expected arrays, so no test passes by avoiding the hard rows"""
    totals = {}
    for name in EVOLVE_SHAPES:
        for o in (0, 1):
            _, gens = _replay(game, name, o, False, hip_lib, oracle_lib)
            for k, v in evolve_stats(game, gens, o, case_evolve(game, name)[0]["depth"]).items():
                totals[k] = totals.get(k, 0) + int(v)
    missing = missing_coverage(game, totals)
    assert not missing, "%s: the evolve cases together never show: %s" % (game, ", ".join(missing))


# ---------------------------------------------------------------- 3. the device equals itself: the consequences of the definition

@pytest.mark.parametrize("game", GAMES)
def test_the_consequences_hold_on_the_device(game, hip_lib, oracle_lib):
    n, L = 24, len(LEGAL[game])
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    depth = SEARCH_DEPTH[game]
    sched = dict(frames=10 * depth, hold=4, rest=LEGAL[game][1], seed=3, t=9)
    for o, objective in enumerate(OBJECTIVES):
        ev = dict(sched, depth=depth, objective=objective, population=12, elite=3, mutation=96, plan_seed=77)
        # (i) one individual, no generation, an init: query 152's row for the init with its first digit replaced
        c = (np.arange(n, dtype=np.int64) * 977 + 5) % L ** depth
        one = _ask(g, dict(sched, depth=depth, objective=objective, population=1, generations=0), init=c)
        for a in range(L):
            assert np.array_equal(one["code"][:, a].astype(np.int64), c - c % L + a)
            assert_fields_equal({k: one[k][:, a] for k in FIELDS}, _plan_rows(g, game, dict(sched, depth=depth), c - c % L + a), "%s (i) first action %d" % (game, a))
        # (ii) more generations are not worse
        rows = [_ask(g, ev, generations=G) for G in (0, 1, 2, 5)]
        for fewer, more in zip(rows, rows[1:]):
            assert not_worse(o, more, fewer).all(), (game, objective)
        assert any(not np.array_equal(rows[0]["code"], r["code"]) for r in rows[1:]), "no generation ever changed a winner"
        # (iii) the returned code, fed to query 152, gives the row
        for a in range(L):
            assert (rows[-1]["code"][:, a] % np.uint64(L) == a).all()
            assert_fields_equal(_plan_rows(g, game, dict(sched, depth=depth), rows[-1]["code"][:, a]), {k: rows[-1][k][:, a] for k in FIELDS}, "%s (iii) %d" % (game, a))
        # (iv) where query 153 accepts the depth, its row is not worse
        search = g.lookahead_search(sched["frames"], depth, hold=4, objective=objective, rest=sched["rest"], seed=3, t=9)
        assert not_worse(o, search, rows[-1]).all() and (rows[-1]["frames_run"] > 0).all()
        # (v) elite = population, or no mutation: generation 0's winner, whatever G is
        for still in (dict(elite=12), dict(mutation=0)):
            for G in (1, 4):
                again = _ask(g, dict(ev, **still), generations=G)
                assert all(np.array_equal(again[k], rows[0][k]) for k in SEARCH_FIELDS + ("plan",)), (game, objective, still, G)
        # (vi) depth 1: query 152's row for code a
        flat = _ask(g, dict(ev, depth=1), generations=2)
        for a in range(L):
            assert (flat["code"][:, a] == a).all()
            assert_fields_equal({k: flat[k][:, a] for k in FIELDS}, _plan_rows(g, game, dict(sched, depth=1), np.full(n, a)), "%s (vi) %d" % (game, a))


@pytest.mark.parametrize("game", GAMES)
def test_env_ranges_change_no_bit(game, hip_lib, oracle_lib):
    """TBX_OPT_BEAM_RANGE_ENVS = 7 on 24 envs: four ranges, the last of three envs, and the one-range answer"""
    g, _, _ = _world(game, 24, 400, hip_lib, oracle_lib)
    ev = dict(frames=56, hold=4, depth=7, population=10, generations=2, elite=3, mutation=64, plan_seed=5, objective="survival", rest=LEGAL[game][0])
    one = _ask(g, ev)
    assert g.evolve_ranges == 1 and g.beam_range_envs == 0
    g.beam_range_envs = 7
    try:
        cut = _ask(g, ev)
        assert g.beam_range_envs == 7 and g.evolve_ranges == 4
    finally:
        g.beam_range_envs = 0
    for k in SEARCH_FIELDS + ("plan",):
        assert np.array_equal(one[k], cut[k]), k
    assert (one["frames_run"] > 0).all() and len(np.unique(one["code"])) > len(LEGAL[game])


# ---------------------------------------------------------------- 4. per-env rows with bad rows among them

@pytest.mark.parametrize("game", GAMES)
def test_per_env_rows_with_bad_rows_among_them(game, hip_lib, oracle_lib):
    """mixed populations, generations, elites, depths and objectives, one row per refusal reason; the host form (which scans its
    rows) and the device form on a caller's stream (which cannot, and runs every round): refused rows are zeros, the others the
    replay's and those of shared arguments"""
    n = 24
    g, states, rngs = _world(game, n, 400, hip_lib, oracle_lib)
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    s = dict(frames=np.full(n, 32), hold=np.resize([4, 2, 8], n), depth=np.resize([1, 2, 3, SEARCH_DEPTH[game] + 1], n), objective=np.resize([0, 1], n),
             rest=np.full(n, LEGAL[game][0]), population=np.resize([1, 5, 9, 70, 2], n), generations=np.resize([0, 1, 3, 2], n), elite=np.resize([1, 2, 1, 5], n),
             plan_seed=np.resize([9, 2 ** 32 - 1], n), mutation=np.resize([64, 256, 0, 200], n), init=np.full(n, -1))
    s["elite"] = np.minimum(s["elite"], s["population"])
    s["init"][[3, 7]] = [L ** int(s["depth"][3]) - 1, 0]
    s["elite"][1] = s["population"][1] + 1                    # elite > population
    s["init"][2] = L ** int(s["depth"][2])                    # init >= L^depth
    s["population"][[5, 8]] = [0, 257]
    s["generations"][10] = 65
    s["mutation"][11] = 257
    s["plan_seed"][13] = 2 ** 32
    s["depth"][14] = top + 1
    s["objective"][16] = 2
    s["init"][17] = -2
    bad = [1, 2, 5, 8, 10, 11, 13, 14, 16, 17]
    good = np.setdiff1d(np.arange(n), bad)
    want, _ = expected_evolve(oracle_lib, game, states, rngs, s)
    assert all((want[k][bad] == 0).all() for k in SEARCH_FIELDS) and (want["frames_run"][good] > 0).all()
    assert (s["depth"][good] > SEARCH_DEPTH[game]).any() and (s["population"][good] > 64).any()
    args, per_env = evolve_args(game, n, s["frames"], s["depth"], s["population"], s["generations"], s["elite"], s["plan_seed"], s["mutation"], s["init"], hold=s["hold"],
                                objective=s["objective"], rest=s["rest"])
    assert per_env and args.shape == (n, 15)
    before = _snapshot(g)
    assert_search_equal(_search_dict(g.reduce(EVOLVE, args), n, L), want, "%s evolve rows (host form)" % game)
    assert_search_equal(_search_dict(_device_reduce(g, EVOLVE, args, 6 * L), n, L), want, "%s evolve rows (device form)" % game)
    _assert_same_snapshot(_snapshot(g), before, "%s per-env rows" % game)
    keys = ("frames", "hold", "depth", "objective", "population", "generations", "elite", "plan_seed", "mutation", "init")
    for i in good[:8]:                                        # the same envs asked alone, with shared arguments
        shared = _ask(g, {k: int(s[k][i]) for k in keys}, rest=LEGAL[game][0])
        for k in SEARCH_FIELDS:
            assert np.array_equal(np.asarray(shared[k][i], np.float64), np.asarray(want[k][i], np.float64)), (game, i, k)


# ---------------------------------------------------------------- 5. forms

def _evolve_against_replay(g, game, oracle_lib, what):
    states, rngs = g.get_states(), sim_rngs(g)
    ev = dict(frames=48, hold=4, depth=5, population=9, generations=2, elite=2, mutation=80, plan_seed=21, rest=LEGAL[game][2])
    for o, objective in enumerate(OBJECTIVES):
        want, gens = expected_evolve(oracle_lib, game, states, rngs, dict(ev, objective=o))
        assert_search_equal(_ask(g, ev, objective=objective), want, "%s evolve %s" % (what, objective))
    return gens


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
    gens = _evolve_against_replay(g, game, oracle_lib, "%s written states" % game)
    assert any((gen["ret"] > 0).any() for gen in gens)
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
    _evolve_against_replay(g, "breakout", oracle_lib, "breakout, wave per env")
    g.close(); o.close()


@pytest.mark.parametrize("game", GAMES)
def test_the_device_form_on_a_callers_stream_is_the_host_form(game, hip_lib, oracle_lib):
    n, L = 24, len(LEGAL[game])
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    args, _ = evolve_args(game, n, 40, np.full(n, 6), 7, 2, 2, 3, 100, hold=4, objective=1, rest=LEGAL[game][0], seed=5, t=1, env_offset=9)
    host = g.reduce(EVOLVE, args)
    assert np.array_equal(_device_reduce(g, EVOLVE, args, 6 * L), host) and (host.reshape(n, L, 6)[..., 3] > 0).all()


@pytest.mark.parametrize("cls", ["ToyboxVecEnv", "ToyboxPreprocVecEnv"])
def test_the_adapters(cls, hip_lib, oracle_lib):
    """evolve_search: (agent) steps, action indices, the engine's rows and the winner among an env's rows; best_plan fed back as
    init_plan with one individual and no generation reproduces best_action's row; the next observation is untouched"""
    from toybox_amd import envs
    game, n, depth = "space_invaders", 24, 5
    L = len(LEGAL[game])
    v, twin = (getattr(envs, cls)(game, n, seed=3, engine=Engine(game, n, lib=hip_lib)) for _ in range(2))
    rng = np.random.default_rng(0)
    for e in (v, twin):
        e.reset()
    for _ in range(20):
        a = rng.integers(0, v.action_space.n, n)
        v.step(a); twin.step(a)
    skip = getattr(v, "_skip", 1) if cls == "ToyboxPreprocVecEnv" else 1
    a = rng.integers(0, v.action_space.n, n)
    v.step_async(a); twin.step_async(a); twin.step_wait()     # a pending step ends first
    for o, objective in enumerate(OBJECTIVES):
        got = v.evolve_search(12, depth, 9, 2, elite=2, mutation=80, plan_seed=4, objective=objective, rest=0)
        assert v._in_flight is None and getattr(v, "_pending", None) is None
        ev = dict(frames=12 * skip, hold=skip, depth=depth, population=9, generations=2, elite=2, mutation=80, plan_seed=4, rest=LEGAL[game][0])
        want, _ = expected_evolve(oracle_lib, game, v.engine.get_states(), sim_rngs(v.engine), dict(ev, objective=o))
        assert_search_equal(got, want, "%s.evolve_search %s" % (cls, objective))
        digits = np.stack([want["code"] // L ** p % L for p in range(depth)], axis=-1)
        assert np.array_equal(got["plan"], digits)
        best = pick_rows(want, o)
        assert np.array_equal(got["best_action"], best) and np.array_equal(got["best_plan"], got["plan"][np.arange(n), best])
        assert np.array_equal(got["best_plan"][:, 0], got["best_action"]), "the first digit of the best plan is the best action"
        again = v.evolve_search(12, depth, 1, 0, init_plan=got["best_plan"], objective=objective, rest=0)
        for k in SEARCH_FIELDS:
            assert np.array_equal(again[k][np.arange(n), best], got[k][np.arange(n), best]), (cls, objective, k)
        shared = v.evolve_search(12, depth, 1, 0, init_plan=got["best_plan"][0], objective=objective, rest=0)
        assert all(again[k][0, best[0]] == shared[k][0, best[0]] for k in SEARCH_FIELDS)
    a = rng.integers(0, v.action_space.n, n)
    for x, y in zip(v.step(a)[:3], twin.step(a)[:3]):
        assert np.array_equal(np.asarray(x), np.asarray(y)), "%s: the step after the queries differs from an untouched twin's" % cls
    v.close(); twin.close()


def test_batch_intervention_mirrors_the_engine(hip_lib, oracle_lib):
    from toybox_amd.interventions import BatchIntervention
    game, n, first, count = "breakout", 24, 5, 11
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    depth, population = np.resize([7, 2, 5], n), np.resize([6, 3], n)
    whole = g.lookahead_evolve(48, depth, population, 2, hold=4, objective="survival", rest=0, plan_seed=8)
    with BatchIntervention(g, first, count) as bi:
        part = bi.lookahead_evolve(48, depth[first:first + count], population[first:first + count], 2, hold=4, objective="survival", rest=0, plan_seed=8)
        sole = bi.lookahead_evolve(48, 7, 6, 2, hold=4, objective="survival", rest=0, plan_seed=8)
    for k in SEARCH_FIELDS:
        assert np.array_equal(part[k], whole[k][first:first + count]), k
    same = np.flatnonzero((depth[first:first + count] == 7) & (population[first:first + count] == 6))
    assert len(same) and all(np.array_equal(sole[k][same], part[k][same]) for k in SEARCH_FIELDS) and (whole["frames_run"] > 0).all()


# ---------------------------------------------------------------- 6. nothing written

@pytest.mark.parametrize("game", GAMES)
def test_the_query_leaves_the_engine_untouched(game, hip_lib, oracle_lib):
    """state records, simulator RNGs, step outputs and scalars are byte-equal before and after a query of several ranges and
    generations, a checkpoint store keeps what it held, and the next synthetic step gives what an untouched twin gives"""
    n = 24
    g, twin = batch(hip_lib, game, n), batch(hip_lib, game, n)
    g.checkpoint_slots(1)
    g.checkpoint_save(0)
    saved = bytes(g.get_states())
    g.step_synthetic(1337, 399, auto_reset=True); twin.step_synthetic(1337, 399, auto_reset=True)
    before = _snapshot(g)
    g.beam_range_envs = 7
    g.lookahead_evolve(40, 7, 12, 3, hold=4, objective="survival", rest=LEGAL[game][0])
    assert g.evolve_ranges == 4
    g.beam_range_envs = 0
    _assert_same_snapshot(_snapshot(g), before, game)
    assert (g.checkpoint_valid(0) == 1).all()
    for e in (g, twin):
        e.step_synthetic(1337, 400, auto_reset=True)
    _assert_same_snapshot(_snapshot(g), _snapshot(twin), "%s: the step after the query" % game)
    g.checkpoint_restore(0)
    assert bytes(g.get_states()) == saved, "%s: the checkpoint store changed" % game
    g.close(); twin.close()


@pytest.mark.parametrize("game", GAMES)
def test_the_query_leaves_the_agent_layer_untouched(game, hip_lib, oracle_lib):
    n = 16
    case = Agent(game, n)
    g, o = case.make(hip_lib), case.make(oracle_lib)
    case.run(g, 0, 12); case.run(o, 0, 12)
    obs, before = read_buffer(g, _abi.BUF_AGENT_OBS, (n, 84, 84, 4)), _snapshot(g)
    ev = dict(frames=24, hold=4, depth=4, population=6, generations=2, elite=2, mutation=90, plan_seed=1, seed=11, t=12)
    got = _ask(g, ev)
    assert np.array_equal(read_buffer(g, _abi.BUF_AGENT_OBS, (n, 84, 84, 4)), obs), "TBX_BUF_AGENT_OBS changed"
    _assert_same_snapshot(_snapshot(g), before, "%s with the agent layer" % game)
    assert_search_equal(got, expected_evolve(oracle_lib, game, g.get_states(), sim_rngs(g), ev)[0], "%s with the agent layer on: raw frames from the state as it stands" % game)
    rows_g, rows_o = case.run(g, 12, 16), case.run(o, 12, 16)
    for x, y in zip(rows_g, rows_o):
        for u, w in zip(x, y):
            assert np.array_equal(u, w), "%s: the agent steps after the query" % game
    g.close(); o.close()


# ---------------------------------------------------------------- 7. shared refusals

@pytest.mark.parametrize("game", GAMES)
def test_shared_refusals(game, hip_lib, oracle_lib):
    """TBX_E_INVALID before anything is launched: the message names the value, TBX_OPT_EVOLVE_RANGES stands, a caller's output buffer
    keeps its bytes"""
    from toybox_amd import hip
    n = 24
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    illegal = 2 if game == "breakout" else 17
    g.lookahead_evolve(8, 2, 2, 1)
    ranges, before = g.evolve_ranges, _snapshot(g)
    tail = [8, 1, 2, 0, -1, 0, 0, 0, 0]
    bad = {"depth": [[8, 1, 0], [8, 1, top + 1]], "objective": [[8, 1, 2, 2]], "rest": [[8, 1, 2, 0, illegal]], "frames": [[0], [1025]], "hold": [[8, 0]],
           "population": [tail + [0], tail + [257]], "generations": [tail + [4, -1], tail + [4, 65]], "elite": [tail + [4, 1, 0], tail + [4, 1, 5]],
           "plan_seed": [tail + [4, 1, 1, -1], tail + [4, 1, 1, 2 ** 32]], "mutation": [tail + [4, 1, 1, 0, -1], tail + [4, 1, 1, 0, 257]],
           "init": [tail + [4, 1, 1, 0, 64, -2], tail + [4, 1, 1, 0, 64, L * L]], "evolve takes": [tail + [4, 1, 1, 0, 64, -1, 0], []]}
    pattern = np.arange(n * 6 * L, dtype=np.float64) + 0.5
    o_dev = hip.malloc(pattern.nbytes)
    g.beam_range_envs = 5
    try:
        hip.memcpy_htod(o_dev, pattern, pattern.nbytes)
        for name, rows in bad.items():
            for args in rows:
                with pytest.raises(ToyboxAmdError) as ei:
                    g.reduce(EVOLVE, args)
                assert ei.value.code == _abi.E_INVALID and name in str(ei.value), (name, args, str(ei.value))
                if args:
                    with pytest.raises(ToyboxAmdError) as ei:
                        g.reduce_device(EVOLVE, o_dev, args)
                    assert ei.value.code == _abi.E_INVALID and name in str(ei.value), (name, args, str(ei.value))
                assert g.evolve_ranges == ranges, "a refusal leaves TBX_OPT_EVOLVE_RANGES standing"
        g.sync()
        back = np.empty_like(pattern)
        hip.memcpy_dtoh(back, o_dev, back.nbytes)
        assert np.array_equal(back, pattern), "a refused query wrote into the output buffer"
    finally:
        g.beam_range_envs = 0
        g.sync()
        hip.free(o_dev)
    _assert_same_snapshot(_snapshot(g), before, "%s after the refusals" % game)
    # the largest query there is: the deepest plans, the largest population, every generation
    assert g.reduce(EVOLVE, [8, 1, top, 1, -1, 0, 0, 0, 0, 256, 64, 256, 2 ** 32 - 1, 256, L ** top - 1]).shape == (n, 6 * L)
    with pytest.raises(ToyboxAmdError):
        g.set_option(_abi.OPT_EVOLVE_RANGES, 1)
    for name in GAMES:
        assert hip_lib.tbx_reduce_width(_abi.GAME_IDS[name], EVOLVE) == 6 * len(LEGAL[name])
