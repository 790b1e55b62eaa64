"""The search over sampled futures on the device (TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES, include/toybox_amd.h) against SALT, PLAY ALL
CODES AND PICK on the CPU checker (tests/search_samples_replay.py; its own checks are in tests/test_search_samples.py).  Every
comparison is exact, on every field of every (env, first action) row.

The engine under test is made by the input recipe of tests/lookahead_replay.py and held to its checker twin byte for byte before any
query (the worlds of tests/test_gpu_search.py, shared with it); the plans of a case are played on clones of the records the DEVICE
engine reports, once per (case, rest), and shared by both objectives.  Every case runs with rest "fixed" (the game's second legal
action, seed 77) and "drawn" (rest -1, a seed above 32 bits, t = 2^32 - 3, env offset 70 000).

Measured on the checker alone (seconds to replay fixed / drawn, 16 checker threads on a small CPU-only box that has fewer cores;
on an MI355X host the same replays take 0.3 - 1.1 s each and the whole module 8 s) and counted on the EXPECTED arrays -- groups whose
winner is not their smallest code / groups won on the code tie-break / groups where the objectives pick different plans / plans
whose futures differ in their return / groups whose winner under the S futures is not their winner under future 0 alone, fixed +
drawn, out of the case's groups:
  breakout-deep   24 envs x 96 frames x hold 8 x depth 3 x 4 samples          21 s / 27 s   13 + 16 / 91 + 89 / 0 + 0 / 0 + 6 / 0 + 8 of 96
  breakout-wide   96 x 96 x 8 x depth 2 x 8                                   12 s / 5 s    47 + 72 / 337 + 314 / 0 + 1 / 0 + 52 / 0 + 47 of 384
  space_invaders  12 x 96 x 8 x depth 2 x 5, salt 1000                        4 s / 9 s     40 + 39 / 52 + 51 / 28 + 15 / 82 + 306 / 21 + 29 of 72
  amidar          24 x 96 x 4 x depth 2 x 4                                   9 s / 5 s     17 + 35 / 127 + 109 / 0 + 6 / 0 + 184 / 0 + 21 of 144
  gridworld       24 x 24 x 2 x depth 3 x 3                                   6 s / 3 s     6 + 62 / 115 + 79 / 0 + 1 / 0 + 409 / 0 + 28 of 120
(on the small box the deep Breakout case is above ten seconds: 64 codes x 4 samples are 256 clones of 96 frames each).
Under fixed actions and an unsalted RNG the S futures of a plan are one future: those columns are 0 by construction; SpaceInvaders
is salted in both."""
import functools

import numpy as np
import pytest

from fork_replay import sim_rngs
from lookahead_replay import batch
from sample_replay import LEAF_FIELDS
from sample_replay import aggregate as aggregate_samples
from search_samples_replay import (BIG_SEED, BIG_T, CASES, ENV_OFFSET, RESTS, ROW_FIELDS, aggregate, assert_rows_equal, case_args, expected_search_samples, group_stats,
                                   pick, play_all)
from support import LEGAL
from test_gpu_custom_states import _engines, _write_all, fuzz_seed, generate  # noqa: F401  (fuzz_seed: the fixture)
from test_gpu_search import _assert_same_snapshot, _device_reduce, _held_to_twin, _snapshot, _world
from toybox_amd import ToyboxAmdError, _abi
from toybox_amd.engine import SAMPLE_FIELDS, Engine, plan_actions, plan_args, sample_seed, search_samples_args

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
OBJECTIVES = ["return", "survival"]
QUERY = _abi.QUERY_LOOKAHEAD_SEARCH_SAMPLES


def _case_world(name, hip_lib, oracle_lib):
    game, n = CASES[name][:2]
    return _world(game, n, CASES[name][7], hip_lib, oracle_lib)


@functools.lru_cache(maxsize=None)
def _played(name, rest, hip_lib, oracle_lib):
    _, states, rngs = _case_world(name, hip_lib, oracle_lib)
    leaves, active, ok, depth = play_all(oracle_lib, CASES[name][0], states, rngs, case_args(name, rest))
    for v in leaves.values():
        v.flags.writeable = False
    return leaves, active, ok, depth


def _ask(g, case, objective):
    c = dict(case)
    if c.get("rest") == -1:
        c["rest"] = None
    return g.lookahead_search_samples(c.pop("frames"), c.pop("depth"), c.pop("samples"), objective=objective, **c)


# ---------------------------------------------------------------- 1. the device == every plan replayed on every future, summed, picked

@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("rest", RESTS)
@pytest.mark.parametrize("name", list(CASES))
def test_rows_equal_replay(name, rest, objective, hip_lib, oracle_lib):
    game, n, _, _, depth, samples = CASES[name][:6]
    L = len(LEGAL[game])
    g, _, _ = _case_world(name, hip_lib, oracle_lib)
    leaves, active, ok, d = _played(name, rest, hip_lib, oracle_lib)
    assert ok.all()
    want = pick(game, aggregate(leaves, active), ok, d, OBJECTIVES.index(objective))
    got = _ask(g, case_args(name, rest), objective)
    assert all(got[k].shape == (n, L) and got[k].dtype == np.int64 for k in SAMPLE_FIELDS) and (got["samples"] == samples).all()
    assert got["code"].dtype == np.uint64 and got["plan"].shape == (n, L, depth)
    assert_rows_equal(got, want, "%s %s %s" % (name, rest, objective))
    assert np.array_equal(got["plan"], plan_actions(game, want["code"], depth)) and np.array_equal(got["plan"][:, :, 0], np.tile(LEGAL[game], (n, 1)))
    assert g.reduce_width(QUERY) == 9 * L and g.search_samples_launches == 1
    if name == "breakout-deep":
        assert g.search_samples_chunks > 1, "16 suffix codes over 96 groups of a thread each: this case is the chunked one"


@pytest.mark.parametrize("game", GAMES)
def test_the_cases_cover_what_they_must(game, hip_lib, oracle_lib):
    """asserted on the expected arrays, so no test passes by avoiding the hard rows"""
    total = {}
    for name in CASES:
        if CASES[name][0] == game:
            for rest in RESTS:
                for k, v in group_stats(game, *_played(name, rest, hip_lib, oracle_lib)).items():
                    total[k] = total.get(k, 0) + int(v)
    need = ["winner_not_first", "ties", "spread_plans"] + ([] if game == "gridworld" else ["disagree"]) + (["future0_differs"] if game in ("space_invaders", "breakout") else [])
    missing = [k for k in need if not total[k]]
    assert not missing, "%s: the cases together never show: %s (%r)" % (game, ", ".join(missing), total)


# ---------------------------------------------------------------- 2. the device == itself

@pytest.mark.parametrize("game", GAMES)
def test_depth_1_is_the_sampled_lookahead(game, hip_lib, oracle_lib):
    name = "breakout-wide" if game == "breakout" else game
    g, _, _ = _case_world(name, hip_lib, oracle_lib)
    n, frames, hold = CASES[name][1:4]
    kw = dict(hold=hold, salt=1000, seed=(7 << 33) | 5, t=2 ** 32 - 2, env_offset=99)
    want = g.lookahead_samples(frames, 6, **kw)
    for objective in OBJECTIVES:
        got = g.lookahead_search_samples(frames, 1, 6, objective=objective, **kw)
        for k in SAMPLE_FIELDS:
            assert np.array_equal(got[k], want[k]), (game, objective, k)
        assert np.array_equal(got["code"], np.tile(np.arange(len(LEGAL[game]), dtype=np.uint64), (n, 1)))


@pytest.mark.parametrize("name", [k for k in CASES if CASES[k][6] == 0])
def test_every_returned_code_reproduces_its_row_from_plan_calls(name, hip_lib, oracle_lib):
    """salt 0: future s of a plan is TBX_QUERY_LOOKAHEAD_PLAN under sample_seed(seed, s), so S plan calls per first action, summed
    on the host, are the row"""
    game, n, frames, hold, depth, samples = CASES[name][:6]
    g, _, _ = _case_world(name, hip_lib, oracle_lib)
    c = case_args(name, "drawn")
    for objective in OBJECTIVES:
        res = _ask(g, c, objective)
        for a in range(len(LEGAL[game])):
            calls = []
            for s in range(samples):
                args, _ = plan_args(game, n, frames, hold=hold, depth=depth, code=res["code"][:, a], rest=None, seed=sample_seed(c["seed"], s), t=c["t"], env_offset=c["env_offset"])
                calls.append(Engine._lookahead_dict(g.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args)))
            leaves = {k: np.stack([np.asarray(x[k]).astype(np.int64)[:, None] for x in calls]) for k in LEAF_FIELDS}
            sums = aggregate_samples(leaves, np.ones((samples, n), bool))
            for k in SAMPLE_FIELDS:
                assert np.array_equal(sums[k][:, 0], res[k][:, a]), (name, objective, a, k)


# ---------------------------------------------------------------- 3. per-env rows, tbx_reduce_device on a caller's stream

def _mixed_rows(game, n):
    """four kinds of row, env i of kind i % 4: mixed depths, sample counts, salts, objectives and holds; the rest shared"""
    deep = 3 if len(LEGAL[game]) <= 5 else 2
    kinds = [dict(depth=1, samples=3, salt=0, objective=0, hold=4), dict(depth=2, samples=2, salt=1000, objective=1, hold=2),
             dict(depth=deep, samples=1, salt=5, objective=0, hold=8), dict(depth=2, samples=4, salt=0, objective=1, hold=4)]
    rows = {k: np.array([kinds[i % 4][k] for i in range(n)], np.int64) for k in kinds[0]}
    rows.update(frames=np.full(n, 24), rest=np.full(n, -1), seed=(0xC0FFEE << 32) | 0x5EED, t=2 ** 32 - 2, env_offset=99)
    return kinds, rows


@pytest.mark.parametrize("game", GAMES)
def test_per_env_rows_with_bad_rows_among_them(game, hip_lib, oracle_lib):
    """mixed depths and sample counts; a row refused for each reason answers zeros and the others are answered; per-env rows are
    budgeted as the largest valid row (65 536 leaves x 1 024 frames = 2^26 leaf-frames per env), so these small batches already take
    several launches (Breakout, a thread per unit, 64 envs per launch: 96 envs; the others 2 to 16 per launch: 24 envs); the rows are
    the replay's and the same envs' rows asked one kind at a time with shared arguments"""
    n = 96 if game == "breakout" else 24
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    too_deep = {4: 7, 5: 6, 6: 5}[L]
    g, states, rngs = _world(game, n, 40 if game == "gridworld" else 400, hip_lib, oracle_lib)
    kinds, rows = _mixed_rows(game, n)
    rows["depth"][[1, 2, 3]] = [0, too_deep, top + 1]
    rows["objective"][[5, 6]] = [2, -1]
    rows["rest"][8] = 2 if game == "breakout" else 17
    rows["frames"][[10, 11]] = [0, 1025]
    rows["hold"][13] = 0
    rows["samples"][[14, 15]] = [0, 4097]
    rows["depth"][17], rows["samples"][17] = too_deep - 1, 64  # the most plans a search may have, x 64 samples: above TBX_LOOKAHEAD_MAX_LEAVES
    rows["salt"][[18, 19, 20]] = [-1, 2 ** 32 - 2, 2 ** 32]
    rows["samples"][19] = 3                                    # (2^32 - 2) + 3 - 1 = 2^32: one too many
    bad = [1, 2, 3, 5, 6, 8, 10, 11, 13, 14, 15, 17, 18, 19, 20]
    good = np.setdiff1d(np.arange(n), bad)
    want = expected_search_samples(oracle_lib, game, states, rngs, rows)
    assert all((want[k][bad] == 0).all() for k in ROW_FIELDS) and np.array_equal(want["samples"][good, 0], rows["samples"][good])
    args, per_env = search_samples_args(game, n, **rows)
    assert per_env and args.shape == (n, 11)
    dev = g._search_samples_dict(_device_reduce(g, QUERY, args, 9 * L).reshape(n, L, 9), rows["depth"])
    assert g.search_samples_launches > 1, "per-env rows: %d envs cross a launch seam" % n
    assert_rows_equal(dev, want, "%s per-env rows (device form)" % game)
    host = g._search_samples_dict(g.reduce(QUERY, args).reshape(n, L, 9), rows["depth"])
    assert_rows_equal(host, want, "%s per-env rows (host form)" % game)
    for j, kind in enumerate(kinds):
        shared = g.lookahead_search_samples(24, kind["depth"], kind["samples"], hold=kind["hold"], objective=kind["objective"], salt=kind["salt"], rest=None,
                                            seed=rows["seed"], t=rows["t"], env_offset=rows["env_offset"])
        mine = good[good % 4 == j]
        assert len(mine) >= 1
        for k in ROW_FIELDS:
            assert np.array_equal(shared[k][mine], dev[k][mine]), (game, j, k)


# ---------------------------------------------------------------- 4. forms

def _both_objectives_against_replay(g, game, oracle_lib, what, frames=64, hold=4, depth=2, samples=3):
    states, rngs = g.get_states(), sim_rngs(g)
    case = dict(frames=frames, hold=hold, depth=depth, samples=samples, salt=1000, rest=-1, seed=BIG_SEED, t=BIG_T, env_offset=ENV_OFFSET)
    leaves, active, ok, d = play_all(oracle_lib, game, states, rngs, case)
    for objective in OBJECTIVES:
        assert_rows_equal(_ask(g, case, objective), pick(game, aggregate(leaves, active), ok, d, OBJECTIVES.index(objective)), "%s %s" % (what, objective))
    return aggregate(leaves, active)


@pytest.mark.parametrize("game", ["breakout", "space_invaders"])
def test_written_states(game, fuzz_seed, hip_lib, oracle_lib):
    """a Breakout batch after custom bricks were written (it has left the canonical wall: the wave form with per-env brick tables)
    and a SpaceInvaders batch off the formation grid (the full load), built the way tests/test_gpu_custom_states.py builds them"""
    n = 16
    es = g, o = _engines(game, n, (hip_lib, oracle_lib))
    _write_all(es, generate(game, o, np.random.default_rng(fuzz_seed)))
    for e in es:
        for t in range(20):
            e.step_synthetic(1337, t, auto_reset=True)
    _held_to_twin(g, o, "%s written states" % game)
    sums = _both_objectives_against_replay(g, game, oracle_lib, "%s written states" % game)
    assert (sums["ret_max"] > 0).any() and (sums["ret_min"] < sums["ret_max"]).any()
    _held_to_twin(g, o, "%s written states after the queries" % game)
    g.close(); o.close()


def test_breakout_wave_per_env_step_form(hip_lib, oracle_lib):
    """TBX_OPT_STEP_FORM = 2: the canonical wall through the wave form"""
    n = 16
    g = Engine("breakout", n, lib=hip_lib)
    g.set_option(_abi.OPT_STEP_FORM, _abi.STEP_FORM_WAVE_PER_ENV)
    o = batch(oracle_lib, "breakout", n)
    g.set_states(0, o.get_states())
    for i, r in enumerate(sim_rngs(o)):
        g.set_sim_rng((int(r[0]), int(r[1])), env=i)
    _held_to_twin(g, o, "breakout, wave per env")
    sums = _both_objectives_against_replay(g, "breakout", oracle_lib, "breakout, wave per env", frames=96, hold=8)
    assert (sums["lost"] > 0).any() and (sums["ended"] > 0).any()
    g.close(); o.close()


def test_batch_intervention_mirrors_the_engine(hip_lib, oracle_lib):
    from toybox_amd.interventions import BatchIntervention
    game, n, first, count = "breakout", 24, 5, 11
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    whole = g.lookahead_search_samples(48, 2, 3, hold=4, objective="survival", salt=9, rest=0)
    with BatchIntervention(g, first, count) as bi:
        part = bi.lookahead_search_samples(48, 2, 3, hold=4, objective="survival", salt=9, rest=0)
    for k in ROW_FIELDS + ("plan",):
        assert np.array_equal(part[k], whole[k][first:first + count]), k


# ---------------------------------------------------------------- 5. nothing written

@pytest.mark.parametrize("game", GAMES)
def test_the_query_leaves_the_engine_untouched(game, hip_lib, oracle_lib):
    """state records, simulator RNGs, step outputs and scalars are byte-equal before and after the query -- chunked, its partial
    rows in a scratch of the engine's, and salted -- and the next synthetic step gives what an untouched twin gives"""
    n = 24
    g, twin = batch(hip_lib, game, n), batch(hip_lib, game, n)
    before = _snapshot(g)
    g.lookahead_search_samples(40, 3 if len(LEGAL[game]) <= 5 else 2, 3, hold=4, objective="survival", salt=7)
    assert g.search_samples_chunks > 1
    _assert_same_snapshot(_snapshot(g), before, game)
    for e in (g, twin):
        e.step_synthetic(1337, 400, auto_reset=True)
    _assert_same_snapshot(_snapshot(g), _snapshot(twin), "%s: the step after the query" % game)
    g.close(); twin.close()


# ---------------------------------------------------------------- 6. refusals

@pytest.mark.parametrize("game", GAMES)
def test_shared_refusals(game, hip_lib, oracle_lib):
    """TBX_E_INVALID with a message that names the argument, nothing launched (the chunk and launch counters of the last call
    stand), nothing changed"""
    g, _, _ = _world(game, 24, 40 if game == "gridworld" else 400, hip_lib, oracle_lib)
    L = len(LEGAL[game])
    illegal = 2 if game == "breakout" else 17
    too_deep = {4: 7, 5: 6, 6: 5}[L]
    assert g.lookahead_search_samples(8, 1, 1)["samples"].shape == (24, L)
    counters = (g.search_samples_chunks, g.search_samples_launches)
    before = _snapshot(g)
    tail = [-1, 0, 0, 0, 0]
    bad = {"frames 0": ([0], "frames"), "frames 1025": ([1025], "frames"), "hold 0": ([8, 0], "hold"), "depth 0": ([8, 1, 0], "depth"),
           "too many plans": ([8, 1, too_deep], "depth"), "objective 2": ([8, 1, 2, 2], "objective"), "illegal rest": ([8, 1, 2, 0, illegal], "rest"),
           "samples 0": ([8, 1, 2, 0] + tail + [0], "samples"), "samples 4097": ([8, 1, 2, 0] + tail + [4097], "samples"),
           "too many leaves": ([8, 1, too_deep - 1, 0] + tail + [64], "TBX_LOOKAHEAD_MAX_LEAVES"), "salt -1": ([8, 1, 2, 0] + tail + [2, -1], "salt"),
           "salt 2^32": ([8, 1, 2, 0] + tail + [2, 2 ** 32], "salt"), "salt + samples": ([8, 1, 2, 0] + tail + [3, 2 ** 32 - 2], "salt"),
           "twelve arguments": ([8, 1, 2, 0] + tail + [2, 0, 0], "samples, salt]"), "no arguments": ([], "samples, salt]")}
    for what, (args, word) in bad.items():
        with pytest.raises(ToyboxAmdError) as ei:
            g.reduce(QUERY, args)
        assert ei.value.code == _abi.E_INVALID and word in str(ei.value), (what, str(ei.value))
        assert (g.search_samples_chunks, g.search_samples_launches) == counters, what
    _assert_same_snapshot(_snapshot(g), before, "%s after the refusals" % game)
    assert g.reduce(QUERY, [8, 1, too_deep - 1]).shape == (24, 9 * L)                          # the deepest search, one sample
    cap = 65536 // L ** 2
    if cap * L ** 2 == 65536:
        assert (g.reduce(QUERY, [8, 1, 2, 0] + tail + [cap]).reshape(24, L, 9)[..., 0] == cap).all()   # exactly TBX_LOOKAHEAD_MAX_LEAVES
    for name in GAMES:
        assert hip_lib.tbx_reduce_width(_abi.GAME_IDS[name], QUERY) == 9 * len(LEGAL[name])
