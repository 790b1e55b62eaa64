"""Plans and the search on the device (TBX_QUERY_LOOKAHEAD_PLAN / _SEARCH, include/toybox_amd.h) against CLONE AND PLAY on the
CPU checker (tests/search_replay.py; its own checks are in tests/test_search.py).  Every comparison is exact, on every field of
every env.

The engine under test is made by the input recipe of tests/lookahead_replay.py and held to its checker twin byte for byte before any
query; the expected rows are played on clones of the records the DEVICE engine reports.  The leaves of a case are played once and
shared by both objectives.  Measured on the checker for the first case of every game (tests/test_search.py prints them), with
rest = the first legal action -- groups whose winner is not their smallest code / groups won on the tie-break / groups where the
objectives disagree / envs with an ended leaf: Breakout (96, 200, 8, 3) 110 of 384 / 349 / 4 / 80; SpaceInvaders (24, 96, 8, 2)
31 / 127 / 7 / 9; Amidar (96, 128, 4, 2, batch 900) 40 / 536 / 4 / 3; GridWorld (96, 40, 2, 4, batch 40) 119 / 406 / 0 / 0."""
import functools

import numpy as np
import pytest

from fork_replay import Agent, sim_rngs, states_bytes
from lookahead_replay import FIELDS, assert_fields_equal, batch, clone
from search_replay import (DRAWN_CASE, SEARCH_CASES, SEARCH_FIELDS, assert_search_equal, case_search, expected_plan, expected_search, group_stats, pick,
                           play_all_codes)
from support import LEGAL, read_buffer
from test_gpu_custom_states import _engines, _write_all, fuzz_seed, generate  # noqa: F401  (fuzz_seed: the fixture)
from toybox_amd import ToyboxAmdError, _abi
from toybox_amd.engine import Engine, plan_actions, plan_args, search_args

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
OBJECTIVES = ["return", "survival"]
STEP_BUFFERS = ((_abi.BUF_REWARD, np.int32), (_abi.BUF_DONE, np.uint8), (_abi.BUF_LIVES, np.int32), (_abi.BUF_SCORE, np.int32), (_abi.BUF_PACKED, np.uint64))
CASES = [(game, case) for game in GAMES for case in SEARCH_CASES[game]]
_WORLDS = {}


def _held_to_twin(g, o, what):
    assert np.array_equal(states_bytes(g), states_bytes(o)), "%s: the device engine's state records are not its checker twin's" % what
    assert np.array_equal(sim_rngs(g), sim_rngs(o)), "%s: simulator RNGs differ from the checker twin's" % what


def _world(game, n, batch_frames, hip_lib, oracle_lib):
    """(device engine, its state records, its simulator RNGs) of the input recipe, made once and only ever queried"""
    key = (game, n, batch_frames)
    if key not in _WORLDS:
        g, o = batch(hip_lib, game, n, frames=batch_frames), batch(oracle_lib, game, n, frames=batch_frames)
        _held_to_twin(g, o, "%s n=%d" % (game, n))
        o.close()
        _WORLDS[key] = (g, g.get_states(), sim_rngs(g))
    return _WORLDS[key]


@functools.lru_cache(maxsize=None)
def _leaves(game, case, hip_lib, oracle_lib):
    _, states, rngs = _world(game, case[0], case[4], hip_lib, oracle_lib)
    leaves, ok, depth = play_all_codes(oracle_lib, game, states, rngs, case_search(game, case))
    for v in leaves.values():
        v.flags.writeable = False
    return leaves, ok, depth


def _search_dict(rows, n, L):
    """float64 [n, 6 L] as tbx_reduce returns it -> the five named fields and the code, each [n, L]"""
    rows = np.asarray(rows).reshape(n, L, 6)
    out = Engine._lookahead_dict(rows[..., :5])
    out["code"] = rows[..., 5].astype(np.int64)
    return out


def _snapshot(g):
    return (states_bytes(g), sim_rngs(g)) + tuple(read_buffer(g, b, (g.n_envs,), dt) for b, dt in STEP_BUFFERS) + tuple(g.scalars())


def _assert_same_snapshot(a, b, what):
    names = ("state records", "simulator RNGs", "reward", "done", "lives", "score", "packed", "scalar score", "scalar lives", "scalar level", "scalar over")
    for name, x, y in zip(names, a, b):
        assert np.array_equal(x, y), "%s: %s changed" % (what, name)


def _device_reduce(g, query, args, width):
    """tbx_reduce_device on a caller's stream with the per-env rows in HBM"""
    from toybox_amd import hip
    n = g.n_envs
    s = hip.Stream()
    a_dev, o_dev = hip.malloc(args.nbytes), hip.malloc(n * width * 8)
    try:
        hip.memcpy_htod(a_dev, args, args.nbytes)
        g.reduce_device(query, o_dev, stream=s.ptr, per_env_ptr=a_dev, n_args=args.shape[1])
        s.synchronize()
        rows = np.empty((n, width), np.float64)
        hip.memcpy_dtoh(rows, o_dev, rows.nbytes)
    finally:
        g.sync()
        hip.free(a_dev)
        hip.free(o_dev)
        s.close()
    return rows


# ---------------------------------------------------------------- 1. the search == all codes replayed, then picked

@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("game,case", CASES, ids=["%s-%d-%d-%d-%d" % ((g,) + c[:4]) for g, c in CASES])
def test_search_equals_replay(game, case, objective, hip_lib, oracle_lib):
    n, frames, hold, depth, batch_frames = case
    L = len(LEGAL[game])
    g, _, _ = _world(game, n, batch_frames, hip_lib, oracle_lib)
    want = pick(game, *_leaves(game, case, hip_lib, oracle_lib), OBJECTIVES.index(objective))
    got = g.lookahead_search(frames, depth, hold=hold, objective=objective, rest=LEGAL[game][0])
    assert got["ret"].shape == (n, L) and got["ret"].dtype == np.float64 and got["code"].dtype == np.uint64 and got["plan"].shape == (n, L, depth)
    assert_search_equal(got, want, "%s %r %s" % (game, case, objective))
    assert np.array_equal(got["plan"], plan_actions(game, want["code"], depth)) and np.array_equal(got["plan"][:, :, 0], np.tile(LEGAL[game], (n, 1)))
    assert g.reduce_width(_abi.QUERY_LOOKAHEAD_SEARCH) == 6 * L and g.reduce_width(_abi.QUERY_LOOKAHEAD_PLAN) == 5
    if (game, depth) == ("breakout", 4):
        assert g.search_chunks > 1, "256 leaves over 24 envs: this case is the chunked one"


@pytest.mark.parametrize("game", GAMES)
def test_search_with_drawn_rest_actions(game, hip_lib, oracle_lib):
    """rest = -1: the synthetic rule with a seed above 32 bits, a counter that leaves 32 bits and an env offset"""
    c = dict(DRAWN_CASE)
    n, batch_frames = c.pop("n"), c.pop("batch_frames")
    g, states, rngs = _world(game, n, batch_frames, hip_lib, oracle_lib)
    leaves, ok, depth = play_all_codes(oracle_lib, game, states, rngs, c)
    assert ok.all()
    for objective in reversed(OBJECTIVES):
        got = g.lookahead_search(c["frames"], c["depth"], hold=c["hold"], objective=objective, rest=None, seed=c["seed"], t=c["t"], env_offset=c["env_offset"])
        assert_search_equal(got, pick(game, leaves, ok, depth, OBJECTIVES.index(objective)), "%s drawn rest, %s" % (game, objective))
    other = g.lookahead_search(c["frames"], c["depth"], hold=c["hold"], rest=None, seed=c["seed"] ^ (1 << 40), t=c["t"], env_offset=c["env_offset"])
    assert any(not np.array_equal(other[k], got[k]) for k in FIELDS), "the upper half of the seed is not read"


@pytest.mark.parametrize("game", GAMES)
def test_the_cases_cover_what_they_must(game, hip_lib, oracle_lib):
    """asserted on the expected arrays, so no test passes by avoiding the hard rows"""
    total = {}
    for case in SEARCH_CASES[game]:
        for k, v in group_stats(game, *_leaves(game, case, hip_lib, oracle_lib)).items():
            total[k] = total.get(k, 0) + int(v)
    need = ["winner_not_first", "ties", "scored"] + ([] if game == "gridworld" else ["disagree", "ended_envs"])
    missing = [k for k in need if not total[k]]
    assert not missing, "%s: the search cases together never show: %s" % (game, ", ".join(missing))


# ---------------------------------------------------------------- 2. the answer does not depend on how the work is cut up

@pytest.mark.parametrize("game", GAMES)
def test_chunking_independence(game, hip_lib, oracle_lib):
    """8 envs replicated into an engine of 2 048: the small batch is cut into many chunks per (env, first action) group, the large
    one into fewer, and every copy's rows are the original's"""
    small, copies, depth = 8, 256, 3
    g, states, rngs = _world(game, small, 400, hip_lib, oracle_lib)
    rec = np.frombuffer(states, dtype=np.dtype(g.state_type))
    big = Engine(game, small * copies, lib=hip_lib)
    big.set_states_np(0, np.tile(rec, copies))
    for i in range(small * copies):
        big.set_sim_rng((int(rngs[i % small][0]), int(rngs[i % small][1])), env=i)
    kw = dict(hold=4, rest=LEGAL[game][0])
    a = g.lookahead_search(48, depth, **kw)
    chunks_small = g.search_chunks
    b = big.lookahead_search(48, depth, **kw)
    chunks_big = big.search_chunks
    assert chunks_small >= 1 and chunks_big >= 1 and chunks_small != chunks_big, (chunks_small, chunks_big)
    for k in SEARCH_FIELDS + ("plan",):
        assert np.array_equal(b[k], np.tile(a[k], (copies,) + (1,) * (a[k].ndim - 1))), k
    assert_search_equal(a, expected_search(oracle_lib, game, states, rngs, dict(frames=48, depth=depth, **kw)), "%s 8 envs" % game)
    big.close()


# ---------------------------------------------------------------- 3. the plan query

def _plan_rows(game, n):
    rng = np.random.default_rng(11)
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    depth = np.resize([0, 1, 5, top], n)
    code = np.array([int(rng.integers(0, L ** int(d))) for d in depth], np.int64)
    code[3] = L ** top - 1                                    # the largest code there is (Breakout: 2^32 - 1)
    legal = np.asarray(LEGAL[game] + [-1])
    return dict(frames=np.resize([1, 17, 64, 130, 200, 33, 96], n), hold=np.resize([1, 4, 7, 8, 2], n), depth=depth, code=code,
                rest=legal[rng.integers(0, len(legal), n)], seed=(0xC0FFEE << 32) | 0x5EED, t=rng.integers(0, 2 ** 32, n, dtype=np.uint64),
                env_offset=rng.integers(0, 2 ** 32, n, dtype=np.uint64))


@pytest.mark.parametrize("game", GAMES)
def test_plan_query_per_env_rows(game, hip_lib, oracle_lib):
    """random codes at depths 0, 1, 5 and TBX_PLAN_MAX_DEPTH, mixed frames and hold; the host form, and the device form on a
    caller's stream with the rows in HBM"""
    n = 96
    g, states, rngs = _world(game, n, 400, hip_lib, oracle_lib)
    rows = _plan_rows(game, n)
    want = expected_plan(oracle_lib, game, states, rngs, rows)
    assert (want["frames_run"] > 0).all() and (want["ret"] > 0).any()
    args, per_env = plan_args(game, n, **rows)
    assert per_env and args.shape == (n, 9)
    assert_fields_equal(Engine._lookahead_dict(g.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args)), want, "%s plan rows (host form)" % game)
    assert_fields_equal(Engine._lookahead_dict(_device_reduce(g, _abi.QUERY_LOOKAHEAD_PLAN, args, 5)), want, "%s plan rows (device form)" % game)
    # Engine.lookahead_plan: ALE ids [N, depth]
    L = len(LEGAL[game])
    plan = np.asarray(LEGAL[game])[np.random.default_rng(2).integers(0, L, (n, 5))]
    code = (np.searchsorted(LEGAL[game], plan) * L ** np.arange(5)).sum(axis=1)
    got = g.lookahead_plan(70, plan, hold=6, rest=LEGAL[game][1])
    assert_fields_equal(got, expected_plan(oracle_lib, game, states, rngs, dict(frames=70, hold=6, depth=5, code=code, rest=LEGAL[game][1])), "%s lookahead_plan" % game)


@pytest.mark.parametrize("game", GAMES)
def test_plan_of_depth_0_and_1_is_the_lookahead(game, hip_lib, oracle_lib):
    n = 96
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    legal = np.asarray(LEGAL[game])
    digit = np.resize(np.arange(len(legal)), n)
    sched = dict(hold=4, seed=77, t=5, env_offset=1000)
    one = g.reduce(_abi.QUERY_LOOKAHEAD_PLAN, plan_args(game, n, 120, depth=1, code=digit, **sched)[0])
    assert_fields_equal(Engine._lookahead_dict(one), g.lookahead(120, first=legal[digit], **sched), "%s depth 1 = first is legal[code]" % game)
    zero = g.reduce(_abi.QUERY_LOOKAHEAD_PLAN, plan_args(game, n, 120, depth=0, rest=legal[1], **sched)[0])
    assert_fields_equal(Engine._lookahead_dict(zero), g.lookahead(120, first=legal[1], rest=legal[1], **sched), "%s depth 0 = first is rest" % game)


@pytest.mark.parametrize("game,case", [(g, SEARCH_CASES[g][0]) for g in GAMES], ids=GAMES)
def test_every_code_the_search_returns_reproduces_its_row(game, case, hip_lib, oracle_lib):
    n, frames, hold, depth, batch_frames = case
    g, _, _ = _world(game, n, batch_frames, hip_lib, oracle_lib)
    for objective in OBJECTIVES:
        res = g.lookahead_search(frames, depth, hold=hold, objective=objective, rest=LEGAL[game][0])
        for a in range(len(LEGAL[game])):
            args, _ = plan_args(game, n, frames, hold=hold, depth=depth, code=res["code"][:, a], rest=LEGAL[game][0])
            again = Engine._lookahead_dict(g.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args))
            assert_fields_equal(again, {k: res[k][:, a] for k in FIELDS}, "%s %s first action %d" % (game, objective, a))


# ---------------------------------------------------------------- 4. forms

def _both_queries_against_replay(g, game, oracle_lib, what, frames=64, hold=4, depth=2):
    n, L = g.n_envs, len(LEGAL[game])
    states, rngs = g.get_states(), sim_rngs(g)
    rest = LEGAL[game][2]
    leaves, ok, d = play_all_codes(oracle_lib, game, states, rngs, dict(frames=frames, hold=hold, depth=depth, rest=rest))
    for objective in OBJECTIVES:
        got = g.lookahead_search(frames, depth, hold=hold, objective=objective, rest=rest)
        assert_search_equal(got, pick(game, leaves, ok, d, OBJECTIVES.index(objective)), "%s search %s" % (what, objective))
    code = np.random.default_rng(4).integers(0, L ** 5, n)
    got = Engine._lookahead_dict(g.reduce(_abi.QUERY_LOOKAHEAD_PLAN, plan_args(game, n, 90, hold=6, depth=5, code=code, seed=21)[0]))
    assert_fields_equal(got, expected_plan(oracle_lib, game, states, rngs, dict(frames=90, hold=6, depth=5, code=code, seed=21)), "%s plan" % what)
    return leaves


@pytest.mark.parametrize("game", ["breakout", "space_invaders"])
def test_written_states(game, fuzz_seed, hip_lib, oracle_lib):
    """a Breakout batch that has left the canonical wall (the wave form with per-env brick tables) and a SpaceInvaders batch off the
    formation grid (the full load), built the way tests/test_gpu_custom_states.py builds them"""
    n = 40
    es = g, o = _engines(game, n, (hip_lib, oracle_lib))
    _write_all(es, generate(game, o, np.random.default_rng(fuzz_seed)))
    for e in es:
        for t in range(20):
            e.step_synthetic(1337, t, auto_reset=True)
    _held_to_twin(g, o, "%s written states" % game)
    leaves = _both_queries_against_replay(g, game, oracle_lib, "%s written states" % game)
    assert (leaves["ret"] > 0).any()
    _held_to_twin(g, o, "%s written states after the queries" % game)
    g.close(); o.close()


def test_breakout_wave_per_env_step_form(hip_lib, oracle_lib):
    """TBX_OPT_STEP_FORM = 2: the canonical wall through the wave form"""
    n = 40
    g = Engine("breakout", n, lib=hip_lib)
    g.set_option(_abi.OPT_STEP_FORM, _abi.STEP_FORM_WAVE_PER_ENV)
    o = batch(oracle_lib, "breakout", n)
    g.set_states(0, o.get_states())
    for i, r in enumerate(sim_rngs(o)):
        g.set_sim_rng((int(r[0]), int(r[1])), env=i)
    _held_to_twin(g, o, "breakout, wave per env")
    leaves = _both_queries_against_replay(g, "breakout", oracle_lib, "breakout, wave per env")
    assert (leaves["ret"] > 0).any() and (leaves["lives"] <= 0).any()
    g.close(); o.close()


def test_the_adapter_after_agent_init(hip_lib, oracle_lib):
    """ToyboxPreprocVecEnv.search / lookahead_plan: agent steps, action indices, the winner among an env's rows"""
    from toybox_amd.envs import ToyboxPreprocVecEnv
    game, n = "space_invaders", 24
    v = ToyboxPreprocVecEnv(game, n, seed=3, engine=Engine(game, n, lib=hip_lib))
    v.reset()
    rng = np.random.default_rng(0)
    for _ in range(20):
        v.step(rng.integers(0, v.action_space.n, n))
    v.step_async(rng.integers(0, v.action_space.n, n))        # a pending step ends first
    for objective in OBJECTIVES:
        got = v.search(steps=12, depth=2, objective=objective, rest=0)
        assert v._in_flight is None
        want = expected_search(oracle_lib, game, v.engine.get_states(), sim_rngs(v.engine), dict(frames=48, hold=4, depth=2, objective=OBJECTIVES.index(objective), rest=0))
        assert_search_equal(got, want, "ToyboxPreprocVecEnv.search %s" % objective)
        L = len(LEGAL[game])
        assert np.array_equal(got["plan"], np.stack([want["code"] % L, want["code"] // L], axis=-1))
        best = pick_rows(want, OBJECTIVES.index(objective))
        assert np.array_equal(got["best_action"], best) and np.array_equal(got["best_plan"], got["plan"][np.arange(n), best])
    plan = rng.integers(0, v.action_space.n, (n, 3))
    got = v.lookahead_plan(steps=10, plan=plan, rest=1)
    code = (plan * len(LEGAL[game]) ** np.arange(3)).sum(axis=1)
    assert_fields_equal(got, expected_plan(oracle_lib, game, v.engine.get_states(), sim_rngs(v.engine), dict(frames=40, hold=4, depth=3, code=code, rest=1)),
                        "ToyboxPreprocVecEnv.lookahead_plan")
    v.close()


def test_batch_intervention_mirrors_both(hip_lib, oracle_lib):
    """BatchIntervention.lookahead_search / lookahead_plan over a sub-range: the engine's rows of that range, per-env columns of the
    range included"""
    from toybox_amd.interventions import BatchIntervention
    game, n, first, count = "breakout", 24, 5, 11
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    whole = g.lookahead_search(48, 2, hold=4, objective="survival", rest=0)
    plan = np.asarray(LEGAL[game])[np.random.default_rng(1).integers(0, 4, (n, 3))]
    frames = np.resize([40, 64, 17], n)
    whole_plan = g.lookahead_plan(frames, plan, hold=4)
    with BatchIntervention(g, first, count) as bi:
        part = bi.lookahead_search(48, 2, hold=4, objective="survival", rest=0)
        part_plan = bi.lookahead_plan(frames[first:first + count], plan[first:first + count], hold=4)
    for k in SEARCH_FIELDS + ("plan",):
        assert np.array_equal(part[k], whole[k][first:first + count]), k
    for k in FIELDS:
        assert np.array_equal(part_plan[k], whole_plan[k][first:first + count]), k


def pick_rows(rows, objective):
    """the winner among the rows [n, L] of every env, a plain loop: larger keys first, then the smaller code"""
    n, L = rows["ret"].shape
    best = np.zeros(n, np.int64)
    for i in range(n):
        def key(a):
            loss = 1025 if rows["life_lost_at"][i, a] < 0 else int(rows["life_lost_at"][i, a])
            k = (rows["ret"][i, a], rows["lives"][i, a], loss) if objective == 0 else (rows["lives"][i, a], loss, rows["ret"][i, a])
            return tuple(-float(x) for x in k) + (int(rows["code"][i, a]),)
        best[i] = min(range(L), key=key)
    return best


# ---------------------------------------------------------------- 5. nothing written

@pytest.mark.parametrize("game", GAMES)
def test_the_queries_leave_the_engine_untouched(game, hip_lib, oracle_lib):
    """state records, simulator RNGs, step outputs and scalars are byte-equal before and after both queries -- the chunked search,
    whose partial rows go to a scratch of the engine's, included -- and the next synthetic step gives what an untouched twin gives"""
    n = 24
    g, twin = batch(hip_lib, game, n), batch(hip_lib, game, n)
    before = _snapshot(g)
    g.lookahead_search(40, 3, hold=4, objective="survival", rest=LEGAL[game][0])
    assert g.search_chunks > 1
    g.lookahead_plan(64, np.resize(LEGAL[game], (n, 4)), hold=4)
    _assert_same_snapshot(_snapshot(g), before, game)
    for e in (g, twin):
        e.step_synthetic(1337, 400, auto_reset=True)
    _assert_same_snapshot(_snapshot(g), _snapshot(twin), "%s: the step after the queries" % game)
    g.close(); twin.close()


@pytest.mark.parametrize("game", GAMES)
def test_the_queries_leave_the_agent_layer_untouched(game, hip_lib, oracle_lib):
    n = 16
    case = Agent(game, n)
    g, o = case.make(hip_lib), case.make(oracle_lib)
    case.run(g, 0, 12); case.run(o, 0, 12)
    obs, before = read_buffer(g, _abi.BUF_AGENT_OBS, (n, 84, 84, 4)), _snapshot(g)
    got = g.lookahead_search(24, 2, hold=4, seed=11, t=12)
    g.lookahead_plan(24, [LEGAL[game][1], LEGAL[game][0]], hold=4)
    assert np.array_equal(read_buffer(g, _abi.BUF_AGENT_OBS, (n, 84, 84, 4)), obs), "TBX_BUF_AGENT_OBS changed"
    _assert_same_snapshot(_snapshot(g), before, "%s with the agent layer" % game)
    assert_search_equal(got, expected_search(oracle_lib, game, g.get_states(), sim_rngs(g), dict(frames=24, hold=4, depth=2, seed=11, t=12)),
                        "%s with the agent layer on: raw frames from the state as it stands" % game)
    rows_g, rows_o = case.run(g, 12, 16), case.run(o, 12, 16)
    for x, y in zip(rows_g, rows_o):
        for u, w in zip(x, y):
            assert np.array_equal(u, w), "%s: the agent steps after the queries" % game
    g.close(); o.close()


# ---------------------------------------------------------------- 6. refusals

@pytest.mark.parametrize("game", GAMES)
def test_shared_refusals(game, hip_lib, oracle_lib):
    g, _, _ = _world(game, 24, 400, hip_lib, oracle_lib)
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    illegal = 2 if game == "breakout" else 17
    too_deep = {4: 7, 5: 6, 6: 5}[L]
    before = _snapshot(g)
    bad_search = {"depth 0": [8, 1, 0], "too many plans": [8, 1, too_deep], "objective 2": [8, 1, 2, 2], "illegal rest": [8, 1, 2, 0, illegal], "frames 0": [0],
                  "frames 1025": [1025], "hold 0": [8, 0], "ten arguments": [8, 1, 1, 0, -1, 0, 0, 0, 0, 0], "no arguments": []}
    bad_plan = {"code = L^depth": [8, 1, 2, L * L], "code -1": [8, 1, 2, -1], "code at depth 0": [8, 1, 0, 1], "depth too large": [8, 1, top + 1, 0], "depth -1": [8, 1, -1],
                "illegal rest": [8, 1, 2, 0, illegal], "frames 0": [0], "frames 1025": [1025], "hold 0": [8, 0], "ten arguments": [8, 1, 1, 0, -1, 0, 0, 0, 0, 0]}
    for query, cases in ((_abi.QUERY_LOOKAHEAD_SEARCH, bad_search), (_abi.QUERY_LOOKAHEAD_PLAN, bad_plan)):
        for what, args in cases.items():
            with pytest.raises(ToyboxAmdError) as ei:
                g.reduce(query, args)
            assert ei.value.code == _abi.E_INVALID, (what, query)
    _assert_same_snapshot(_snapshot(g), before, "%s after the refusals" % game)
    assert g.reduce(_abi.QUERY_LOOKAHEAD_PLAN, [8, 1, top, L ** top - 1]).shape == (24, 5)       # the deepest plan, its largest code
    assert g.reduce(_abi.QUERY_LOOKAHEAD_SEARCH, [8, 1, too_deep - 1]).shape == (24, 6 * L)       # the deepest search
    for name in GAMES:
        assert hip_lib.tbx_reduce_width(_abi.GAME_IDS[name], _abi.QUERY_LOOKAHEAD_PLAN) == 5
        assert hip_lib.tbx_reduce_width(_abi.GAME_IDS[name], _abi.QUERY_LOOKAHEAD_SEARCH) == 6 * len(LEGAL[name])


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("game", GAMES)
def test_refused_rows_answer_zeros_and_leave_their_neighbours(game, form, hip_lib, oracle_lib):
    """per-env rows with each kind of bad value: zeros for those envs, the right rows for the others"""
    n = 24
    g, states, rngs = _world(game, n, 400, hip_lib, oracle_lib)
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    illegal = 2 if game == "breakout" else 17
    too_deep = {4: 7, 5: 6, 6: 5}[L]
    # the search: depth 0, too many plans, depth beyond every plan, objective 2 and -1, illegal rest, frames 0 / 1025, hold 0
    s = dict(frames=np.full(n, 32), hold=np.full(n, 4), depth=np.resize([1, 2, 3], n), objective=np.resize([0, 1], n), rest=np.full(n, LEGAL[game][0]))
    s["depth"][[1, 2, 3]] = [0, too_deep, top + 1]
    s["objective"][[5, 6]] = [2, -1]
    s["rest"][8] = illegal
    s["frames"][[10, 11]] = [0, 1025]
    s["hold"][13] = 0
    bad = [1, 2, 3, 5, 6, 8, 10, 11, 13]
    want = expected_search(oracle_lib, game, states, rngs, s)
    assert all((want[k][bad] == 0).all() for k in SEARCH_FIELDS) and (want["frames_run"][np.setdiff1d(np.arange(n), bad)] > 0).all()
    args, per_env = search_args(game, n, **s)
    assert per_env
    rows = g.reduce(_abi.QUERY_LOOKAHEAD_SEARCH, args) if form == "host" else _device_reduce(g, _abi.QUERY_LOOKAHEAD_SEARCH, args, 6 * L)
    assert g.search_chunks > 1
    assert_search_equal(_search_dict(rows, n, L), want, "%s search rows (%s form)" % (game, form))
    # the plan: code = L^depth, code -1, a code at depth 0, depth beyond the largest, depth -1, illegal rest, frames 0 / 1025, hold 0
    p = dict(frames=np.full(n, 32), hold=np.full(n, 4), depth=np.resize([0, 1, 2, 5], n), code=np.zeros(n, np.int64), rest=np.full(n, -1), seed=9)
    p["code"][[2, 6]] = [L * L - 1, L * L]
    p["code"][[7, 4]] = [-1, 1]
    p["depth"][[9, 10]] = [top + 1, -1]
    p["rest"][12] = illegal
    p["frames"][[14, 15]] = [0, 1025]
    p["hold"][17] = 0
    bad = [6, 7, 4, 9, 10, 12, 14, 15, 17]
    want = expected_plan(oracle_lib, game, states, rngs, p)
    assert all((want[k][bad] == 0).all() for k in FIELDS) and (want["frames_run"][np.setdiff1d(np.arange(n), bad)] > 0).all()
    args, _ = plan_args(game, n, **p)
    rows = g.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args) if form == "host" else _device_reduce(g, _abi.QUERY_LOOKAHEAD_PLAN, args, 5)
    assert_fields_equal(Engine._lookahead_dict(rows), want, "%s plan rows (%s form)" % (game, form))
