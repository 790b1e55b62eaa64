"""Lookahead on the device (TBX_QUERY_LOOKAHEAD / _ALL, include/toybox_amd.h) against CLONE AND PLAY on the CPU checker
(tests/lookahead_replay.py; its own checks are in tests/test_lookahead.py).  Every comparison is exact, on all five fields.

The engine under test is made by the input recipe and held to its checker twin byte for byte (state records, simulator RNGs) before
any query; the expected rows are then played on clones of the records the DEVICE engine reports."""
import functools

import numpy as np
import pytest

from fork_replay import Agent, Raw, assert_rows_equal, sim_rngs, states_bytes
from lookahead_replay import FIELDS, assert_coverage, assert_fields_equal, batch, coverage, expected, merge_coverage
from support import LEGAL, read_buffer
from test_gpu_custom_states import _engines, _write_all, fuzz_seed, generate  # noqa: F401  (fuzz_seed: the fixture)
from toybox_amd import ToyboxAmdError, _abi
from toybox_amd.engine import LOOKAHEAD_FIELDS, Engine, lookahead_args

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
H = 300
SCHEDULES = {"random": dict(frames=H, seed=1337), "hold4_noop": dict(frames=H, hold=4, rest=0)}
STEP_BUFFERS = ((_abi.BUF_REWARD, np.int32), (_abi.BUF_DONE, np.uint8), (_abi.BUF_LIVES, np.int32), (_abi.BUF_SCORE, np.int32), (_abi.BUF_PACKED, np.uint64))
_WORLDS = {}


def _held_to_twin(g, o, what):
    assert np.array_equal(states_bytes(g), states_bytes(o)), "%s: the device engine's state records are not its checker twin's" % what
    assert np.array_equal(sim_rngs(g), sim_rngs(o)), "%s: simulator RNGs differ from the checker twin's" % what


def _world(game, n, hip_lib, oracle_lib):
    """(device engine, its state records, its simulator RNGs) of the input recipe, made once per (game, n) and only ever queried"""
    if (game, n) not in _WORLDS:
        g, o = batch(hip_lib, game, n), batch(oracle_lib, game, n)
        _held_to_twin(g, o, "%s n=%d" % (game, n))
        o.close()
        _WORLDS[(game, n)] = (g, g.get_states(), sim_rngs(g))
    return _WORLDS[(game, n)]


@functools.lru_cache(maxsize=None)
def _expected_all(game, n, name, hip_lib, oracle_lib):
    g, states, rngs = _world(game, n, hip_lib, oracle_lib)
    out = expected(oracle_lib, game, states, rngs, SCHEDULES[name], all_actions=True)
    for v in out.values():
        v.flags.writeable = False
    return out


def _dict_of(rows):
    """float64 [..., 5] as tbx_reduce returns it -> the five named fields"""
    return Engine._lookahead_dict(np.asarray(rows))


def _snapshot(g):
    return (states_bytes(g), sim_rngs(g)) + tuple(read_buffer(g, b, (g.n_envs,), dt) for b, dt in STEP_BUFFERS)


def _assert_same_snapshot(a, b, what):
    for name, x, y in zip(("state records", "simulator RNGs", "reward", "done", "lives", "score", "packed"), a, b):
        assert np.array_equal(x, y), "%s: %s changed" % (what, name)


# ---------------------------------------------------------------- 1. all actions == replay

@pytest.mark.parametrize("name", list(SCHEDULES))
@pytest.mark.parametrize("n", [1, 97])
@pytest.mark.parametrize("game", GAMES)
def test_all_actions_equal_replay(game, n, name, hip_lib, oracle_lib):
    """97 envs are 388 / 582 / 485 (env, candidate) pairs: partial blocks, and an env's candidates straddle block and wave-group seams"""
    g, _, _ = _world(game, n, hip_lib, oracle_lib)
    s = SCHEDULES[name]
    got = g.lookahead_all(s["frames"], hold=s.get("hold", 1), rest=s.get("rest"), seed=s.get("seed", 0))
    assert got["ret"].shape == (n, len(LEGAL[game])) and got["ret"].dtype == np.float64 and got["lives"].dtype == np.int64
    assert_fields_equal(got, _expected_all(game, n, name, hip_lib, oracle_lib), "%s n=%d %s" % (game, n, name))
    assert g.reduce_width(_abi.QUERY_LOOKAHEAD_ALL) == 5 * len(LEGAL[game])


@pytest.mark.parametrize("game", GAMES)
def test_the_cases_cover_what_they_must(game, hip_lib, oracle_lib):
    """over this module's all-action cases together: an env ends inside the horizon, one runs all of it, one scores, one loses a life
    without ending (not GridWorld)"""
    total = {}
    for name in SCHEDULES:
        for n in (1, 97):
            merge_coverage(total, coverage(_expected_all(game, n, name, hip_lib, oracle_lib), H))
    assert_coverage(game, total)


# ---------------------------------------------------------------- 2. the single form, one row per env

def _per_env_schedule(game, n):
    rng = np.random.default_rng(7)
    legal = np.asarray(LEGAL[game] + [-1])
    frames = np.resize([1, 2, 4, 299, 300, 1024, 17, 64, 33], n)
    hold = np.resize([1, 4, 7], n)
    first, rest = legal[rng.integers(0, len(legal), n)], legal[rng.integers(0, len(legal), n)]
    t = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    t[:3] = [0, 2 ** 32 - 1, 2 ** 32 - 5]                     # (the counter t + p leaves 32 bits)
    env_offset = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    env_offset[:2] = [0, 2 ** 32 - 1]
    first[11] = 2 if game == "breakout" else 17               # an illegal first: that env's row is zeros
    frames[20] = 0                                            # ... and a horizon of 0
    return dict(frames=frames, hold=hold, first=first, rest=rest, seed=(0xC0FFEE << 32) | 0x5EED, t=t, env_offset=env_offset), [11, 20]


@pytest.mark.parametrize("game", GAMES)
def test_single_form_per_env_rows(game, hip_lib, oracle_lib):
    from toybox_amd import hip
    n = 97
    g, states, rngs = _world(game, n, hip_lib, oracle_lib)
    sched, refused = _per_env_schedule(game, n)
    assert {1, 2, 4, 299, 300, 1024} <= set(sched["frames"].tolist()) and set(sched["hold"].tolist()) == {1, 4, 7}
    want = expected(oracle_lib, game, states, rngs, sched)
    for k in FIELDS:
        assert (want[k][refused] == 0).all()
    got = g.lookahead(**sched)
    assert got["ret"].shape == (n,)
    assert_fields_equal(got, want, "%s single form, per-env rows (host form)" % game)
    # the device form with the rows uploaded, on a caller's stream
    args, per_env = lookahead_args(n, **sched)
    assert per_env and args.shape == (n, 8)
    s = hip.Stream()
    a_dev, o_dev = hip.malloc(args.nbytes), hip.malloc(n * 5 * 8)
    try:
        hip.memcpy_htod(a_dev, args, args.nbytes)
        g.reduce_device(_abi.QUERY_LOOKAHEAD, o_dev, stream=s.ptr, per_env_ptr=a_dev, n_args=8)
        s.synchronize()
        rows = np.empty((n, 5), np.float64)
        hip.memcpy_dtoh(rows, o_dev, rows.nbytes)
    finally:
        g.sync()
        hip.free(a_dev)
        hip.free(o_dev)
        s.close()
    assert_fields_equal(_dict_of(rows), want, "%s single form, per-env rows (device form)" % game)
    assert g.reduce_width(_abi.QUERY_LOOKAHEAD) == 5


def test_breakout_wave_per_env_step_form(hip_lib, oracle_lib):
    """TBX_OPT_STEP_FORM = 2: both queries on the canonical wall through the wave form (40 envs: 120 pairs, a partial block)"""
    n = 40
    g = Engine("breakout", n, lib=hip_lib)
    g.set_option(_abi.OPT_STEP_FORM, _abi.STEP_FORM_WAVE_PER_ENV)
    o = batch(oracle_lib, "breakout", n)
    g.set_states(0, o.get_states())
    for i, r in enumerate(sim_rngs(o)):
        g.set_sim_rng((int(r[0]), int(r[1])), env=i)
    _held_to_twin(g, o, "breakout, wave per env")
    states, rngs = g.get_states(), sim_rngs(g)
    s = SCHEDULES["hold4_noop"]
    sched, refused = _per_env_schedule("breakout", n)
    assert refused == [11, 20]
    want_all = expected(oracle_lib, "breakout", states, rngs, s, all_actions=True)
    want = expected(oracle_lib, "breakout", states, rngs, sched)
    for w, frames in ((want_all, H), (want, sched["frames"])):
        cov = coverage(w, frames)
        assert cov["scored"] and cov["ended"], cov
    for k in FIELDS:
        assert (want[k][refused] == 0).all()
    assert_fields_equal(g.lookahead_all(s["frames"], hold=s["hold"], rest=s["rest"]), want_all, "breakout, wave per env, all actions")
    assert_fields_equal(g.lookahead(**sched), want, "breakout, wave per env, single form")
    _held_to_twin(g, o, "breakout, wave per env, after the queries")
    g.close(); o.close()


# ---------------------------------------------------------------- 3. untouched

@pytest.mark.parametrize("game", GAMES)
def test_the_query_leaves_the_engine_untouched(game, hip_lib, oracle_lib):
    """state bytes, simulator RNGs and every step output buffer are the same before and after; the next 50 steps with RGB frames equal
    those of a checker twin that was never queried"""
    n = 97
    g, o = batch(hip_lib, game, n), batch(oracle_lib, game, n)
    _held_to_twin(g, o, game)
    before = _snapshot(g)
    g.lookahead_all(H, seed=3)
    g.lookahead(64, hold=4, first=LEGAL[game][1], rest=np.resize(LEGAL[game], n))
    _assert_same_snapshot(_snapshot(g), before, game)
    case = Raw(game, n, lives_one=False)
    assert_rows_equal(case.run(g, 400, 450, frames=3), case.run(o, 400, 450, frames=3), "%s: the 50 steps after the query" % game)
    _held_to_twin(g, o, "%s after 50 more steps" % game)
    g.close(); o.close()


@pytest.mark.parametrize("new_plane", [0, 2], ids=["rolled_stack", "ring"])
@pytest.mark.parametrize("game", GAMES)
def test_the_query_leaves_the_agent_layer_untouched(game, new_plane, hip_lib, oracle_lib):
    """with every wrapper on: the observation is the same before and after, and the next 8 agent steps equal the unqueried twin's"""
    n = 33
    case = Agent(game, n, new_plane=new_plane)
    g, o = case.make(hip_lib), case.make(oracle_lib)
    assert_rows_equal(case.run(g, 0, 30), case.run(o, 0, 30), "%s: 30 agent steps" % game)
    obs, before = case.observation(g), _snapshot(g)
    got = g.lookahead_all(20, hold=4, seed=11, t=30)
    assert np.array_equal(case.observation(g), obs), "the observation changed"
    _assert_same_snapshot(_snapshot(g), before, "%s with the agent layer" % game)
    assert_fields_equal(got, expected(oracle_lib, game, g.get_states(), sim_rngs(g), dict(frames=20, hold=4, seed=11, t=30), all_actions=True),
                        "%s with the agent layer on: raw frames from the state as it stands" % game)
    assert_rows_equal(case.run(g, 30, 38), case.run(o, 30, 38), "%s: the 8 agent steps after the query" % game)
    g.close(); o.close()


# ---------------------------------------------------------------- 4. the query foretells the engine's own random rollout

@pytest.mark.parametrize("game", GAMES)
def test_foretells_the_synthetic_rollout(game, hip_lib, oracle_lib):
    n, frames, seed, t = 700, 64, (9 << 40) | 1337, 12345
    g = batch(hip_lib, game, n)
    q = g.lookahead(frames, seed=seed, t=t)
    lives0 = g.scalars()[1].astype(np.int64)
    ret, run, lost = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    score, lives, live = np.zeros(n, np.int64), lives0.copy(), np.ones(n, bool)
    for j in range(frames):
        g.step_synthetic(seed, t + j, auto_reset=False)
        reward, done, lv, sc = (read_buffer(g, b, (n,), dt).astype(np.int64) for b, dt in STEP_BUFFERS[:4])
        ret[live] += reward[live]
        score[live], lives[live] = sc[live], lv[live]
        lost[live & (lost < 0) & (lv < lives0)] = j
        run[live] = j + 1
        assert np.array_equal(done != 0, lv <= 0)
        live &= done == 0
    assert live.any() and not live.all(), "the rollout must end some games inside the horizon and leave others running"
    assert_fields_equal(q, dict(ret=ret.astype(np.float64), score=score, lives=lives, frames_run=run, life_lost_at=lost), "%s foretold" % game)
    g.close()


# ---------------------------------------------------------------- 5. program order

ORDER_FORMS = ["chunks1", "chunks2", "chunks3", "chunks4", "fused_overlap", "pipeline3"]


@pytest.mark.parametrize("form", ORDER_FORMS)
@pytest.mark.parametrize("game", ["breakout", "space_invaders"])
def test_program_order_behind_unsynchronised_loop_forms(game, form, hip_lib, oracle_lib):
    """the query, issued through the host form straight behind unsynchronised calls on a caller's stream, sees the state after them"""
    from toybox_amd import hip
    n, frames = 700, 48
    g, o = batch(hip_lib, game, n), batch(oracle_lib, game, n)
    if form.startswith("chunks"):
        g.set_option(_abi.OPT_ROLLOUT_CHUNKS, int(form[-1]))
    elif form == "fused_overlap":
        g.set_option(_abi.OPT_FUSED_OVERLAP, _abi.FUSED_OVERLAP_ON)
    else:
        g.set_option(_abi.OPT_PIPELINE, _abi.PIPELINE_OVERLAP_RENDERS)
    s = hip.Stream()
    t = 400
    for _ in range(3):
        if form.startswith("chunks"):
            g.rollout_synthetic(1337, t, 3, channels=3, auto_reset=True, stream=s.ptr)
            t += 3
        elif form == "fused_overlap":
            g.render_step_synthetic(1337, t, channels=3, auto_reset=True, stream=s.ptr)
            t += 1
        else:
            g.step_synthetic(1337, t, auto_reset=True, stream=s.ptr)
            g.render_device(0, 3, stream=s.ptr)
            t += 1
    got = g.lookahead_all(frames, seed=5, t=t)                 # (no synchronisation in between)
    for k in range(400, t):
        o.step_synthetic(1337, k, auto_reset=True)
    want = expected(oracle_lib, game, o.get_states(), sim_rngs(o), dict(frames=frames, seed=5, t=t), all_actions=True)
    assert_fields_equal(got, want, "%s behind %s" % (game, form))
    g.sync()
    _held_to_twin(g, o, "%s after %s and the query" % (game, form))
    s.close()
    g.close(); o.close()


# ---------------------------------------------------------------- 6. written states

@pytest.mark.parametrize("game", ["breakout", "space_invaders"])
def test_written_states(game, fuzz_seed, hip_lib, oracle_lib):
    """a Breakout batch that has left the canonical wall (per-env brick tables: the wave-per-env lookahead kernel) and a SpaceInvaders
    batch off the formation grid (the full load), built the way tests/test_gpu_custom_states.py builds them"""
    n = 203
    es = g, o = _engines(game, n, (hip_lib, oracle_lib))
    _write_all(es, generate(game, o, np.random.default_rng(fuzz_seed)))
    for e in es:
        for t in range(20):
            e.step_synthetic(1337, t, auto_reset=True)
    _held_to_twin(g, o, "%s written states" % game)
    states, rngs = g.get_states(), sim_rngs(g)
    for sched in (dict(frames=200, seed=21), dict(frames=120, hold=4, rest=LEGAL[game][2])):
        want = expected(oracle_lib, game, states, rngs, sched, all_actions=True)
        got = g.lookahead_all(sched["frames"], hold=sched.get("hold", 1), rest=sched.get("rest"), seed=sched.get("seed", 0))
        assert_fields_equal(got, want, "%s written states %r" % (game, sched))
        assert (want["ret"] > 0).any() and (want["lives"] <= 0).any()
    _held_to_twin(g, o, "%s written states after the queries" % game)
    g.close(); o.close()


# ---------------------------------------------------------------- 7. refusals

@pytest.mark.parametrize("game", GAMES)
def test_refusals_and_widths(game, hip_lib, oracle_lib):
    g, _, _ = _world(game, 97, hip_lib, oracle_lib)
    before = _snapshot(g)
    illegal = 2 if game == "breakout" else 17
    bad = {"frames 0": [0], "frames 1025": [1025], "hold 0": [8, 0], "illegal first": [8, 1, illegal], "illegal rest": [8, 1, -1, illegal],
           "nine arguments": [8, 1, -1, -1, 0, 0, 0, 0, 0]}
    for what, args in bad.items():
        for query in (_abi.QUERY_LOOKAHEAD, _abi.QUERY_LOOKAHEAD_ALL):
            if what == "illegal first" and query == _abi.QUERY_LOOKAHEAD_ALL:
                continue                                       # (the all-actions form ignores the column)
            with pytest.raises(ToyboxAmdError) as ei:
                g.reduce(query, args)
            assert ei.value.code == _abi.E_INVALID, (what, query)
    _assert_same_snapshot(_snapshot(g), before, "%s after the refusals" % game)
    assert g.reduce(_abi.QUERY_LOOKAHEAD_ALL, [8, 1, illegal]).shape == (97, 5 * len(LEGAL[game]))
    widths = {"breakout": 20, "space_invaders": 30, "amidar": 30, "gridworld": 25}
    for name, w in widths.items():
        assert hip_lib.tbx_reduce_width(_abi.GAME_IDS[name], _abi.QUERY_LOOKAHEAD) == 5
        assert hip_lib.tbx_reduce_width(_abi.GAME_IDS[name], _abi.QUERY_LOOKAHEAD_ALL) == w
    assert tuple(LOOKAHEAD_FIELDS) == tuple(FIELDS)


# ---------------------------------------------------------------- 8. the adapters

def test_adapters(hip_lib, oracle_lib):
    from toybox_amd.envs import ToyboxPreprocVecEnv, ToyboxVecEnv
    n = 64
    v = ToyboxPreprocVecEnv("space_invaders", n, seed=3, engine=Engine("space_invaders", n, lib=hip_lib))
    v.reset()
    rng = np.random.default_rng(0)
    for _ in range(20):
        v.step(rng.integers(0, v.action_space.n, n))
    want = v.engine.lookahead_all(frames=20, hold=4, seed=8, t=2)
    got = v.lookahead(steps=5, all_actions=True, seed=8, t=2)
    assert_fields_equal(got, want, "ToyboxPreprocVecEnv.lookahead(all_actions)")
    assert got["ret"].shape == (n, v.action_space.n)
    one = v.lookahead(steps=5, first=4, rest=0)
    assert_fields_equal(one, v.engine.lookahead(20, hold=4, first=11, rest=0), "action indices -> ALE ids")
    assert_fields_equal(one, expected(oracle_lib, "space_invaders", v.engine.get_states(), sim_rngs(v.engine), dict(frames=20, hold=4, first=11, rest=0)),
                        "ToyboxPreprocVecEnv.lookahead against the replay")
    a = rng.integers(0, v.action_space.n, n)
    v.step_async(a)                                           # a pending step ends first: the answer is about the state after it
    got = v.lookahead(steps=3, all_actions=True)
    assert v._in_flight is None
    assert_fields_equal(got, expected(oracle_lib, "space_invaders", v.engine.get_states(), sim_rngs(v.engine), dict(frames=12, hold=4), all_actions=True),
                        "lookahead behind step_async")
    v.close()
    r = ToyboxVecEnv("breakout", n, seed=1, engine=Engine("breakout", n, lib=hip_lib))
    r.reset()
    for _ in range(30):
        r.step(rng.integers(0, r.action_space.n, n))
    r.step_async(rng.integers(0, r.action_space.n, n))
    got = r.lookahead(steps=40, first=np.resize([1, 2, 3], n), seed=5)
    want = expected(oracle_lib, "breakout", r.engine.get_states(), sim_rngs(r.engine), dict(frames=40, first=np.resize([1, 3, 4], n), seed=5))
    assert_fields_equal(got, want, "ToyboxVecEnv.lookahead")
    r.close()
