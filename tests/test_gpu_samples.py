"""The sampled lookahead on the device (TBX_QUERY_LOOKAHEAD_SAMPLES, include/toybox_amd.h) against CLONE, SALT AND PLAY on the CPU
checker (tests/sample_replay.py; its own checks are in tests/test_samples.py).  Every comparison is exact, on every field of every
(env, first action) group.

The engine under test is made by the input recipe of tests/lookahead_replay.py and held to its checker twin byte for byte before any
query (the worlds of tests/test_gpu_search.py, shared with it); the expected rows are played on clones of the records the DEVICE
engine reports, once per case, and shared.  Measured on the checker for the "coverage" case of every game (samples 8, rest drawn,
seed 77; tests/test_samples.py prints them) -- groups whose futures differ in their return / with 0 < lost < S / with an ended
future / with lost == S, out of the game's groups: Breakout (24, 160, 4) 37 / 36 / 71 / 55 of 96; SpaceInvaders (16, 120, 4)
92 / 48 / 32 / 4 of 96; Amidar (24, 96, 4) 69 / 28 / 17 / 13 of 144; GridWorld (24, 24, 2) a spread in 40 of 120.  The salt alone,
under fixed actions, leaves 22 of SpaceInvaders' 96 groups with 0 < lost < S."""
import functools

import numpy as np
import pytest

from fork_replay import Agent, sim_rngs
from lookahead_replay import batch
from sample_replay import (LEAF_FIELDS, SALT_PAIRS, WORLDS, aggregate, assert_samples_equal, best_action, coverage, expected_samples, settings)
from support import LEGAL, read_buffer
from test_gpu_custom_states import _engines, _write_all, fuzz_seed, generate  # noqa: F401  (fuzz_seed: the fixture)
from test_gpu_search import _assert_same_snapshot, _device_reduce, _held_to_twin, _snapshot, _world
from toybox_amd import ToyboxAmdError, _abi
from toybox_amd.engine import SAMPLE_FIELDS, Engine, sample_args, sample_seed

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
MAIN = ("coverage", "one", "five", "thirtythree")


def _game_world(game, hip_lib, oracle_lib):
    n, _, _, batch_frames = WORLDS[game]
    return _world(game, n, batch_frames, hip_lib, oracle_lib)


@functools.lru_cache(maxsize=None)
def _expected(game, name, hip_lib, oracle_lib):
    _, states, rngs = _game_world(game, hip_lib, oracle_lib)
    _, frames, hold, _ = WORLDS[game]
    out = expected_samples(oracle_lib, game, states, rngs, settings(game, frames, hold)[name])
    for v in out.values():
        v.flags.writeable = False
    return out


def _ask(g, case):
    c = dict(case)
    if c.get("rest") == -1:
        c["rest"] = None
    return g.lookahead_samples(c.pop("frames"), c.pop("samples"), **c)


def _assert_chunks(g, samples, what):
    if samples == 1:
        assert g.sample_chunks == 1, "%s: one sample cannot be cut up" % what
    else:
        assert g.sample_chunks > 1, "%s: %d envs are far below a wave per SIMD, the samples are cut into chunks" % (what, g.n_envs)


# ---------------------------------------------------------------- 1. the device == every future replayed, then summed

@pytest.mark.parametrize("name", MAIN)
@pytest.mark.parametrize("game", GAMES)
def test_samples_equal_replay(game, name, hip_lib, oracle_lib):
    g, _, _ = _game_world(game, hip_lib, oracle_lib)
    n, frames, hold, _ = WORLDS[game]
    L = len(LEGAL[game])
    case = settings(game, frames, hold)[name]
    got = _ask(g, case)
    assert all(got[k].shape == (n, L) and got[k].dtype == np.int64 for k in SAMPLE_FIELDS) and (got["samples"] == case["samples"]).all()
    _assert_chunks(g, case["samples"], "%s %s" % (game, name))
    assert_samples_equal(got, _expected(game, name, hip_lib, oracle_lib), "%s %s %r" % (game, name, case))
    assert g.reduce_width(_abi.QUERY_LOOKAHEAD_SAMPLES) == 8 * L


def _all_settings_against_replay(g, game, oracle_lib, what, frames=64, hold=4):
    """the settings of the main cases on an engine in another form (smaller: the replay is per engine here)"""
    states, rngs = g.get_states(), sim_rngs(g)
    total = {}
    for name in MAIN:
        case = settings(game, frames, hold)[name]
        want = expected_samples(oracle_lib, game, states, rngs, case)
        assert_samples_equal(_ask(g, case), want, "%s %s" % (what, name))
        _assert_chunks(g, case["samples"], "%s %s" % (what, name))
        for k, v in coverage(want).items():
            total[k] = total.get(k, 0) + v
    return total


@pytest.mark.parametrize("game", ["breakout", "space_invaders"])
def test_written_states(game, fuzz_seed, hip_lib, oracle_lib):
    """a Breakout batch that has left the canonical wall (the wave form with per-env brick tables) and a SpaceInvaders batch off the
    formation grid (the full load), built the way tests/test_gpu_custom_states.py builds them"""
    n = 16
    es = g, o = _engines(game, n, (hip_lib, oracle_lib))
    _write_all(es, generate(game, o, np.random.default_rng(fuzz_seed)))
    for e in es:
        for t in range(20):
            e.step_synthetic(1337, t, auto_reset=True)
    _held_to_twin(g, o, "%s written states" % game)
    total = _all_settings_against_replay(g, game, oracle_lib, "%s written states" % game)
    assert total["scored"] and total["spread"], total
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
    total = _all_settings_against_replay(g, "breakout", oracle_lib, "breakout, wave per env", frames=160)
    assert total["spread"] and total["some_lost"] and total["ended"], total
    g.close(); o.close()


# ---------------------------------------------------------------- 2. the device == itself: samples calls of lookahead_all, summed

@pytest.mark.parametrize("game", GAMES)
def test_unsalted_samples_are_lookahead_all_calls_summed(game, hip_lib, oracle_lib):
    g, _, _ = _game_world(game, hip_lib, oracle_lib)
    n, frames, hold, _ = WORLDS[game]
    S, seed, t, off = 12, (7 << 33) | 5, 2 ** 32 - 2, 99
    got = g.lookahead_samples(frames, S, hold=hold, seed=seed, t=t, env_offset=off)
    calls = [g.lookahead_all(frames, hold=hold, seed=sample_seed(seed, s), t=t, env_offset=off) for s in range(S)]
    leaves = {k: np.stack([np.asarray(c[k]).astype(np.int64) for c in calls]) for k in LEAF_FIELDS}
    assert_samples_equal(got, aggregate(leaves, np.ones((S, n), bool)), "%s against %d lookahead_all calls" % (game, S))


# ---------------------------------------------------------------- 3. per-env rows, tbx_reduce_device on a caller's stream

def _mixed_rows(game, n):
    legal = np.asarray(LEGAL[game] + [-1])
    rng = np.random.default_rng(13)
    return dict(frames=np.resize([24, 17, 40, 1, 33], n), hold=np.resize([4, 1, 3, 8], n), samples=np.resize([3, 1, 7, 2, 5, 4], n),
                salt=np.resize([0, 1000, 2 ** 32 - 7, 0, 5], n), rest=legal[rng.integers(0, len(legal), n)], seed=(0xC0FFEE << 32) | 0x5EED,
                t=rng.integers(0, 2 ** 32, n, dtype=np.uint64), env_offset=rng.integers(0, 2 ** 32, n, dtype=np.uint64))


@pytest.mark.parametrize("game", GAMES)
def test_per_env_rows_with_bad_rows_among_them(game, hip_lib, oracle_lib):
    """mixed samples, salts, frames and holds; samples 0 and 4097, a negative salt, a salt that overflows, frames 0 and an illegal rest
    answer zeros and the others are answered -- the host form, and the device form on a caller's stream with the rows in HBM"""
    n, L = 24, len(LEGAL[game])
    g, states, rngs = _world(game, n, 400, hip_lib, oracle_lib)
    rows = _mixed_rows(game, n)
    rows["samples"][[1, 5]] = [0, 4097]
    rows["salt"][[7, 9, 10]] = [-1, 2 ** 32 - 2, 2 ** 32]
    rows["samples"][9] = 3                                    # (2^32 - 2) + 3 - 1 = 2^32: one too many
    rows["frames"][12] = 0
    rows["rest"][14] = 2 if game == "breakout" else 17
    bad = [1, 5, 7, 9, 10, 12, 14]
    want = expected_samples(oracle_lib, game, states, rngs, rows)
    good = np.setdiff1d(np.arange(n), bad)
    assert all((want[k][bad] == 0).all() for k in SAMPLE_FIELDS) and np.array_equal(want["samples"][good, 0], rows["samples"][good])
    args, per_env = sample_args(game, n, **rows)
    assert per_env and args.shape == (n, 9)
    host = Engine._samples_dict(g.reduce(_abi.QUERY_LOOKAHEAD_SAMPLES, args).reshape(n, L, 8))
    assert g.sample_chunks > 1
    assert_samples_equal(host, want, "%s per-env rows (host form)" % game)
    dev = Engine._samples_dict(_device_reduce(g, _abi.QUERY_LOOKAHEAD_SAMPLES, args, 8 * L).reshape(n, L, 8))
    assert_samples_equal(dev, want, "%s per-env rows (device form)" % game)


def test_per_env_rows_across_the_launch_seam(hip_lib, oracle_lib):
    """600 envs: per-env rows are budgeted as the largest valid row, 512 envs per launch, so the batch takes two launches of the
    sample kernel and two of the sum kernel (a thread per unit: 2 400 groups are cut into chunks, most of them empty for so few
    samples)"""
    game, n, L = "breakout", 600, 4
    g, states, rngs = _world(game, n, 400, hip_lib, oracle_lib)
    rows = _mixed_rows(game, n)
    rows["samples"][[3, 511, 512, 599]] = [0, 4, 4097, 2]
    want = expected_samples(oracle_lib, game, states, rngs, rows)
    assert (want["samples"][[3, 512]] == 0).all() and (want["samples"][[511, 599], 0] == [4, 2]).all() and (want["lost"][513:] > 0).any()
    args, _ = sample_args(game, n, **rows)
    got = Engine._samples_dict(_device_reduce(g, _abi.QUERY_LOOKAHEAD_SAMPLES, args, 8 * L).reshape(n, L, 8))
    assert g.sample_chunks > 1
    assert_samples_equal(got, want, "breakout, 600 per-env rows")


# ---------------------------------------------------------------- 4. shared bad values

@pytest.mark.parametrize("game", GAMES)
def test_shared_refusals(game, hip_lib, oracle_lib):
    from toybox_amd import hip
    g, _, _ = _world(game, 24, 400, hip_lib, oracle_lib)
    L = len(LEGAL[game])
    illegal = 2 if game == "breakout" else 17
    before = _snapshot(g)
    cases = {"samples 0": [8, 1, 0], "samples 4097": [8, 1, 4097], "salt -1": [8, 1, 4, -1], "salt 2^32": [8, 1, 1, 2 ** 32], "salt overflows": [8, 1, 4, 2 ** 32 - 3],
             "illegal rest": [8, 1, 2, 0, illegal], "frames 0": [0], "frames 1025": [1025], "hold 0": [8, 0], "ten arguments": [8, 1, 1, 0, -1, 0, 0, 0, 0, 0],
             "no arguments": []}
    o_dev = hip.malloc(24 * 8 * L * 8)
    fill = np.full((24, 8 * L), -7.0)
    try:
        hip.memcpy_htod(o_dev, fill, fill.nbytes)
        for what, args in cases.items():
            with pytest.raises(ToyboxAmdError) as ei:
                g.reduce(_abi.QUERY_LOOKAHEAD_SAMPLES, args)
            assert ei.value.code == _abi.E_INVALID, what
            with pytest.raises(ToyboxAmdError) as ei:
                g.reduce_device(_abi.QUERY_LOOKAHEAD_SAMPLES, o_dev, args)
            assert ei.value.code == _abi.E_INVALID, what
        g.sync()
        back = np.empty_like(fill)
        hip.memcpy_dtoh(back, o_dev, back.nbytes)
        assert np.array_equal(back, fill), "a refused query wrote to the output buffer"
    finally:
        g.sync()
        hip.free(o_dev)
    _assert_same_snapshot(_snapshot(g), before, "%s after the refusals" % game)
    assert g.reduce(_abi.QUERY_LOOKAHEAD_SAMPLES, [8]).shape == (24, 8 * L)                               # every default
    assert g.reduce(_abi.QUERY_LOOKAHEAD_SAMPLES, [8, 1, 4, 2 ** 32 - 4]).reshape(24, L, 8)[..., 0].tolist() == [[4] * L] * 24      # the largest salt that fits
    for name in GAMES:
        assert hip_lib.tbx_reduce_width(_abi.GAME_IDS[name], _abi.QUERY_LOOKAHEAD_SAMPLES) == 8 * len(LEGAL[name])


# ---------------------------------------------------------------- 5. nothing written

@pytest.mark.parametrize("game", GAMES)
def test_the_query_leaves_the_engine_untouched(game, hip_lib, oracle_lib):
    """state records, simulator RNGs, step outputs and scalars are byte-equal before and after the chunked, salted query, and the
    next synthetic step gives what an untouched twin gives"""
    n = 24
    g, twin = batch(hip_lib, game, n), batch(hip_lib, game, n)
    before = _snapshot(g)
    g.lookahead_samples(40, 9, hold=4, salt=1000, seed=3)
    assert g.sample_chunks > 1
    g.lookahead_samples(40, 1, hold=4, salt=5, rest=LEGAL[game][0])
    _assert_same_snapshot(_snapshot(g), before, game)
    for e in (g, twin):
        e.step_synthetic(1337, 400, auto_reset=True)
    _assert_same_snapshot(_snapshot(g), _snapshot(twin), "%s: the step after the queries" % game)
    g.close(); twin.close()


@pytest.mark.parametrize("game", GAMES)
def test_the_query_leaves_the_agent_layer_untouched(game, hip_lib, oracle_lib):
    n = 16
    case = Agent(game, n)
    g, o = case.make(hip_lib), case.make(oracle_lib)
    case.run(g, 0, 12); case.run(o, 0, 12)
    obs, before = read_buffer(g, _abi.BUF_AGENT_OBS, (n, 84, 84, 4)), _snapshot(g)
    got = g.lookahead_samples(24, 6, hold=4, salt=77, seed=11, t=12)
    assert np.array_equal(read_buffer(g, _abi.BUF_AGENT_OBS, (n, 84, 84, 4)), obs), "TBX_BUF_AGENT_OBS changed"
    _assert_same_snapshot(_snapshot(g), before, "%s with the agent layer" % game)
    assert_samples_equal(got, expected_samples(oracle_lib, game, g.get_states(), sim_rngs(g), dict(frames=24, hold=4, samples=6, salt=77, seed=11, t=12)),
                         "%s with the agent layer on: raw frames from the state as it stands" % game)
    rows_g, rows_o = case.run(g, 12, 16), case.run(o, 12, 16)
    for x, y in zip(rows_g, rows_o):
        for u, w in zip(x, y):
            assert np.array_equal(u, w), "%s: the agent steps after the query" % game
    g.close(); o.close()


# ---------------------------------------------------------------- 6. coverage, on the expected arrays

@pytest.mark.parametrize("game", GAMES)
def test_the_cases_cover_what_they_must(game, hip_lib, oracle_lib):
    """asserted on the expected arrays, so no test passes by avoiding the hard rows"""
    cov = coverage(_expected(game, "coverage", hip_lib, oracle_lib))
    n = WORLDS[game][0]
    need = ["spread", "scored"] + ([] if game == "gridworld" else ["some_lost", "ended", "all_lost"])
    assert cov["groups"] == n * len(LEGAL[game]) and not [k for k in need if not cov[k]], cov


@pytest.mark.parametrize("game", GAMES)
def test_the_salt_is_read(game, hip_lib, oracle_lib):
    """SpaceInvaders under fixed actions and Breakout under drawn ones (a ball start needs them): salt 1000 against salt 0 differs,
    on the expected arrays and on the device.  Default Amidar draws nothing and GridWorld has no game RNG: identical rows."""
    g, _, _ = _game_world(game, hip_lib, oracle_lib)
    _, frames, hold, _ = WORLDS[game]
    plain_name, salted_name, differ = SALT_PAIRS[game]
    cases = settings(game, frames, hold)
    plain, salted = _expected(game, plain_name, hip_lib, oracle_lib), _expected(game, salted_name, hip_lib, oracle_lib)
    got_plain, got_salted = _ask(g, cases[plain_name]), _ask(g, cases[salted_name])
    assert_samples_equal(got_plain, plain, "%s %s" % (game, plain_name))
    assert_samples_equal(got_salted, salted, "%s %s" % (game, salted_name))
    if differ:
        assert any(not np.array_equal(plain[k], salted[k]) for k in SAMPLE_FIELDS), "%s: the salt changes nothing in the expected rows" % game
        if game == "space_invaders":
            assert coverage(plain)["some_lost"] == 0 and coverage(salted)["some_lost"] > 0, "the salt alone splits groups"
    else:
        assert all(np.array_equal(plain[k], salted[k]) for k in SAMPLE_FIELDS)


# ---------------------------------------------------------------- 7. the adapters

def test_the_adapters(hip_lib):
    """lookahead_samples on both VecEnvs against the engine call: agent steps, action indices, the means and best_action"""
    from toybox_amd.envs import ToyboxPreprocVecEnv, ToyboxVecEnv
    game, n = "space_invaders", 16
    legal = LEGAL[game]
    rng = np.random.default_rng(0)
    for cls, skip in ((ToyboxPreprocVecEnv, 4), (ToyboxVecEnv, 1)):
        v = cls(game, n, seed=3, engine=Engine(game, n, lib=hip_lib))
        v.reset()
        for _ in range(20):
            v.step(rng.integers(0, v.action_space.n, n))
        v.step_async(rng.integers(0, v.action_space.n, n))        # a pending step ends first
        for objective in ("return", "survival"):
            got = v.lookahead_samples(steps=12, samples=6, rest=4, seed=5, t=2, salt=1000, objective=objective)
            assert v._in_flight is None and getattr(v, "_pending", None) is None
            want = v.engine.lookahead_samples(12 * skip, 6, hold=skip, salt=1000, rest=legal[4], seed=5, t=2)
            assert_samples_equal(got, want, "%s.lookahead_samples" % cls.__name__)
            assert np.array_equal(got["ret_mean"], want["ret_sum"] / 6.0) and np.array_equal(got["lost_frac"], want["lost"] / 6.0)
            assert np.array_equal(got["ended_frac"], want["ended"] / 6.0)
            assert np.array_equal(got["best_action"], best_action(want, objective)), objective
        drawn = v.lookahead_samples(steps=12, samples=6)
        assert_samples_equal(drawn, v.engine.lookahead_samples(12 * skip, 6, hold=skip), "%s, drawn, no salt" % cls.__name__)
        v.close()


def test_batch_intervention_mirrors_the_engine(hip_lib, oracle_lib):
    from toybox_amd.interventions import BatchIntervention
    game, n, first, count = "breakout", 24, 5, 11
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    salt = np.resize([0, 9, 1000], n)
    whole = g.lookahead_samples(48, 5, hold=4, salt=salt, seed=2)
    with BatchIntervention(g, first, count) as bi:
        part = bi.lookahead_samples(48, 5, hold=4, salt=salt[first:first + count], seed=2)
    for k in SAMPLE_FIELDS:
        assert np.array_equal(part[k], whole[k][first:first + count]), k
