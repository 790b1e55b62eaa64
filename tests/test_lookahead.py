"""Lookahead (TBX_QUERY_LOOKAHEAD / _ALL), the part that needs no GPU: the constants, the argument shaping of Engine.lookahead, and
the yardstick of tests/test_gpu_lookahead.py under test itself, over the CPU checker alone (tests/lookahead_replay.py): a clone
continues like its original, expected() composes over time, the freeze rule holds, and the cases cover what they must."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from fork_replay import sim_rngs, states_bytes
from lookahead_replay import (FIELDS, assert_coverage, assert_fields_equal, batch, clone, clone_of, coverage, expected, merge_coverage, play,
                              schedule_columns)
from support import LEGAL, synthetic_actions
from toybox_amd import Engine, ToyboxAmdError, _abi
from toybox_amd.engine import lookahead_args

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
HEADER = open(os.path.join(ROOT, "include", "toybox_amd.h")).read()
N, H = 96, 300


def test_header_and_python_agree_on_the_constants():
    want = {"TBX_LOOKAHEAD_MAX_FRAMES": (_abi.LOOKAHEAD_MAX_FRAMES, 1024), "TBX_QUERY_LOOKAHEAD": (_abi.QUERY_LOOKAHEAD, 150),
            "TBX_QUERY_LOOKAHEAD_ALL": (_abi.QUERY_LOOKAHEAD_ALL, 151)}
    for name, (py, value) in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, HEADER)
        assert m and int(m.group(1)) == py == value, name


def test_the_abi_has_no_new_symbols_and_keeps_its_version():
    assert len(re.findall(r"\btbx_\w*lookahead\w*\s*\(", HEADER)) == 0, "the lookahead goes through tbx_reduce"
    assert re.search(r"#define\s+TBX_ABI_VERSION\s+1\b", HEADER)


def test_the_checker_has_no_lookahead(oracle_lib):
    """the expected values cannot come from the checker's own: it answers "unknown query" """
    with Engine("breakout", 4, lib=oracle_lib) as e:
        for call in (lambda: e.lookahead(8), lambda: e.lookahead_all(8)):
            with pytest.raises(ToyboxAmdError) as ei:
                call()
            assert ei.value.code == _abi.E_INVALID


# ---------------------------------------------------------------- the argument shaping

def test_args_defaults_are_one_shared_row():
    args, per_env = lookahead_args(8, 16)
    assert per_env is False and args == [16.0, 1.0, -1.0, -1.0, 0.0, 0.0, 0.0, 0.0]


def test_args_scalars_and_the_seed_split():
    seed = (0xDEADBEEF << 32) | 0x12345678
    args, per_env = lookahead_args(8, 300, hold=4, first=3, rest=0, seed=seed, t=77, env_offset=4096)
    assert per_env is False
    assert args == [300.0, 4.0, 3.0, 0.0, float(0x12345678), float(0xDEADBEEF), 77.0, 4096.0]
    assert lookahead_args(8, 1, seed=2 ** 64 - 1)[0][4:6] == [float(2 ** 32 - 1)] * 2


def test_args_per_env_rows():
    n = 6
    frames = np.array([1, 2, 4, 299, 300, 1024])
    args, per_env = lookahead_args(n, frames, hold=7, first=np.array([0, 1, 3, 4, -1, 0]), seed=np.arange(n, dtype=np.uint64) << np.uint64(33), t=5)
    assert per_env is True and args.shape == (n, 8) and args.dtype == np.float64
    assert np.array_equal(args[:, 0], frames) and np.array_equal(args[:, 1], np.full(n, 7.0))
    assert np.array_equal(args[:, 2], [0, 1, 3, 4, -1, 0]) and np.array_equal(args[:, 3], np.full(n, -1.0))
    assert np.array_equal(args[:, 4], np.zeros(n)) and np.array_equal(args[:, 5], 2.0 * np.arange(n)) and np.array_equal(args[:, 6], np.full(n, 5.0))
    # per-env rows are checked on the device (a bad row answers zeros), not here
    args, per_env = lookahead_args(n, np.array([0, 1, 2, 3, 4, 2000]), hold=np.zeros(n, np.int64))
    assert per_env is True and args[0, 0] == 0 and args[5, 0] == 2000


@pytest.mark.parametrize("bad", [dict(frames=0), dict(frames=1025), dict(frames=8, hold=0), dict(frames=8, seed=-1), dict(frames=8, seed=2 ** 64),
                                 dict(frames=8, t=2 ** 32), dict(frames=8, env_offset=-3), dict(frames=np.ones(5)), dict(frames=8, first=np.zeros(7)),
                                 dict(frames=8, rest=np.zeros((6, 1)))])
def test_args_range_and_shape_errors(bad):
    with pytest.raises(ValueError):
        lookahead_args(6, **bad)


def test_the_adapters_map_action_indices_and_steps(monkeypatch):
    """ToyboxVecEnv.lookahead: frames = steps, hold = 1; ToyboxPreprocVecEnv.lookahead: frames = steps x skip, hold = skip; action
    indices become ALE ids; a pending step ends first"""
    from toybox_amd.envs import vec_env

    class FakeEngine:
        def lookahead(self, frames, **kw):
            self.call = ("one", frames, kw)

        def lookahead_all(self, frames, **kw):
            self.call = ("all", frames, kw)

    lut = np.asarray(LEGAL["space_invaders"], np.int32)
    for cls, skip in ((vec_env.ToyboxVecEnv, 1), (vec_env.ToyboxPreprocVecEnv, 4)):
        v = object.__new__(cls)
        v.num_envs, v._in_flight, v._pending, v.engine, v._lut, v._action_set, v._skip = 3, None, None, FakeEngine(), lut, list(lut), 4
        waited = []
        monkeypatch.setattr(cls, "step_wait", lambda self: waited.append(1) or setattr(self, "_in_flight", None))
        v.lookahead(5, first=4, rest=np.array([0, 5, 2]), seed=9, t=3)
        kind, frames, kw = v.engine.call
        assert (kind, frames, kw["hold"], kw["first"], kw["seed"], kw["t"]) == ("one", 5 * skip, skip, 11, 9, 3) and np.array_equal(kw["rest"], [0, 12, 3])
        v.lookahead(5, all_actions=True)
        kind, frames, kw = v.engine.call
        assert (kind, frames, kw["hold"], kw["rest"]) == ("all", 5 * skip, skip, None) and "first" not in kw
        assert not waited
        v._in_flight = object()
        v.lookahead(1)
        assert waited == [1]
        with pytest.raises(AssertionError):
            v.lookahead(1, first=6)


# ---------------------------------------------------------------- the yardstick, on the checker alone

@pytest.fixture(scope="module")
def batches(oracle_lib):
    """game -> (state records, simulator RNGs) of the input recipe at N = 96; built once, read only"""
    out = {}
    for game in GAMES:
        e = batch(oracle_lib, game, N)
        out[game] = (e.get_states(), sim_rngs(e))
        e.close()
    return out


@pytest.mark.parametrize("game", GAMES)
def test_a_clone_continues_like_its_original(game, oracle_lib):
    """state records + simulator RNGs are the whole env: 120 frames with auto-reset (which draws from the simulator RNG) leave the
    same bytes, and every step the same lives, score and done"""
    o = batch(oracle_lib, game, N)
    c = clone_of(oracle_lib, o)
    assert np.array_equal(states_bytes(o), states_bytes(c)) and np.array_equal(sim_rngs(o), sim_rngs(c))
    resets = 0
    for t in range(120):
        a = synthetic_actions(game, N, 1000 + t, seed=3)
        ro, rc = o.step(a, auto_reset=True), c.step(a, auto_reset=True)
        for k in (1, 2, 3):
            assert np.array_equal(ro[k], rc[k]), (t, k)
        resets += int(ro[1].sum())
    assert resets > 0, "no game ended: the simulator RNG was never drawn from"
    assert np.array_equal(states_bytes(o), states_bytes(c)) and np.array_equal(sim_rngs(o), sim_rngs(c))
    o.close(); c.close()


@pytest.mark.parametrize("game", GAMES)
def test_expected_composes_over_time(game, batches, oracle_lib):
    """expected(H1 + H2) = expected(H1), then expected(H2) from the stepped clone with the counter moved on, for the envs that have
    not ended at H1"""
    states, rngs = batches[game]
    h1, h2, sched = 60, 90, dict(seed=77, t=5, env_offset=1000)
    whole = expected(oracle_lib, game, states, rngs, dict(frames=h1 + h2, **sched))
    e = clone(oracle_lib, game, states, rngs)
    a = play(e, game, schedule_columns(N, frames=h1, **sched))
    b = play(e, game, schedule_columns(N, frames=h2, **dict(sched, t=5 + h1)))
    going = a["lives"] > 0
    assert going.any() and (~going).any()
    assert np.array_equal(whole["ret"][going], (a["ret"] + b["ret"])[going])
    for k in ("score", "lives"):
        assert np.array_equal(whole[k][going], b[k][going])
    assert np.array_equal(whole["frames_run"][going], (h1 + b["frames_run"])[going])
    lost = np.where(a["life_lost_at"] >= 0, a["life_lost_at"], np.where(b["life_lost_at"] >= 0, h1 + b["life_lost_at"], -1))
    assert np.array_equal(whole["life_lost_at"][going], lost[going])    # (b counts against the lives at H1: the start's, unless a lost one)
    for k in FIELDS:                                           # ended inside H1: the longer horizon changes nothing
        assert np.array_equal(whole[k][~going], a[k][~going]), k
    e.close()


@pytest.mark.parametrize("game", GAMES)
def test_the_freeze_rule(game, batches, oracle_lib):
    """an ended env's row is what it was at its last frame: run = the first frame with lives <= 0, plus one; the fields equal those of
    a horizon cut exactly there"""
    states, rngs = batches[game]
    long = expected(oracle_lib, game, states, rngs, dict(frames=H, seed=1))
    ended = long["lives"] <= 0
    assert ended.any()
    assert (long["frames_run"][ended] <= H).all() and (long["frames_run"][~ended] == H).all() and (long["frames_run"] >= 1).all()
    cut = expected(oracle_lib, game, states, rngs, dict(frames=np.maximum(long["frames_run"], 1), seed=1))
    assert_fields_equal(cut, long, "%s: horizon cut at the end of every env's run" % game)
    one_less = np.maximum(long["frames_run"] - 1, 1)
    before = expected(oracle_lib, game, states, rngs, dict(frames=one_less, seed=1))
    alive_before = ended & (long["frames_run"] > 1)
    assert (before["lives"][alive_before] > 0).all(), "an env ended before the frame its row names"


@pytest.mark.parametrize("game", GAMES)
def test_refused_rows_are_zero_and_leave_the_others(game, batches, oracle_lib):
    states, rngs = batches[game]
    frames = np.full(N, 40)
    frames[3], frames[10] = 0, 1025
    first = np.full(N, -1)
    first[5] = 2 if game == "breakout" else 17                # (2 = UP is no Breakout action)
    hold = np.ones(N, np.int64)
    hold[7] = 0
    got = expected(oracle_lib, game, states, rngs, dict(frames=frames, hold=hold, first=first, seed=4))
    plain = expected(oracle_lib, game, states, rngs, dict(frames=40, seed=4))
    bad = np.isin(np.arange(N), [3, 5, 7, 10])
    for k in FIELDS:
        assert (got[k][bad] == 0).all() and np.array_equal(got[k][~bad], plain[k][~bad]), k


@pytest.mark.parametrize("game", GAMES)
def test_the_cases_cover_what_they_must(game, batches, oracle_lib):
    """the coverage conditions of the GPU module's cases, on the checker: an env ends inside the horizon, one runs all of it, one
    scores, one loses a life without ending -- over the cases together"""
    states, rngs = batches[game]
    total = {}
    for sched in (dict(frames=H, seed=1337), dict(frames=H, hold=4, rest=0)):
        merge_coverage(total, coverage(expected(oracle_lib, game, states, rngs, sched, all_actions=True), H))
    assert_coverage(game, total)
    alone = coverage(expected(oracle_lib, game, states, rngs, dict(frames=H, seed=1337)), H)
    assert_coverage(game, alone)                              # first = rest = -1 alone meets them too
