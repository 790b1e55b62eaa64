"""The sampled lookahead (TBX_QUERY_LOOKAHEAD_SAMPLES), the part that needs no GPU: the constants, the argument shaping, the
sample seeds, the adapters' mapping and best_action rule, and the yardstick of tests/test_gpu_samples.py under test itself over
the CPU checker alone (tests/sample_replay.py): one unsalted sample is the all-actions lookahead's own replay, a refused row is
zeros, the sums do not depend on the order of the futures, and the GPU module's cases cover what they must."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from fork_replay import sim_rngs
from lookahead_replay import batch, expected
from sample_replay import SALT_PAIRS, WORLDS, aggregate, best_action, coverage, expected_samples, play_samples, settings
from support import LEGAL, splitmix64
from toybox_amd import Engine, ToyboxAmdError, _abi
from toybox_amd.engine import SAMPLE_FIELDS, sample_args, sample_seed

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
HEADER = open(os.path.join(ROOT, "include", "toybox_amd.h")).read()


def test_header_and_python_agree_on_the_constants():
    want = {"TBX_QUERY_LOOKAHEAD_SAMPLES": (_abi.QUERY_LOOKAHEAD_SAMPLES, 154), "TBX_LOOKAHEAD_MAX_SAMPLES": (_abi.LOOKAHEAD_MAX_SAMPLES, 4096),
            "TBX_OPT_SAMPLE_CHUNKS": (_abi.OPT_SAMPLE_CHUNKS, 106)}
    for name, (py, value) in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, HEADER)
        assert m and int(m.group(1)) == py == value, name
    assert re.search(r"#define\s+TBX_QUERY_LOOKAHEAD_SAMPLES\s+154\s*/\*.*->\s*8\s*\*\s*n_legal", HEADER), "the width stands on the #define line"
    assert len(re.findall(r"\btbx_\w*(lookahead|sample)\w*\s*\(", HEADER)) == 0, "the query goes through tbx_reduce: no new symbol"
    assert re.search(r"#define\s+TBX_ABI_VERSION\s+1\b", HEADER)
    assert SAMPLE_FIELDS == ("samples", "ret_sum", "ret_min", "ret_max", "lives_sum", "lost", "ended", "safe_frames_sum")


def test_the_checker_does_not_have_the_query(oracle_lib):
    """the expected values cannot come from the checker's own: it answers "unknown query" """
    with Engine("breakout", 4, lib=oracle_lib) as e:
        for call in (lambda: e.lookahead_samples(8, 2), lambda: e.reduce(154, [8])):
            with pytest.raises(ToyboxAmdError) as ei:
                call()
            assert ei.value.code == _abi.E_INVALID


def test_sample_seed_is_splitmix64_of_the_sum():
    for seed, s in ((0, 0), (77, 3), ((0xABCDE << 32) | 0x1234567, 32), (2 ** 64 - 1, 0), (2 ** 64 - 1, 5), (2 ** 64 - 3, 4095)):
        want = int(splitmix64(np.uint64((seed + s) % 2 ** 64)))
        assert sample_seed(seed, s) == want and 0 <= sample_seed(seed, s) < 2 ** 64, (seed, s)
    assert sample_seed(2 ** 64 - 1, 1) == sample_seed(0, 0), "the sum wraps at 2^64"
    assert sample_seed(5, 1) != sample_seed(5, 0) + 1 and sample_seed(5, 1) == sample_seed(6, 0)


def test_args_defaults_and_scalars():
    assert sample_args("breakout", 8, 16, 1) == ([16.0, 1.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0], False)
    seed = (0xDEADBEEF << 32) | 0x12345678
    args, per_env = sample_args("space_invaders", 8, 300, 64, hold=4, salt=1000, rest=11, seed=seed, t=77, env_offset=4096)
    assert per_env is False and args == [300.0, 4.0, 64.0, 1000.0, 11.0, float(0x12345678), float(0xDEADBEEF), 77.0, 4096.0]
    assert sample_args(_abi.GAME_IDS["amidar"], 8, 8, 4096, salt=2 ** 32 - 4096)[0][2:4] == [4096.0, float(2 ** 32 - 4096)], "the largest salt that fits"
    assert sample_args("gridworld", 8, 8, 4096, salt=0)[0][3] == 0.0


def test_args_per_env_rows():
    n = 6
    samples, salt = np.array([1, 5, 0, 4097, 8, 8]), np.array([0, 7, 0, 0, -1, 2 ** 32 - 3])
    args, per_env = sample_args("breakout", n, np.array([1, 2, 4, 299, 0, 1024]), samples, hold=7, salt=salt, seed=np.arange(n, dtype=np.uint64) << np.uint64(33), t=5)
    assert per_env is True and args.shape == (n, 9) and args.dtype == np.float64
    assert args[:, 0].tolist() == [1, 2, 4, 299, 0, 1024] and args[:, 1].tolist() == [7] * n
    # per-env rows are checked on the device (a bad row answers zeros), not here
    assert args[:, 2].tolist() == samples.tolist() and args[:, 3].tolist() == salt.tolist() and args[:, 4].tolist() == [-1] * n
    assert args[:, 5].tolist() == [0] * n and args[:, 6].tolist() == [2.0 * i for i in range(n)] and args[:, 7].tolist() == [5] * n
    args, per_env = sample_args("breakout", n, 8, 3, salt=np.arange(n))
    assert per_env is True and args[:, 2].tolist() == [3] * n and args[:, 3].tolist() == list(range(n))


@pytest.mark.parametrize("bad", [dict(frames=0, samples=1), dict(frames=1025, samples=1), dict(frames=8, samples=1, hold=0), dict(frames=8, samples=0),
                                 dict(frames=8, samples=4097), dict(frames=8, samples=2, salt=-1), dict(frames=8, samples=2, salt=2 ** 32),
                                 dict(frames=8, samples=2, salt=2 ** 32 - 1), dict(frames=8, samples=4096, salt=2 ** 32 - 4095), dict(frames=8, samples=1, rest=2),
                                 dict(frames=8, samples=1, seed=2 ** 64), dict(frames=8, samples=1, t=2 ** 32), dict(frames=8, samples=1, env_offset=-3),
                                 dict(frames=8, samples=np.ones(5)), dict(frames=8, samples=2, salt=np.zeros((6, 1))), dict(frames=np.ones(5), samples=1)])
def test_sample_args_range_and_shape_errors(bad):
    with pytest.raises(ValueError):
        sample_args("breakout", 6, **bad)
    assert sample_args("breakout", 6, 8, 1, salt=2 ** 32 - 1)[0][3] == float(2 ** 32 - 1), "one sample: the largest salt"


def _rows(L, **cells):
    """three envs: every field zero but the cells named, field=(env, action, value)"""
    out = {k: np.zeros((3, L), np.int64) for k in SAMPLE_FIELDS}
    out["samples"][:] = 4
    for k, triples in cells.items():
        for i, a, v in triples:
            out[k][i, a] = v
    return out


def test_best_action_rule_on_hand_made_rows():
    from toybox_amd.envs.vec_env import sample_best_action
    L = 6
    # env 0: action 4 has the largest ret_sum but loses a life in every future; 2 never loses and keeps the most safe frames
    # env 1: actions 2 and 5 tie in everything -> the smaller index; env 2: equal ret_sum, 3 loses less than 1
    rows = _rows(L, ret_sum=[(0, 4, 120), (0, 2, 40), (1, 2, 10), (1, 5, 10), (2, 1, 50), (2, 3, 50)],
                 lost=[(0, 0, 1), (0, 1, 1), (0, 3, 1), (0, 4, 4), (0, 5, 1), (2, 0, 2), (2, 1, 2), (2, 2, 2), (2, 3, 1), (2, 4, 2), (2, 5, 2)],
                 safe_frames_sum=[(0, a, 30) for a in range(L)] + [(0, 2, 64)] + [(1, a, 64) for a in range(L)] + [(2, a, 20) for a in range(L)])
    assert sample_best_action(rows, "return").tolist() == [4, 2, 3] == best_action(rows, "return").tolist()
    assert sample_best_action(rows, "survival").tolist() == [2, 2, 3] == best_action(rows, "survival").tolist()
    # the third key: equal ret_sum and lost, more safe frames wins under "return"; under "survival" ret_sum is the last key
    rows = _rows(L, ret_sum=[(0, a, 7) for a in range(L)] + [(1, 0, 5), (1, 3, 9)], safe_frames_sum=[(0, 3, 12), (0, 5, 12), (1, 0, 8), (1, 3, 8)])
    assert sample_best_action(rows, "return").tolist() == [3, 3, 0] == best_action(rows, "return").tolist()
    assert sample_best_action(rows, "survival").tolist() == [3, 3, 0] == best_action(rows, "survival").tolist()
    rng = np.random.default_rng(1)
    rows = {k: rng.integers(0, 3, (50, L)) for k in SAMPLE_FIELDS}
    for objective in ("return", "survival"):
        assert np.array_equal(sample_best_action(rows, objective), best_action(rows, objective)), objective
    with pytest.raises(ValueError):
        sample_best_action(rows, "score")


def test_the_adapters_map_action_indices_and_steps(monkeypatch):
    """ToyboxVecEnv.lookahead_samples: frames = steps, hold = 1; ToyboxPreprocVecEnv: frames = steps x skip, hold = skip; `rest` an
    action index going in; the means and best_action are added; a pending step ends first"""
    from toybox_amd.envs import vec_env
    lut = np.asarray(LEGAL["space_invaders"], np.int32)
    L = len(lut)

    class FakeEngine:
        legal_actions = list(lut)

        def lookahead_samples(self, frames, samples, **kw):
            self.call = (frames, samples, kw)
            out = _rows(L, ret_sum=[(0, 4, 120), (0, 2, 40)], lost=[(0, a, 1) for a in (0, 1, 3, 5)] + [(0, 4, 4)], ended=[(0, 4, 2)])
            out["samples"][2] = 0                                 # a refused env: its means are 0, not a division by 0
            return out

    for cls, skip in ((vec_env.ToyboxVecEnv, 1), (vec_env.ToyboxPreprocVecEnv, 4)):
        v = object.__new__(cls)
        v.num_envs, v._in_flight, v._pending, v.engine, v._lut, v._action_set, v._skip = 3, None, None, FakeEngine(), lut, list(lut), 4
        waited = []
        monkeypatch.setattr(cls, "step_wait", lambda self: waited.append(1) or setattr(self, "_in_flight", None))
        out = v.lookahead_samples(5, 4, rest=4, seed=9, t=3, salt=1000)
        frames, samples, kw = v.engine.call
        assert (frames, samples, kw["hold"], kw["rest"], kw["seed"], kw["t"], kw["salt"]) == (5 * skip, 4, skip, 11, 9, 3, 1000)
        assert out["ret_mean"][0].tolist() == [0, 0, 10.0, 0, 30.0, 0] and out["lost_frac"][0, 4] == 1.0 and out["ended_frac"][0, 4] == 0.5
        assert (out["ret_mean"][2] == 0).all() and np.isfinite(out["lost_frac"]).all()
        assert out["best_action"].tolist() == [4, 0, 0]
        out = v.lookahead_samples(5, 4, objective="survival")
        assert out["best_action"].tolist() == [2, 0, 0] and v.engine.call[2]["rest"] is None and v.engine.call[2]["salt"] == 0
        assert not waited
        v._in_flight = object()
        v.lookahead_samples(1, 1)
        assert waited == [1]
        with pytest.raises(AssertionError):
            v.lookahead_samples(1, 1, rest=6)
        with pytest.raises(ValueError):
            v.lookahead_samples(1, 1, objective="score")


# ---------------------------------------------------------------- the yardstick, on the checker alone

@pytest.fixture(scope="module")
def batches(oracle_lib):
    out = {}
    for game in GAMES:
        n, _, _, batch_frames = WORLDS[game]
        e = batch(oracle_lib, game, n, frames=batch_frames)
        out[game] = (e.get_states(), sim_rngs(e))
        e.close()
    return out


@pytest.mark.parametrize("game", GAMES)
def test_one_unsalted_sample_is_the_all_actions_lookahead_replay(game, batches, oracle_lib):
    states, rngs = batches[game]
    sched = dict(frames=60, hold=4, rest=-1, seed=(3 << 40) | 9, t=2 ** 32 - 2, env_offset=11)
    got = expected_samples(oracle_lib, game, states, rngs, dict(sched, samples=1, salt=0))
    one = expected(oracle_lib, game, states, rngs, dict(sched, seed=sample_seed(sched["seed"], 0)), all_actions=True)
    ret = one["ret"].astype(np.int64)
    assert (got["samples"] == 1).all()
    for k in ("ret_sum", "ret_min", "ret_max"):
        assert np.array_equal(got[k], ret), k
    assert np.array_equal(got["lives_sum"], one["lives"]) and np.array_equal(got["lost"], one["life_lost_at"] >= 0)
    assert np.array_equal(got["ended"], one["lives"] <= 0)
    assert np.array_equal(got["safe_frames_sum"], np.where(one["life_lost_at"] < 0, one["frames_run"], one["life_lost_at"]))


def test_refused_rows_are_zero_and_leave_the_others(batches, oracle_lib):
    game = "breakout"
    states, rngs = batches[game]
    n = len(states)
    samples, salt, frames = np.full(n, 3), np.full(n, 9), np.full(n, 24)
    samples[[2, 3]] = [0, 4097]
    salt[[5, 6]] = [-1, 2 ** 32 - 2]
    frames[8] = 1025
    got = expected_samples(oracle_lib, game, states, rngs, dict(frames=frames, hold=4, samples=samples, salt=salt, rest=0, seed=4))
    plain = expected_samples(oracle_lib, game, states, rngs, dict(frames=24, hold=4, samples=3, salt=9, rest=0, seed=4))
    bad = np.isin(np.arange(n), [2, 3, 5, 6, 8])
    for k in SAMPLE_FIELDS:
        assert (got[k][bad] == 0).all() and np.array_equal(got[k][~bad], plain[k][~bad]), k
    assert (plain["samples"] == 3).all()


@pytest.mark.parametrize("game", ["breakout", "space_invaders"])
def test_the_sums_do_not_depend_on_the_order_of_the_futures(game, batches, oracle_lib):
    states, rngs = batches[game]
    samples = np.resize([6, 3, 1, 5], len(states))
    _, frames, hold, _ = WORLDS[game]
    leaves, active = play_samples(oracle_lib, game, states, rngs, dict(frames=frames, hold=hold, samples=samples, salt=1000, rest=-1, seed=21))
    want = aggregate(leaves, active)
    assert np.array_equal(want["samples"], np.tile(samples[:, None], (1, len(LEGAL[game])))) and (want["ret_min"] < want["ret_max"]).any()
    for order in ([5, 4, 3, 2, 1, 0], [3, 0, 5, 1, 4, 2]):
        got = aggregate(leaves, active, order)
        for k in SAMPLE_FIELDS:
            assert np.array_equal(got[k], want[k]), (k, order)


# ---------------------------------------------------------------- the GPU module's cases cover what they must

@pytest.mark.parametrize("game", GAMES)
def test_the_coverage_case_shows_what_it_must(game, batches, oracle_lib):
    """samples 8, rest drawn, seed 77: every game but GridWorld shows a group whose futures differ in their return, one where some
    but not all futures lost a life, one with an ended future and one where every future lost a life; GridWorld a spread and a
    scored group"""
    states, rngs = batches[game]
    _, frames, hold, _ = WORLDS[game]
    cov = coverage(expected_samples(oracle_lib, game, states, rngs, settings(game, frames, hold)["coverage"]))
    print(game, cov)
    need = ["spread", "scored"] + ([] if game == "gridworld" else ["some_lost", "ended", "all_lost"])
    assert cov["groups"] == len(states) * len(LEGAL[game]) and not [k for k in need if not cov[k]], cov


@pytest.mark.parametrize("game", ["space_invaders", "amidar"])
def test_the_salt_pair_on_the_checker(game, batches, oracle_lib):
    """SpaceInvaders: under fixed actions the salt alone spreads the futures; default Amidar draws nothing: identical rows"""
    states, rngs = batches[game]
    _, frames, hold, _ = WORLDS[game]
    plain_name, salted_name, differ = SALT_PAIRS[game]
    cases = settings(game, frames, hold)
    plain, salt = (expected_samples(oracle_lib, game, states, rngs, cases[k]) for k in (plain_name, salted_name))
    print(game, coverage(plain), coverage(salt))
    assert coverage(plain)["spread"] == 0 and coverage(plain)["some_lost"] == 0, "fixed actions, the RNG as it stands: eight equal futures"
    if differ:
        assert coverage(salt)["some_lost"] > 0 and coverage(salt)["spread"] > 0
    else:
        assert all(np.array_equal(plain[k], salt[k]) for k in SAMPLE_FIELDS)
