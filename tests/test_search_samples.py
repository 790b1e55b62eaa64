"""The search over sampled futures (TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES), the part that needs no GPU: the constants, the argument
shaping, the adapters' mapping, and the yardstick of tests/test_gpu_search_samples.py under test itself over the CPU checker alone
(tests/search_samples_replay.py), held to the older yardsticks: at depth 1 it is the sampled lookahead's replay, with one sample and a
fixed `rest` every plan's sums are the five fields of the search's replay folded, and the rows do not depend on the order in which
the futures are added."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from fork_replay import sim_rngs
from lookahead_replay import FIELDS, batch
from sample_replay import expected_samples
from search_replay import play_all_codes
from search_samples_replay import ROW_FIELDS, aggregate, columns, expected_search_samples, pick, play_all, valid_rows
from support import LEGAL
from toybox_amd import Engine, ToyboxAmdError, _abi
from toybox_amd.engine import SAMPLE_FIELDS, sample_seed, search_args, search_samples_args

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
HEADER = open(os.path.join(ROOT, "include", "toybox_amd.h")).read()


def test_header_and_python_agree_on_the_constants():
    want = {"TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES": (_abi.QUERY_LOOKAHEAD_SEARCH_SAMPLES, 155), "TBX_LOOKAHEAD_MAX_LEAVES": (_abi.LOOKAHEAD_MAX_LEAVES, 65536),
            "TBX_OPT_SEARCH_SAMPLES_CHUNKS": (_abi.OPT_SEARCH_SAMPLES_CHUNKS, 107), "TBX_OPT_SEARCH_SAMPLES_LAUNCHES": (_abi.OPT_SEARCH_SAMPLES_LAUNCHES, 108)}
    for name, (py, value) in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, HEADER)
        assert m and int(m.group(1)) == py == value, name
    assert re.search(r"#define\s+TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES\s+155\s*/\*.*->\s*9\s*\*\s*n_legal", HEADER), "the width stands on the #define line"
    assert len(re.findall(r"\btbx_\w*(lookahead|sample|search)\w*\s*\(", HEADER)) == 0, "the query goes through tbx_reduce: no new symbol"
    assert re.search(r"#define\s+TBX_ABI_VERSION\s+1\b", HEADER)


def test_the_checker_does_not_have_the_query(oracle_lib):
    """the expected values cannot come from the checker's own: it answers "unknown query" """
    with Engine("breakout", 4, lib=oracle_lib) as e:
        for call in (lambda: e.lookahead_search_samples(8, 2, 2), lambda: e.reduce(_abi.QUERY_LOOKAHEAD_SEARCH_SAMPLES, [8])):
            with pytest.raises(ToyboxAmdError) as ei:
                call()
            assert ei.value.code == _abi.E_INVALID


def test_args_defaults_and_scalars():
    assert search_samples_args("breakout", 8, 16, 1, 1) == ([16.0, 1.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0], False)
    seed = (0xDEADBEEF << 32) | 0x12345678
    args, per_env = search_samples_args("space_invaders", 8, 300, 2, 64, hold=4, objective="survival", salt=1000, rest=11, seed=seed, t=77, env_offset=4096)
    assert per_env is False and args == [300.0, 4.0, 2.0, 1.0, 11.0, float(0x12345678), float(0xDEADBEEF), 77.0, 4096.0, 64.0, 1000.0]
    assert args[:9] == search_args("space_invaders", 8, 300, 4, 2, "survival", 11, seed, 77, 4096)[0], "columns 0 .. 8 stand where the search's stand"
    # exactly at the cap of n_legal ** depth * samples: 16 x 4096 and 64 x 1024 are 65536
    assert search_samples_args("breakout", 8, 8, 2, 4096)[0][9] == 4096.0 and search_samples_args(_abi.GAME_IDS["breakout"], 8, 8, 3, 1024)[0][9] == 1024.0
    assert search_samples_args("amidar", 8, 8, 1, 4096, salt=2 ** 32 - 4096)[0][9:] == [4096.0, float(2 ** 32 - 4096)], "the largest salt that fits"


def test_args_per_env_rows():
    n = 6
    depth, samples, salt = np.array([1, 2, 0, 7, 3, 2]), np.array([1, 5, 0, 4097, 8, 8]), np.array([0, 7, 0, 0, -1, 2 ** 32 - 3])
    args, per_env = search_samples_args("breakout", n, np.array([1, 2, 4, 299, 0, 1024]), depth, samples, hold=7, objective=np.array([0, 1, 2, 0, 1, 0]), salt=salt,
                                        seed=np.arange(n, dtype=np.uint64) << np.uint64(33), t=5)
    assert per_env is True and args.shape == (n, 11) and args.dtype == np.float64
    # per-env rows are checked on the device (a bad row answers zeros), not here
    assert args[:, 0].tolist() == [1, 2, 4, 299, 0, 1024] and args[:, 1].tolist() == [7] * n and args[:, 2].tolist() == depth.tolist()
    assert args[:, 3].tolist() == [0, 1, 2, 0, 1, 0] and args[:, 4].tolist() == [-1] * n and args[:, 5].tolist() == [0] * n
    assert args[:, 6].tolist() == [2.0 * i for i in range(n)] and args[:, 7].tolist() == [5] * n and args[:, 8].tolist() == [0] * n
    assert args[:, 9].tolist() == samples.tolist() and args[:, 10].tolist() == salt.tolist()
    args, per_env = search_samples_args("breakout", n, 8, 2, 3, salt=np.arange(n))
    assert per_env is True and args[:, 2].tolist() == [2] * n and args[:, 9].tolist() == [3] * n and args[:, 10].tolist() == list(range(n))
    args, per_env = search_samples_args("breakout", n, 8, 2, np.arange(n))
    assert per_env is True and args[:, 9].tolist() == list(range(n)) and args[:, 10].tolist() == [0] * n


@pytest.mark.parametrize("bad", [dict(frames=0, depth=1, samples=1), dict(frames=1025, depth=1, samples=1), dict(frames=8, depth=1, samples=1, hold=0),
                                 dict(frames=8, depth=0, samples=1), dict(frames=8, depth=7, samples=1), dict(frames=8, depth=2, samples=0),
                                 dict(frames=8, depth=2, samples=4097), dict(frames=8, depth=3, samples=1025), dict(frames=8, depth=6, samples=17),
                                 dict(frames=8, depth=2, samples=2, objective=2), dict(frames=8, depth=2, samples=2, objective="score"),
                                 dict(frames=8, depth=2, samples=2, salt=-1), dict(frames=8, depth=2, samples=2, salt=2 ** 32),
                                 dict(frames=8, depth=2, samples=2, salt=2 ** 32 - 1), dict(frames=8, depth=2, samples=4096, salt=2 ** 32 - 4095),
                                 dict(frames=8, depth=2, samples=1, rest=2), dict(frames=8, depth=2, samples=1, seed=2 ** 64), dict(frames=8, depth=2, samples=1, t=2 ** 32),
                                 dict(frames=8, depth=2, samples=np.ones(5)), dict(frames=8, depth=2, samples=2, salt=np.zeros((6, 1))),
                                 dict(frames=8, depth=np.ones(5), samples=1)])
def test_search_samples_args_range_and_shape_errors(bad):
    with pytest.raises(ValueError):
        search_samples_args("breakout", 6, **bad)
    assert search_samples_args("breakout", 6, 8, 3, 1024)[0][9] == 1024.0, "64 plans x 1 024 samples: exactly at the cap; 1 025 is one above"
    assert search_samples_args("breakout", 6, 8, 6, 16)[0][2] == 6.0, "4 096 plans x 16 samples: exactly at the cap; 17 is above"


def test_the_adapters_map_action_indices_and_steps(monkeypatch):
    """search_samples: ToyboxVecEnv frames = steps, hold = 1; ToyboxPreprocVecEnv frames = steps x skip, hold = skip; `rest` an action
    index going in, `plan` action indices coming out; the means are added, best_action is sample_best_action over the rows and
    best_plan that row's plan; a pending step ends first"""
    from toybox_amd.envs import vec_env
    lut = np.asarray(LEGAL["space_invaders"], np.int32)
    L = len(lut)

    class FakeEngine:
        legal_actions = list(lut)

        def lookahead_search_samples(self, frames, depth, samples, **kw):
            self.call = (frames, depth, samples, kw)
            out = {k: np.zeros((3, L), np.int64) for k in SAMPLE_FIELDS}
            out["samples"][:] = 4
            out["ret_sum"][0, 4], out["ret_sum"][0, 2] = 120, 40
            out["lost"][0] = [1, 1, 0, 1, 4, 1]
            out["ended"][0, 4] = 2
            out["samples"][2] = 0                                 # a refused env: its means are 0, not a division by 0
            out["code"] = (np.arange(L)[None, :] + L * np.array([[1], [3], [0]])).astype(np.uint64)
            out["plan"] = np.full((3, L, depth), -7)              # (ALE ids: the adapter puts action indices in their place)
            return out

    for cls, skip in ((vec_env.ToyboxVecEnv, 1), (vec_env.ToyboxPreprocVecEnv, 4)):
        v = object.__new__(cls)
        v.num_envs, v._in_flight, v._pending, v.engine, v._lut, v._action_set, v._skip = 3, None, None, FakeEngine(), lut, list(lut), 4
        waited = []
        monkeypatch.setattr(cls, "step_wait", lambda self: waited.append(1) or setattr(self, "_in_flight", None))
        out = v.search_samples(5, 2, 4, rest=4, seed=9, t=3, salt=1000)
        frames, depth, samples, kw = v.engine.call
        assert (frames, depth, samples, kw["hold"], kw["objective"], kw["rest"], kw["seed"], kw["t"], kw["salt"]) == (5 * skip, 2, 4, skip, "return", 11, 9, 3, 1000)
        assert out["ret_mean"][0].tolist() == [0, 0, 10.0, 0, 30.0, 0] and out["lost_frac"][0, 4] == 1.0 and out["ended_frac"][0, 4] == 0.5
        assert (out["ret_mean"][2] == 0).all() and np.isfinite(out["lost_frac"]).all()
        assert out["plan"].shape == (3, L, 2) and out["plan"][0].tolist() == [[a, 1] for a in range(L)] and out["plan"][1].tolist() == [[a, 3] for a in range(L)]
        assert out["best_action"].tolist() == [4, 0, 0] and out["best_plan"].tolist() == [[4, 1], [0, 3], [0, 0]]
        out = v.search_samples(5, 2, 4, objective="survival")
        assert out["best_action"].tolist() == [2, 0, 0] and out["best_plan"][0].tolist() == [2, 1]
        assert v.engine.call[3]["rest"] is None and v.engine.call[3]["salt"] == 0 and v.engine.call[3]["objective"] == "survival"
        assert not waited
        v._in_flight = object()
        v.search_samples(1, 1, 1)
        assert waited == [1]
        with pytest.raises(AssertionError):
            v.search_samples(1, 1, 1, rest=6)
        with pytest.raises(ValueError):
            v.search_samples(1, 1, 1, objective="score")


def test_the_order_on_hand_made_sums():
    """pick on plans whose sums are written by hand: each key of each objective decides once, and the code breaks the last tie"""
    game, L = "breakout", 4
    sums = {k: np.zeros((1, 16), np.int64) for k in SAMPLE_FIELDS}
    # group 0 (codes 0, 4, 8, 12): 8 has the largest ret_sum but loses more often; 4 and 12 tie in everything
    sums["ret_sum"][0, [0, 4, 8, 12]] = [5, 7, 9, 7]
    sums["lost"][0, [0, 4, 8, 12]] = [0, 1, 2, 1]
    sums["safe_frames_sum"][0, [0, 4, 8, 12]] = [10, 30, 30, 30]
    # group 1 (codes 1, 5, 9, 13): equal ret_sum and lost, 9 keeps the most safe frames
    sums["safe_frames_sum"][0, [1, 5, 9, 13]] = [3, 4, 6, 5]
    # group 2: all equal -> the smallest code; group 3: equal lost and safe frames, 15 has the larger ret_sum
    sums["ret_sum"][0, 15] = 1
    ok, depth = np.ones(1, bool), np.array([2])
    assert pick(game, sums, ok, depth, 0)["code"].tolist() == [[8, 9, 2, 15]]
    assert pick(game, sums, ok, depth, 1)["code"].tolist() == [[0, 9, 2, 15]]
    sums["lost"][0, 0] = 1                                       # now 0, 4, 12 lose once: 4 and 12 keep more safe frames, 4 is the smaller code
    assert pick(game, sums, ok, depth, 1)["code"].tolist() == [[4, 9, 2, 15]]
    assert (pick(game, sums, np.zeros(1, bool), depth, 0)["code"] == 0).all()


# ---------------------------------------------------------------- the yardstick, held to the older yardsticks on the checker alone

SMALL = {"breakout": (8, 48, 4, 400), "space_invaders": (6, 48, 4, 400), "amidar": (6, 32, 4, 400), "gridworld": (8, 16, 2, 40)}


@pytest.fixture(scope="module")
def batches(oracle_lib):
    out = {}
    for game in GAMES:
        n, _, _, batch_frames = SMALL[game]
        e = batch(oracle_lib, game, n, frames=batch_frames)
        out[game] = (e.get_states(), sim_rngs(e))
        e.close()
    return out


@pytest.mark.parametrize("game", GAMES)
def test_depth_1_is_the_sampled_lookahead_replay(game, batches, oracle_lib):
    states, rngs = batches[game]
    _, frames, hold, _ = SMALL[game]
    sched = dict(frames=frames, hold=hold, samples=3, salt=1000, rest=-1, seed=(3 << 40) | 9, t=2 ** 32 - 2, env_offset=11)
    want = expected_samples(oracle_lib, game, states, rngs, sched)
    for objective in (0, 1):
        got = expected_search_samples(oracle_lib, game, states, rngs, dict(sched, depth=1, objective=objective))
        for k in SAMPLE_FIELDS:
            assert np.array_equal(got[k], want[k]), (k, objective)
        assert np.array_equal(got["code"], np.tile(np.arange(len(LEGAL[game])), (len(states), 1))), "one plan per group: its first action"
    assert (want["samples"] == 3).all()


@pytest.mark.parametrize("game", GAMES)
def test_one_sample_is_the_search_replay_folded_into_sums(game, batches, oracle_lib):
    states, rngs = batches[game]
    _, frames, hold, _ = SMALL[game]
    case = dict(frames=frames, hold=hold, depth=2, rest=LEGAL[game][1], seed=5)
    leaves, active, ok, depth = play_all(oracle_lib, game, states, rngs, dict(case, samples=1))
    one, ok_search, _ = play_all_codes(oracle_lib, game, states, rngs, dict(case, seed=sample_seed(5, 0)))
    assert ok.all() and ok_search.all() and active.shape == (1, len(states)) and active.all()
    sums = aggregate(leaves, active)
    ret, lost_at = one["ret"].astype(np.int64), one["life_lost_at"]
    assert (sums["samples"] == 1).all()
    for k in ("ret_sum", "ret_min", "ret_max"):
        assert np.array_equal(sums[k], ret), k
    assert np.array_equal(sums["lives_sum"], one["lives"]) and np.array_equal(sums["lost"], lost_at >= 0) and np.array_equal(sums["ended"], one["lives"] <= 0)
    assert np.array_equal(sums["safe_frames_sum"], np.where(lost_at < 0, one["frames_run"], lost_at))
    for k in FIELDS:
        assert np.array_equal(leaves[k][0], one[k].astype(np.int64)), k


@pytest.mark.parametrize("game", ["breakout", "space_invaders"])
def test_the_rows_do_not_depend_on_the_order_of_the_futures(game, batches, oracle_lib):
    states, rngs = batches[game]
    n = len(states)
    _, frames, hold, _ = SMALL[game]
    case = dict(frames=frames, hold=hold, depth=np.resize([2, 1], n), samples=np.resize([4, 3, 1], n), salt=1000, rest=-1, seed=21)
    leaves, active, ok, depth = play_all(oracle_lib, game, states, rngs, case)
    assert ok.all() and active.sum(axis=0).tolist() == np.resize([4, 3, 1], n).tolist()
    for objective in (0, 1):
        want = pick(game, aggregate(leaves, active), ok, depth, objective)
        assert game == "breakout" or (want["ret_min"] < want["ret_max"]).any(), "SpaceInvaders fires by its salted RNG: the futures of a winner differ"
        for order in ([3, 2, 1, 0], [2, 0, 3, 1]):
            got = pick(game, aggregate(leaves, active, order), ok, depth, objective)
            for k in ROW_FIELDS:
                assert np.array_equal(got[k], want[k]), (k, order, objective)


def test_refused_rows_are_zero_and_leave_the_others(batches, oracle_lib):
    game = "breakout"
    states, rngs = batches[game]
    n = len(states)
    depth, samples, salt, objective = np.full(n, 2), np.full(n, 2), np.full(n, 9), np.zeros(n, np.int64)
    depth[[0, 1]] = [0, 7]
    samples[[2, 3]] = [0, 4097]
    salt[4] = -1
    objective[5] = 2
    base = dict(frames=24, hold=4, rest=0, seed=4)
    assert valid_rows(game, columns(n, depth=depth, samples=samples, salt=salt, objective=objective, **base)).tolist() == [False] * 6 + [True] * (n - 6)
    assert not valid_rows(game, columns(1, 8, depth=3, samples=1025))[0] and valid_rows(game, columns(1, 8, depth=3, samples=1024))[0], "the cap on the leaves"
    got = expected_search_samples(oracle_lib, game, states, rngs, dict(base, depth=depth, samples=samples, salt=salt, objective=objective))
    plain = expected_search_samples(oracle_lib, game, states, rngs, dict(base, depth=2, samples=2, salt=9))
    for k in ROW_FIELDS:
        assert (got[k][:6] == 0).all() and np.array_equal(got[k][6:], plain[k][6:]), k
    assert (plain["samples"] == 2).all()
