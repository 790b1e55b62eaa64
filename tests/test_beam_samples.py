"""Beam search over sampled futures (TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES), the part that needs no GPU: the constants, the argument
shaping with every range error and the leaf cap, and the yardstick of tests/test_gpu_beam_samples.py under test itself over the CPU
checker alone (tests/beam_samples_replay.py): with a beam wide enough its rows are the rows of the search-over-samples replay, at
depth 1 those of the sampled lookahead's replay, and the GPU module's cases cover what they must."""
import functools
import os
import re
import time

import numpy as np
import pytest

from beam_samples_replay import CASES, MAX_WIDTH, case_args, case_coverage, expected_beam_samples, kept_count, leaves_of, missing_coverage
from conftest import ROOT
from fork_replay import sim_rngs
from lookahead_replay import batch
from sample_replay import expected_samples
from search_samples_replay import ROW_FIELDS, assert_rows_equal, expected_search_samples
from support import LEGAL
from toybox_amd import Engine, ToyboxAmdError, _abi
from toybox_amd.engine import SAMPLE_FIELDS, beam_args, beam_kept, beam_samples_args

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
HEADER = open(os.path.join(ROOT, "include", "toybox_amd.h")).read()


def test_header_and_python_agree_on_the_constants():
    want = {"TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES": (_abi.QUERY_LOOKAHEAD_BEAM_SAMPLES, 157), "TBX_OPT_BEAM_SAMPLES_RANGES": (_abi.OPT_BEAM_SAMPLES_RANGES, 111),
            "TBX_OPT_BEAM_SAMPLES_CHUNKS": (_abi.OPT_BEAM_SAMPLES_CHUNKS, 112), "TBX_OPT_BEAM_SAMPLES_MAX_CHUNKS": (_abi.OPT_BEAM_SAMPLES_MAX_CHUNKS, 113)}
    for name, (py, value) in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, HEADER)
        assert m and int(m.group(1)) == py == value, name
    assert re.search(r"#define\s+TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES\s+157\s*/\*.*env_offset, width, samples, salt\}\s*->\s*9\s*\*\s*n_legal", HEADER), \
        "the columns and the width stand on the #define line"
    assert len(re.findall(r"\btbx_\w*(lookahead|sample|search|beam)\w*\s*\(", HEADER)) == 0, "the query goes through tbx_reduce: no new symbol"
    assert re.search(r"#define\s+TBX_ABI_VERSION\s+1\b", HEADER)
    assert MAX_WIDTH == _abi.BEAM_MAX_WIDTH
    assert "caps the ranges of a TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES too" in HEADER, "TBX_OPT_BEAM_RANGE_ENVS says that it covers this query"


def test_the_checker_does_not_have_the_query(oracle_lib):
    """the expected values cannot come from the checker's own: it answers "unknown query\""""
    with Engine("breakout", 4, lib=oracle_lib) as e:
        for call in (lambda: e.lookahead_beam_samples(8, 2, 2, 2), lambda: e.reduce(157, [8])):
            with pytest.raises(ToyboxAmdError) as ei:
                call()
            assert ei.value.code == _abi.E_INVALID


# ---------------------------------------------------------------- the argument shaping

def test_args_defaults_and_scalars():
    assert beam_samples_args("breakout", 8, 16, 1, 1, 1) == ([16.0, 1.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0], False)
    seed = (0xDEADBEEF << 32) | 0x12345678
    args, per_env = beam_samples_args("space_invaders", 8, 300, 12, 4, 16, hold=4, objective="survival", salt=1000, rest=11, seed=seed, t=77, env_offset=4096)
    assert per_env is False and args == [300.0, 4.0, 12.0, 1.0, 11.0, float(0x12345678), float(0xDEADBEEF), 77.0, 4096.0, 4.0, 16.0, 1000.0]
    assert args[:10] == beam_args("space_invaders", 8, 300, 12, 4, 4, "survival", 11, seed, 77, 4096)[0], "columns 0 .. 9 stand where the beam's stand"
    for game in GAMES:                                         # every depth a plan can have
        assert beam_samples_args(game, 2, 8, _abi.PLAN_MAX_DEPTH[game], 2, 3)[0][2] == float(_abi.PLAN_MAX_DEPTH[game])
    assert beam_samples_args("amidar", 8, 8, 1, 1, 4096, salt=2 ** 32 - 4096)[0][10:] == [4096.0, float(2 ** 32 - 4096)], "the largest salt that fits"


def test_args_per_env_rows():
    n = 6
    depth, width, samples, salt = np.array([1, 2, 0, 17, 3, 2]), np.array([1, 64, 0, 65, 2, 3]), np.array([1, 5, 0, 4097, 8, 8]), np.array([0, 7, 0, 0, -1, 2 ** 32 - 3])
    args, per_env = beam_samples_args("breakout", n, np.array([1, 2, 4, 299, 0, 1024]), depth, width, samples, hold=7, objective=np.array([0, 1, 2, 0, 1, 0]), salt=salt,
                                      seed=np.arange(n, dtype=np.uint64) << np.uint64(33), t=5)
    assert per_env is True and args.shape == (n, 12) and args.dtype == np.float64
    # per-env rows are checked on the device (a bad row answers zeros), not here
    assert args[:, 0].tolist() == [1, 2, 4, 299, 0, 1024] and args[:, 1].tolist() == [7] * n and args[:, 2].tolist() == depth.tolist()
    assert args[:, 3].tolist() == [0, 1, 2, 0, 1, 0] and args[:, 4].tolist() == [-1] * n and args[:, 5].tolist() == [0] * n
    assert args[:, 6].tolist() == [2.0 * i for i in range(n)] and args[:, 7].tolist() == [5] * n and args[:, 8].tolist() == [0] * n
    assert args[:, 9].tolist() == width.tolist() and args[:, 10].tolist() == samples.tolist() and args[:, 11].tolist() == salt.tolist()
    for kw, col in ((dict(salt=np.arange(n)), 11), (dict(samples=np.arange(n)), 10), (dict(width=np.arange(n)), 9)):
        call = dict(dict(frames=8, depth=2, width=3, samples=4), **kw)
        args, per_env = beam_samples_args("breakout", n, **call)
        assert per_env is True and args[:, col].tolist() == list(range(n)) and args[:, 2].tolist() == [2] * n
        assert all(args[:, k].tolist() == [v] * n for k, v in ((9, 3), (10, 4), (11, 0)) if k != col)


@pytest.mark.parametrize("bad", [dict(frames=0), dict(frames=1025), dict(hold=0), dict(depth=0), dict(depth=17), dict(width=0), dict(width=65), dict(samples=0),
                                 dict(samples=4097), dict(objective=2), dict(objective="score"), dict(rest=2), dict(salt=-1), dict(salt=2 ** 32),
                                 dict(salt=2 ** 32 - 1), dict(samples=4096, width=1, salt=2 ** 32 - 4095), dict(seed=2 ** 64), dict(t=2 ** 32), dict(env_offset=-3),
                                 dict(depth=np.ones(5)), dict(width=np.ones(5)), dict(width=np.ones((6, 1))), dict(samples=np.ones(5)), dict(salt=np.zeros((6, 1))),
                                 dict(objective=np.zeros(7)),
                                 # the leaf cap: n_legal * kept(depth - 1) * n_legal * samples above 65 536
                                 dict(depth=2, width=1, samples=4097), dict(depth=3, width=4, samples=1025), dict(depth=5, width=64, samples=65),
                                 dict(depth=4, width=64, samples=257), dict(depth=16, width=64, samples=65), dict(depth=3, width=2, samples=2049)])
def test_beam_samples_args_range_and_shape_errors(bad):
    kw = dict(frames=8, depth=2, width=2, samples=2)
    kw.update(bad)
    with pytest.raises(ValueError):
        beam_samples_args("breakout", 6, **kw)


def test_the_leaf_cap():
    """candidates of the widest level x samples <= 65 536, exactly at the cap and one above.  Breakout (L = 4) at width 64: level 5
    is the first whose parents fill the beam (|B_4| = 64), 4 x 64 x 4 = 1 024 candidates and 64 samples; at depth 4 the beam is the
    whole tree (|B_3| = 16, 256 candidates = 4^4) and the cap is that of the search over samples, 256 samples"""
    assert [beam_kept(4, 64, d) for d in range(0, 7)] == [1, 1, 4, 16, 64, 64, 64] and [kept_count(4, 64, d) for d in range(0, 7)] == [1, 1, 4, 16, 64, 64, 64]
    assert [beam_kept(6, 5, d) for d in range(1, 5)] == [1, 5, 5, 5] and beam_kept(5, 1, 9) == 1
    at_cap = {"breakout": [(1, 1, 4096), (1, 7, 4096), (2, 1, 4096), (2, 64, 4096), (3, 1, 4096), (3, 64, 1024), (4, 64, 256), (5, 64, 64), (16, 64, 64), (16, 1, 4096),
                           (7, 2, 2048)],
              "space_invaders": [(1, 64, 4096), (2, 1, 1820), (3, 64, 303), (12, 64, 28), (12, 2, 910)], "gridworld": [(13, 64, 40), (4, 64, 104)]}
    for game, rows in at_cap.items():
        L = len(LEGAL[game])
        for depth, width, samples in rows:
            assert beam_samples_args(game, 4, 8, depth, width, samples)[0][10] == float(samples), (game, depth, width, samples)
            assert leaves_of(L, width, depth, samples) <= _abi.LOOKAHEAD_MAX_LEAVES < leaves_of(L, width, depth, samples + 1) or samples == 4096
            if samples < 4096:
                with pytest.raises(ValueError):
                    beam_samples_args(game, 4, 8, depth, width, samples + 1)
    # where the search over samples accepts a depth, a beam that is the whole tree has the search's cap
    for game in GAMES:
        L = len(LEGAL[game])
        for depth in range(1, 7):
            if L ** depth <= _abi.LOOKAHEAD_MAX_PLANS and L ** max(depth - 2, 0) <= 64:
                assert leaves_of(L, 64, depth, 1) == L ** depth


# ---------------------------------------------------------------- the yardstick, held to the older yardsticks on the checker alone

N = 8
SMALL = {"breakout": (48, 4, 400), "space_invaders": (48, 4, 400), "amidar": (32, 4, 400), "gridworld": (16, 2, 40)}


@pytest.fixture(scope="module")
def batches(oracle_lib):
    out = {}
    for game in GAMES:
        e = batch(oracle_lib, game, N, frames=SMALL[game][2])
        out[game] = (e.get_states(), sim_rngs(e))
        e.close()
    return out


@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("game", GAMES)
def test_a_beam_wide_enough_is_the_search_over_samples(game, objective, batches, oracle_lib):
    """width >= n_legal ** (depth - 2): no level drops a candidate, so the rows are those of all codes played, summed and picked"""
    states, rngs = batches[game]
    frames, hold, _ = SMALL[game]
    L = len(LEGAL[game])
    for depth, width in ((2, 1), (3, L), (3, L + 3)):
        case = dict(frames=frames, hold=hold, depth=depth, samples=2, objective=objective, salt=0 if game == "gridworld" else 1000, rest=-1, seed=(3 << 40) | 9,
                    t=2 ** 32 - 2, env_offset=11)
        got, levels = expected_beam_samples(oracle_lib, game, states, rngs, dict(case, width=width))
        assert len(levels) == depth and levels[-1]["valid"].sum() == N * L * (L ** (depth - 1))
        assert_rows_equal(got, expected_search_samples(oracle_lib, game, states, rngs, case), "%s depth %d width %d objective %d" % (game, depth, width, objective))
        assert (got["samples"] == 2).all()


@pytest.mark.parametrize("game", GAMES)
def test_depth_1_is_the_sampled_lookahead_replay(game, batches, oracle_lib):
    states, rngs = batches[game]
    frames, hold, _ = SMALL[game]
    sched = dict(frames=frames, hold=hold, samples=3, salt=1000, rest=-1, seed=(3 << 40) | 9, t=2 ** 32 - 2, env_offset=11)
    want = expected_samples(oracle_lib, game, states, rngs, sched)
    for objective in (0, 1):
        for width in (1, 5):
            got, _ = expected_beam_samples(oracle_lib, game, states, rngs, dict(sched, depth=1, width=width, objective=objective))
            for k in SAMPLE_FIELDS:
                assert np.array_equal(got[k], want[k]), (k, objective)
            assert np.array_equal(got["code"], np.tile(np.arange(len(LEGAL[game])), (N, 1))), "one candidate per group: its first action"
    assert (want["samples"] == 3).all()


def test_refused_rows_are_zero_and_leave_the_others(batches, oracle_lib):
    game = "breakout"
    states, rngs = batches[game]
    depth, width, samples, salt, objective = np.full(N, 3), np.full(N, 2), np.full(N, 2), np.full(N, 9), np.zeros(N, np.int64)
    depth[0], width[1], samples[2], salt[3], objective[4] = 17, 65, 4097, -1, 2
    depth[5], width[5], samples[5] = 5, 64, 65                  # the leaf cap
    base = dict(frames=24, hold=4, rest=0, seed=4)
    got, _ = expected_beam_samples(oracle_lib, game, states, rngs, dict(base, depth=depth, width=width, samples=samples, salt=salt, objective=objective))
    plain, _ = expected_beam_samples(oracle_lib, game, states, rngs, dict(base, depth=3, width=2, samples=2, salt=9))
    for k in ROW_FIELDS:
        assert (got[k][:6] == 0).all() and np.array_equal(got[k][6:], plain[k][6:]), k
    assert (plain["samples"] == 2).all()


# ---------------------------------------------------------------- the GPU module's cases cover what they must

@functools.lru_cache(maxsize=None)
def case_counts(oracle_lib, game, case):
    e = batch(oracle_lib, game, case[0], frames=case[7])
    states, rngs = e.get_states(), sim_rngs(e)
    e.close()
    t0 = time.perf_counter()
    replays = {o: expected_beam_samples(oracle_lib, game, states, rngs, dict(case_args(case), objective=o)) for o in (0, 1)}
    seconds = time.perf_counter() - t0
    counts = case_coverage(case, replays)
    print(game, case, "replay of both objectives %.1f s" % seconds, counts)
    return counts


@pytest.mark.parametrize("game", GAMES)
def test_the_cases_cover_what_they_must(game, oracle_lib):
    """over a game's two cases (tests/beam_samples_replay.py, CASES), on the replay alone, each above 0: (group, level) cuts decided
    by the code alone, kept sets that are not the first `width` codes, final winners that are not the smallest code, candidates
    whose futures differ in their return, groups whose kept set or final winner under all futures is not the one under future 0
    alone, groups where the two objectives return different codes"""
    deep = CASES[game][0]
    assert game != "breakout" or len(LEGAL[game]) ** deep[3] > _abi.LOOKAHEAD_MAX_PLANS, "Breakout's deep case is beyond the search over samples"
    totals = {}
    for case in CASES[game]:
        for k, v in case_counts(oracle_lib, game, case).items():
            totals[k] = totals.get(k, 0) + int(v)
    missing = missing_coverage(totals)
    assert not missing, "%s: the cases together never show: %s (%r)" % (game, ", ".join(missing), totals)


# ---------------------------------------------------------------- the adapters

def test_the_adapters_map_action_indices_and_steps(monkeypatch):
    """beam_search_samples: ToyboxVecEnv frames = steps, hold = 1; ToyboxPreprocVecEnv frames = steps x skip, hold = skip; `rest` an
    action index going in, `plan` action indices coming out; the means, best_action (sample_best_action) and best_plan are added as
    search_samples adds them; a pending step ends first"""
    from toybox_amd.envs import vec_env
    lut = np.asarray(LEGAL["space_invaders"], np.int32)
    L = len(lut)

    class FakeEngine:
        legal_actions = list(lut)

        def lookahead_beam_samples(self, frames, depth, width, samples, **kw):
            self.call = (frames, depth, width, samples, kw)
            out = {k: np.zeros((3, L), np.int64) for k in SAMPLE_FIELDS}
            out["samples"][:] = 4
            out["ret_sum"][0, 4], out["ret_sum"][0, 2] = 120, 40
            out["lost"][0] = [1, 1, 0, 1, 4, 1]
            out["ended"][0, 4] = 2
            out["samples"][2] = 0                                 # a refused env: its means are 0, not a division by 0
            out["code"] = (np.arange(L)[None, :] + L * np.array([[1], [3], [0]])).astype(np.uint64)
            out["plan"] = np.full((3, L, depth), -7)
            return out

    for cls, skip in ((vec_env.ToyboxVecEnv, 1), (vec_env.ToyboxPreprocVecEnv, 4)):
        v = object.__new__(cls)
        v.num_envs, v._in_flight, v._pending, v.engine, v._lut, v._action_set, v._skip = 3, None, None, FakeEngine(), lut, list(lut), 4
        waited = []
        monkeypatch.setattr(cls, "step_wait", lambda self: waited.append(1) or setattr(self, "_in_flight", None))
        out = v.beam_search_samples(5, 2, 3, 4, rest=4, seed=9, t=3, salt=1000)
        frames, depth, width, samples, kw = v.engine.call
        assert (frames, depth, width, samples, kw["hold"], kw["objective"], kw["rest"], kw["seed"], kw["t"], kw["salt"]) == (5 * skip, 2, 3, 4, skip, "return", 11, 9, 3, 1000)
        assert out["ret_mean"][0].tolist() == [0, 0, 10.0, 0, 30.0, 0] and out["lost_frac"][0, 4] == 1.0 and out["ended_frac"][0, 4] == 0.5
        assert (out["ret_mean"][2] == 0).all() and np.isfinite(out["lost_frac"]).all()
        assert out["plan"].shape == (3, L, 2) and out["plan"][0].tolist() == [[a, 1] for a in range(L)] and out["plan"][1].tolist() == [[a, 3] for a in range(L)]
        assert out["best_action"].tolist() == [4, 0, 0] and out["best_plan"].tolist() == [[4, 1], [0, 3], [0, 0]]
        out = v.beam_search_samples(5, 2, 3, 4, objective="survival")
        assert out["best_action"].tolist() == [2, 0, 0] and out["best_plan"][0].tolist() == [2, 1]
        assert v.engine.call[4]["rest"] is None and v.engine.call[4]["salt"] == 0 and v.engine.call[4]["objective"] == "survival"
        assert not waited
        v._in_flight = object()
        v.beam_search_samples(1, 1, 1, 1)
        assert waited == [1]
        with pytest.raises(AssertionError):
            v.beam_search_samples(1, 1, 1, 1, rest=6)
        with pytest.raises(ValueError):
            v.beam_search_samples(1, 1, 1, 1, objective="score")
