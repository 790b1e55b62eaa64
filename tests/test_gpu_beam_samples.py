"""Beam search over sampled futures on the device (TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES, include/toybox_amd.h) against SALT, PLAY
LEVEL BY LEVEL, SUM AND SORT on the CPU checker (tests/beam_samples_replay.py; its own checks are in tests/test_beam_samples.py).
Every comparison is exact, on all nine fields of every (env, first action) row.

The worlds are those of tests/test_gpu_search.py (_world): made by the input recipe of tests/lookahead_replay.py and held to their
checker twins byte for byte before any query; the expected rows are played on clones of the records the DEVICE engine reports, once
per (case, objective), shared and left unchanged.  Every case has rest = -1 and seed 77: (envs, frames, hold, depth, width, samples,
salt, batch frames).  Measured on the checker alone (tests/test_beam_samples.py prints them; an 8-core host), replay of both
objectives together and, summed over the objectives, (group, level) cuts decided by the code alone / kept sets that are not the
first `width` codes / final winners that are not the smallest code / candidates whose futures differ in their return / groups whose
kept set or final winner under all futures is not the one under future 0 alone / groups where the objectives return different codes:
  Breakout       (24, 96, 8, 7, 2, 3, 1000, 400) 8.1 s 1102 / 98 / 6 / 8 / 46 / 0;      (96, 200, 8, 3, 1, 3, 1000, 400) 10.5 s 1176 / 376 / 189 / 1428 / 272 / 10
  SpaceInvaders  (12, 96, 8, 5, 2, 2, 1000, 400) 9.0 s 341 / 345 / 79 / 3087 / 199 / 15;  (24, 96, 8, 3, 1, 3, 1000, 400) 4.0 s 370 / 321 / 182 / 2273 / 144 / 25
  Amidar         (24, 96, 4, 5, 2, 2, 1000, 400) 8.2 s 1016 / 296 / 50 / 2746 / 142 / 0;  (96, 128, 8, 3, 1, 3, 1000, 900) 6.8 s 1622 / 700 / 346 / 3493 / 467 / 5
  GridWorld      (24, 40, 2, 6, 2, 3, 0, 40) 4.5 s 1007 / 561 / 130 / 5301 / 365 / 12;    (96, 40, 2, 3, 1, 3, 0, 80) 1.4 s 1415 / 505 / 238 / 4792 / 326 / 31
Every condition holds per game with the two cases together; Breakout and Amidar need their shallow case for the objectives to
disagree."""
import functools

import numpy as np
import pytest

from beam_samples_replay import CASES, DRAWN, case_args, case_coverage, expected_beam_samples, missing_coverage
from sample_replay import LEAF_FIELDS
from sample_replay import aggregate as aggregate_samples
from search_samples_replay import ROW_FIELDS, assert_rows_equal
from support import LEGAL
from test_gpu_search import _assert_same_snapshot, _device_reduce, _snapshot, _world
from toybox_amd import ToyboxAmdError, _abi
from toybox_amd.engine import SAMPLE_FIELDS, Engine, beam_samples_args, plan_actions, plan_args, sample_seed

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
OBJECTIVES = ["return", "survival"]
QUERY = _abi.QUERY_LOOKAHEAD_BEAM_SAMPLES
ALL_CASES = [(game, case) for game in GAMES for case in CASES[game]]
SEARCH_DEPTH = {"breakout": 6, "space_invaders": 4, "amidar": 4, "gridworld": 5}      # the deepest the exhaustive searches accept
# rows the host has not seen are budgeted as the largest valid row, 2^26 leaf-frames per env and level: the ranges of 24 envs under
# tbx_search_samples_budget (Breakout, a thread per unit, 2^32: 64 envs; SpaceInvaders 2^29: 8; Amidar 2^27: 2; GridWorld 2^30: 16)
UNSEEN_ROW_RANGES = {"breakout": 1, "space_invaders": 3, "amidar": 12, "gridworld": 2}


@functools.lru_cache(maxsize=None)
def _replay(game, case, objective, drawn, hip_lib, oracle_lib):
    """(rows, levels) of the case replayed on the checker, made once, shared and left unchanged"""
    _, states, rngs = _world(game, case[0], case[7], hip_lib, oracle_lib)
    rows, levels = expected_beam_samples(oracle_lib, game, states, rngs, dict(case_args(case), objective=objective, **(DRAWN if drawn else {})))
    for v in rows.values():
        v.flags.writeable = False
    return rows, levels


def _ask(g, case, objective, **more):
    c = dict(case_args(case), **more)
    assert c.pop("rest") == -1
    return g.lookahead_beam_samples(c.pop("frames"), c.pop("depth"), c.pop("width"), c.pop("samples"), objective=objective, rest=None, **c)


def _assert_same_rows(a, b, what):
    for k in ROW_FIELDS + ("plan",):
        assert np.array_equal(a[k], b[k]), (what, k)


# ---------------------------------------------------------------- 1. rows equal the replay

@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("game,case", ALL_CASES, ids=["%s-%d-%d-%d-%d-%d-%d" % ((g,) + c[:6]) for g, c in ALL_CASES])
def test_rows_equal_replay(game, case, objective, hip_lib, oracle_lib):
    n, frames, hold, depth, width, samples, salt, batch_frames = case
    L = len(LEGAL[game])
    g, _, _ = _world(game, n, batch_frames, hip_lib, oracle_lib)
    want, _ = _replay(game, case, OBJECTIVES.index(objective), False, hip_lib, oracle_lib)
    got = _ask(g, case, objective)
    assert all(got[k].shape == (n, L) and got[k].dtype == np.int64 for k in SAMPLE_FIELDS) and (got["samples"] == samples).all()
    assert got["code"].dtype == np.uint64 and got["plan"].shape == (n, L, depth)
    assert_rows_equal(got, want, "%s %r %s" % (game, case, objective))
    assert np.array_equal(got["plan"], plan_actions(game, want["code"], depth)) and np.array_equal(got["plan"][:, :, 0], np.tile(LEGAL[game], (n, 1)))
    assert g.beam_samples_ranges == 1
    if game == "breakout" and case is CASES[game][0]:
        assert L ** depth > _abi.LOOKAHEAD_MAX_PLANS, "the deep case is one no search over samples reaches"


@pytest.mark.parametrize("game", GAMES)
def test_the_cases_cover_what_they_must(game, hip_lib, oracle_lib):
    """asserted on the expected arrays, so no test passes by avoiding the hard rows"""
    totals = {}
    for case in CASES[game]:
        for k, v in case_coverage(case, {o: _replay(game, case, o, False, hip_lib, oracle_lib) for o in (0, 1)}).items():
            totals[k] = totals.get(k, 0) + int(v)
    missing = missing_coverage(totals)
    assert not missing, "%s: the cases together never show: %s (%r)" % (game, ", ".join(missing), totals)


# ---------------------------------------------------------------- 2. one drawn case per game

@pytest.mark.parametrize("game", GAMES)
def test_a_seed_above_32_bits_a_counter_that_leaves_32_bits_and_an_env_offset(game, hip_lib, oracle_lib):
    """the deep case under seed 0xABCDE01234567, t = 2^32 - 3 and env_offset = 70 000 (the objectives take turns over the games)"""
    case = CASES[game][0]
    o = GAMES.index(game) % 2
    g, _, _ = _world(game, case[0], case[7], hip_lib, oracle_lib)
    assert DRAWN["seed"] >> 32 and DRAWN["t"] + (case[1] - 1) // case[2] >= 2 ** 32
    want, _ = _replay(game, case, o, True, hip_lib, oracle_lib)
    got = _ask(g, case, OBJECTIVES[o], **DRAWN)
    assert_rows_equal(got, want, "%s drawn, %s" % (game, OBJECTIVES[o]))
    other = _ask(g, case, OBJECTIVES[o], **dict(DRAWN, seed=DRAWN["seed"] ^ (1 << 40)))
    assert any(not np.array_equal(other[k], got[k]) for k in ROW_FIELDS), "the upper half of the seed is not read"


# ---------------------------------------------------------------- 3. the device equals itself

@pytest.mark.parametrize("game", GAMES)
def test_depth_1_is_the_sampled_lookahead(game, hip_lib, oracle_lib):
    n = 24
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    kw = dict(hold=4, salt=1000, seed=(7 << 33) | 5, t=2 ** 32 - 2, env_offset=99)
    want = g.lookahead_samples(40, 6, **kw)
    for objective in OBJECTIVES:
        for width in (1, 7):
            got = g.lookahead_beam_samples(40, 1, width, 6, objective=objective, **kw)
            for k in SAMPLE_FIELDS:
                assert np.array_equal(got[k], want[k]), (game, objective, width, k)
            assert np.array_equal(got["code"], np.tile(np.arange(len(LEGAL[game]), dtype=np.uint64), (n, 1)))
    assert (want["samples"] == 6).all()


@pytest.mark.parametrize("game", GAMES)
def test_a_beam_wide_enough_is_the_search_over_samples(game, hip_lib, oracle_lib):
    """width = n_legal ** (depth - 2), and width 64 at the deepest depth the search over samples accepts for 3 samples at which 64
    is still wide enough (Breakout 5, where 4 ** 3 is 64 itself; GridWorld 4; SpaceInvaders and Amidar 4, their deepest): its rows
    and plans, bit for bit"""
    n, L, samples = 24, len(LEGAL[game]), 3
    depth = max(d for d in range(2, SEARCH_DEPTH[game] + 1) if L ** (d - 2) <= _abi.BEAM_MAX_WIDTH and L ** d * samples <= _abi.LOOKAHEAD_MAX_LEAVES)
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    kw = dict(hold=4, salt=0 if game == "gridworld" else 1000, seed=(5 << 36) | 77, t=9, env_offset=3)
    for objective in OBJECTIVES:
        for d, width in ((2, 1), (3, L), (depth, L ** (depth - 2)), (depth, 64)):
            a = g.lookahead_beam_samples(40, d, width, samples, objective=objective, **kw)
            b = g.lookahead_search_samples(40, d, samples, objective=objective, **kw)
            _assert_same_rows(a, b, (game, objective, d, width))
            assert (a["samples"] == samples).all()


@pytest.mark.parametrize("game", GAMES)
def test_every_returned_code_reproduces_its_row_from_plan_calls(game, hip_lib, oracle_lib):
    """salt 0: future s of a candidate is TBX_QUERY_LOOKAHEAD_PLAN under sample_seed(seed, s), so `samples` plan calls per first
    action at the returned code, summed on the host, are the row.  The deep case's shape, at TBX_PLAN_MAX_DEPTH"""
    n, frames, hold, _, width, samples, _, batch_frames = CASES[game][0]
    depth = _abi.PLAN_MAX_DEPTH[game]
    g, _, _ = _world(game, n, batch_frames, hip_lib, oracle_lib)
    for objective in OBJECTIVES:
        res = g.lookahead_beam_samples(frames, depth, width, samples, hold=hold, objective=objective, seed=DRAWN["seed"], t=DRAWN["t"], env_offset=DRAWN["env_offset"])
        assert (res["samples"] == samples).all()
        for a in range(len(LEGAL[game])):
            assert (res["code"][:, a] % np.uint64(len(LEGAL[game])) == a).all()
            calls = []
            for s in range(samples):
                args, _ = plan_args(game, n, frames, hold=hold, depth=depth, code=res["code"][:, a], rest=None, seed=sample_seed(DRAWN["seed"], s), t=DRAWN["t"],
                                    env_offset=DRAWN["env_offset"])
                calls.append(Engine._lookahead_dict(g.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args)))
            leaves = {k: np.stack([np.asarray(x[k]).astype(np.int64)[:, None] for x in calls]) for k in LEAF_FIELDS}
            sums = aggregate_samples(leaves, np.ones((samples, n), bool))
            for k in SAMPLE_FIELDS:
                assert np.array_equal(sums[k][:, 0], res[k][:, a]), (game, objective, a, k)


# ---------------------------------------------------------------- 4. cuts change no bit

def _device_form(g, args, L):
    """tbx_reduce_device with shared arguments on a caller's stream"""
    from toybox_amd import hip
    n = g.n_envs
    s = hip.Stream()
    o_dev = hip.malloc(n * 9 * L * 8)
    try:
        g.reduce_device(QUERY, o_dev, args=args, stream=s.ptr)
        s.synchronize()
        rows = np.empty((n, 9 * L), np.float64)
        hip.memcpy_dtoh(rows, o_dev, rows.nbytes)
    finally:
        g.sync()
        hip.free(o_dev)
        s.close()
    return rows


@pytest.mark.parametrize("game", GAMES)
def test_cuts_change_no_bit(game, hip_lib, oracle_lib):
    """sample chunks (TBX_OPT_BEAM_SAMPLES_MAX_CHUNKS = 1 against the engine's choice, which at 24 envs cuts level 1: 5 samples in 4
    chunks of 1, 1, 1, 2), env ranges (TBX_OPT_BEAM_RANGE_ENVS = 5 on 24 envs: five ranges, the last of four envs) and the host
    form against the device form on a caller's stream, with shared arguments and with the same row for every env (budgeted as the
    largest valid row: several ranges, every level up to TBX_PLAN_MAX_DEPTH launched)"""
    n, L = 24, len(LEGAL[game])
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    call = dict(frames=40, depth=5, width=3, samples=5, hold=4, objective="survival", salt=0 if game == "gridworld" else 7, seed=(9 << 34) | 1, t=2 ** 32 - 2, env_offset=5)
    base = g.lookahead_beam_samples(**call)
    assert g.beam_samples_chunks == 4 and g.beam_samples_ranges == 1 and g.get_option(_abi.OPT_BEAM_SAMPLES_MAX_CHUNKS) == 0
    assert (base["samples"] == 5).all() and len(np.unique(base["code"])) > L
    try:
        g.set_option(_abi.OPT_BEAM_SAMPLES_MAX_CHUNKS, 1)
        whole = g.lookahead_beam_samples(**call)
        assert g.beam_samples_chunks == 1 and g.get_option(_abi.OPT_BEAM_SAMPLES_MAX_CHUNKS) == 1
        g.set_option(_abi.OPT_BEAM_SAMPLES_MAX_CHUNKS, 2)
        halves = g.lookahead_beam_samples(**call)
        assert g.beam_samples_chunks == 2
    finally:
        g.set_option(_abi.OPT_BEAM_SAMPLES_MAX_CHUNKS, 0)
    _assert_same_rows(whole, base, "one chunk")
    _assert_same_rows(halves, base, "two chunks")
    g.beam_range_envs = 5
    try:
        cut = g.lookahead_beam_samples(**call)
        assert g.beam_samples_ranges == 5 and g.beam_samples_chunks == 4
    finally:
        g.beam_range_envs = 0
    _assert_same_rows(cut, base, "five ranges")
    args, per_env = beam_samples_args(game, n, **call)
    assert not per_env
    dev = g._search_samples_dict(_device_form(g, args, L).reshape(n, L, 9), 5)
    _assert_same_rows(dev, base, "device form, shared arguments")
    rows = np.tile(np.asarray(args, np.float64), (n, 1))
    dev = g._search_samples_dict(_device_reduce(g, QUERY, rows, 9 * L).reshape(n, L, 9), 5)
    assert g.beam_samples_ranges == UNSEEN_ROW_RANGES[game], "rows the host has not seen are budgeted as the largest valid row"
    _assert_same_rows(dev, base, "device form, one row per env")
    host = g._search_samples_dict(g.reduce(QUERY, rows).reshape(n, L, 9), 5)
    assert g.beam_samples_ranges == 1, "rows the host has seen are budgeted as they are"
    _assert_same_rows(host, base, "host form, one row per env")


# ---------------------------------------------------------------- 5. per-env rows with bad rows among them

@pytest.mark.parametrize("game", GAMES)
def test_per_env_rows_with_bad_rows_among_them(game, hip_lib, oracle_lib):
    """mixed depths, widths, sample counts, salts, objectives and holds, one row per refusal reason; the host form (its bounds come
    from the valid rows alone) and the device form on a caller's stream: refused rows are nine zeros, the others the replay's, and
    nothing in the engine changes"""
    n = 24
    g, states, rngs = _world(game, n, 40 if game == "gridworld" else 400, hip_lib, oracle_lib)
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    s = dict(frames=np.full(n, 24), hold=np.resize([4, 2, 8], n), depth=np.resize([1, 2, 3, 4], n), objective=np.resize([0, 1], n), rest=np.full(n, -1),
             width=np.resize([1, 2, 3, 2, 2], n), samples=np.resize([3, 1, 2], n), salt=np.resize([0, 1000, 5, 0], n), seed=(0xC0FFEE << 32) | 0x5EED, t=2 ** 32 - 2,
             env_offset=99)
    if game == "gridworld":
        s["salt"][:] = 0
    s["depth"][[1, 2]] = [0, top + 1]
    s["width"][[4, 5]] = [0, 65]
    s["samples"][[7, 8]] = [0, 4097]
    s["salt"][10], s["samples"][10] = 2 ** 32 - 2, 3          # (2^32 - 2) + 3 - 1 = 2^32: one too many
    s["salt"][[11, 12]] = [-1, 2 ** 32]
    s["depth"][13], s["width"][13], s["samples"][13] = 5, 64, _abi.LOOKAHEAD_MAX_LEAVES // (L * 64 * L) + 1      # the leaf cap
    s["rest"][15] = 2 if game == "breakout" else 17
    s["objective"][16] = 2
    s["frames"][[18, 19]] = [0, 1025]
    s["hold"][21] = 0
    bad = [1, 2, 4, 5, 7, 8, 10, 11, 12, 13, 15, 16, 18, 19, 21]
    good = np.setdiff1d(np.arange(n), bad)
    want, _ = expected_beam_samples(oracle_lib, game, states, rngs, s)
    assert all((want[k][bad] == 0).all() for k in ROW_FIELDS) and np.array_equal(want["samples"][good, 0], s["samples"][good])
    assert len({(int(s["depth"][i]), int(s["width"][i]), int(s["samples"][i]), int(s["objective"][i])) for i in good}) >= 6
    args, per_env = beam_samples_args(game, n, **s)
    assert per_env and args.shape == (n, 12)
    before = _snapshot(g)
    host = g._search_samples_dict(g.reduce(QUERY, args).reshape(n, L, 9), s["depth"])
    assert g.beam_samples_ranges == 1
    assert_rows_equal(host, want, "%s per-env rows (host form)" % game)
    dev = g._search_samples_dict(_device_reduce(g, QUERY, args, 9 * L).reshape(n, L, 9), s["depth"])
    assert g.beam_samples_ranges == UNSEEN_ROW_RANGES[game], "the device form crosses range seams (Breakout: TBX_OPT_BEAM_RANGE_ENVS does, in test_cuts_change_no_bit)"
    assert_rows_equal(dev, want, "%s per-env rows (device form)" % game)
    _assert_same_snapshot(_snapshot(g), before, "%s per-env rows" % game)
    # the rows at the cap are answered: one sample fewer than the refused row has
    s["samples"][13] -= 1
    s["frames"][13] = 2
    args, _ = beam_samples_args(game, n, **s)
    at_cap = g.reduce(QUERY, args).reshape(n, L, 9)
    assert (at_cap[13, :, 0] == s["samples"][13]).all() and (at_cap[bad[:9], :, :] == 0).all()


# ---------------------------------------------------------------- 6. refusals

@pytest.mark.parametrize("game", GAMES)
def test_shared_refusals(game, hip_lib, oracle_lib):
    """TBX_E_INVALID with a message that names the argument, nothing launched (the range and chunk counters of the last call
    stand), nothing changed"""
    g, _, _ = _world(game, 24, 40 if game == "gridworld" else 400, hip_lib, oracle_lib)
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    illegal = 2 if game == "breakout" else 17
    g.beam_range_envs = 7
    try:
        assert g.lookahead_beam_samples(8, 2, 2, 2)["samples"].shape == (24, L)
        counters = (g.beam_samples_ranges, g.beam_samples_chunks)
        assert counters[0] == 4
    finally:
        g.beam_range_envs = 0
    before = _snapshot(g)
    head, tail = [8, 1, 2, 0], [-1, 0, 0, 0, 0]
    cap = _abi.LOOKAHEAD_MAX_LEAVES // (L * 64 * L)
    bad = {"frames 0": ([0], "frames"), "frames 1025": ([1025], "frames"), "hold 0": ([8, 0], "hold"), "depth 0": ([8, 1, 0], "depth"),
           "depth above the top": ([8, 1, top + 1], "depth"), "objective 2": ([8, 1, 2, 2], "objective"), "illegal rest": ([8, 1, 2, 0, illegal], "rest"),
           "width 0": (head + tail + [0], "width"), "width 65": (head + tail + [65], "width"), "samples 0": (head + tail + [2, 0], "samples"),
           "samples 4097": (head + tail + [2, 4097], "samples"), "too many leaves": ([8, 1, 5, 0] + tail + [64, cap + 1], "TBX_LOOKAHEAD_MAX_LEAVES"),
           "too many leaves at the top": ([8, 1, top, 0] + tail + [64, cap + 1], "TBX_LOOKAHEAD_MAX_LEAVES"), "salt -1": (head + tail + [2, 2, -1], "salt"),
           "salt 2^32": (head + tail + [2, 2, 2 ** 32], "salt"), "salt + samples": (head + tail + [2, 3, 2 ** 32 - 2], "salt"),
           "thirteen arguments": (head + tail + [2, 2, 0, 0], "samples, salt]"), "no arguments": ([], "samples, salt]")}
    for what, (args, word) in bad.items():
        with pytest.raises(ToyboxAmdError) as ei:
            g.reduce(QUERY, args)
        assert ei.value.code == _abi.E_INVALID and word in str(ei.value), (what, str(ei.value))
        assert (g.beam_samples_ranges, g.beam_samples_chunks) == counters, "%s: a refusal leaves the counters standing" % what
    _assert_same_snapshot(_snapshot(g), before, "%s after the refusals" % game)
    rows = g.reduce(QUERY, [8, 1, top, 1] + tail + [64, cap]).reshape(24, L, 9)                  # the deepest, widest beam at the leaf cap
    assert (rows[..., 0] == cap).all() and g.beam_samples_ranges == 1
    for option in (_abi.OPT_BEAM_SAMPLES_RANGES, _abi.OPT_BEAM_SAMPLES_CHUNKS):
        with pytest.raises(ToyboxAmdError):
            g.set_option(option, 1)
    for value in (-1, 4097):
        with pytest.raises(ToyboxAmdError):
            g.set_option(_abi.OPT_BEAM_SAMPLES_MAX_CHUNKS, value)
    assert g.get_option(_abi.OPT_BEAM_SAMPLES_MAX_CHUNKS) == 0


# ---------------------------------------------------------------- 7. the width of a row

def test_reduce_width(hip_lib):
    for name in GAMES:
        assert hip_lib.tbx_reduce_width(_abi.GAME_IDS[name], QUERY) == 9 * len(LEGAL[name])


# ---------------------------------------------------------------- 8. the adapters and the batch intervention

@pytest.mark.parametrize("preproc", [False, True])
def test_the_adapters_against_the_engine(preproc, hip_lib, oracle_lib):
    """beam_search_samples on 8 envs: steps (agent steps: x skip frames, held), action indices, the engine's rows, the means and
    the winner among an env's rows"""
    from toybox_amd.envs import ToyboxPreprocVecEnv, ToyboxVecEnv
    from toybox_amd.envs.vec_env import sample_best_action
    game, n = "space_invaders", 8
    L = len(LEGAL[game])
    cls = ToyboxPreprocVecEnv if preproc else ToyboxVecEnv
    v = cls(game, n, seed=3, engine=Engine(game, n, lib=hip_lib))
    v.reset()
    rng = np.random.default_rng(0)
    for _ in range(20):
        v.step(rng.integers(0, v.action_space.n, n))
    v.step_async(rng.integers(0, v.action_space.n, n))        # a pending step ends first
    frames, hold = (12 * 4, 4) if preproc else (40, 1)
    for objective in OBJECTIVES:
        got = v.beam_search_samples(steps=12 if preproc else 40, depth=5, width=2, samples=3, objective=objective, rest=None, seed=11, t=4, salt=1000)
        rows = v.engine.lookahead_beam_samples(frames, 5, 2, 3, hold=hold, objective=objective, salt=1000, seed=11, t=4)
        assert_rows_equal(got, rows, "%s.beam_search_samples %s against the engine" % (cls.__name__, objective))
        digits = np.stack([rows["code"].astype(np.int64) // L ** p % L for p in range(5)], axis=-1)
        assert np.array_equal(got["plan"], digits) and np.array_equal(np.asarray(LEGAL[game])[got["plan"]], rows["plan"])
        assert np.array_equal(got["ret_mean"], rows["ret_sum"] / 3.0) and np.array_equal(got["lost_frac"], rows["lost"] / 3.0)
        best = sample_best_action(rows, objective)
        assert np.array_equal(got["best_action"], best) and np.array_equal(got["best_plan"], got["plan"][np.arange(n), best])
        assert np.array_equal(got["best_plan"][:, 0], got["best_action"]), "the first digit of the best plan is the best action"
        assert (rows["samples"] == 3).all()
    v.close()


def test_batch_intervention_mirrors_the_engine(hip_lib, oracle_lib):
    from toybox_amd.interventions import BatchIntervention
    game, n, first, count = "breakout", 24, 5, 11
    g, _, _ = _world(game, n, 400, hip_lib, oracle_lib)
    depth, width, samples = np.resize([7, 2, 5], n), np.resize([2, 3], n), np.resize([2, 3, 1, 4], n)
    whole = g.lookahead_beam_samples(48, depth, width, samples, hold=4, objective="survival", salt=9)
    with BatchIntervention(g, first, count) as bi:
        part = bi.lookahead_beam_samples(48, depth[first:first + count], width[first:first + count], samples[first:first + count], hold=4, objective="survival", salt=9)
    for k in ROW_FIELDS:
        assert np.array_equal(part[k], whole[k][first:first + count]), k
    assert np.array_equal(whole["samples"][:, 0], samples)
