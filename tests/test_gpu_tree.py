"""Tree search on the device (TBX_QUERY_LOOKAHEAD_TREE, include/toybox_amd.h) against SELECT, CLONE, SALT AND PLAY simulation by
simulation on the CPU checker (tests/tree_replay.py; its own checks are in tests/test_tree.py).  Every comparison is exact, on
every field of every row.

The worlds are those of tests/test_gpu_search.py (_world): made by the input recipe of tests/lookahead_replay.py and held to their
checker twins byte for byte before any query; the expected rows are played on clones of the records the DEVICE engine reports.
Common shape: 24 envs behind 400 frames of synthetic play (GridWorld 40), hold 4 (GridWorld 2), frames = hold x 12.  Cases (tests/
tree_replay.py, case_tree): tree -- depth 3, M = 12 L, explore 0 and explore 64; drawn -- drawn rest actions under a seed above 32
bits, t = 2^32 - 3, env_offset 70000, salt 1000, objective 1; deepest -- depth TBX_PLAN_MAX_DEPTH, frames = hold x depth,
M = L x depth + 8; cut -- the explore case under TBX_OPT_BEAM_RANGE_ENVS = 7 and TBX_OPT_TREE_LAUNCH_SIMULATIONS = 5; rows -- per-env
rows with bad rows among them through both forms.
Measured on the checker (tests/test_tree.py prints them), per case tree / explore / drawn / deepest -- selection steps decided by
priority; of them with the two best tied; simulations at full depth without an expansion; principal-variation steps decided by a
tie-break; simulations whose game ended; simulations with a return above 0:
  Breakout      8064 / 6912 / 6912 / 57600;     7976 / 5439 / 5049 / 57464;    3840 / 2688 / 2688 / 1152;  0 / 192 / 167 / 0;  2010 / 1934 / 1867 / 3296;  329 / 252 / 254 / 785
  SpaceInvaders 18144 / 13824 / 13824 / 69696;  17250 / 11592 / 12156 / 53234; 8640 / 4320 / 4320 / 2016;  0 / 275 / 288 / 0;  296 / 364 / 368 / 328;      2481 / 2272 / 3976 / 5056
  Amidar        18144 / 13824 / 13824 / 69696;  17438 / 12084 / 10354 / 68902; 8640 / 4320 / 4320 / 2016;  0 / 288 / 262 / 0;  590 / 718 / 791 / 705;      1167 / 734 / 1280 / 1303
  GridWorld     12600 / 10200 / 10200 / 58320;  12545 / 8205 / 8267 / 58252;   6000 / 3600 / 3600 / 1560;  0 / 120 / 120 / 0;  0 / 0 / 2 / 0;              56 / 36 / 545 / 69
and explore 64 changes 3936 / 9196 / 9214 / 6240 played codes of the tree case.  The replay of a case takes 0.2 to 0.7 s on an
8-core host (the L trees of every env are played side by side in one checker clone per simulation).
The module on an MI355X box: 39 cases in 5.9 s, the longest (Breakout, tree) 0.42 s, most of it the checker's replay."""
import functools

import numpy as np
import pytest

from fork_replay import sim_rngs
from lookahead_replay import batch
from sample_replay import assert_samples_equal
from support import LEGAL
from test_gpu_search import _assert_same_snapshot, _device_reduce, _held_to_twin, _snapshot, _world
from toybox_amd import ToyboxAmdError, _abi
from toybox_amd.engine import TREE_FIELDS, Engine, plan_args, sample_seed, tree_args
from tree_replay import BATCH_FRAMES, ENVS, HOLD, assert_tree_equal, case_tree, expected_tree, played_codes_differ

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
TREE = _abi.QUERY_LOOKAHEAD_TREE


@functools.lru_cache(maxsize=None)
def _replay(game, name, hip_lib, oracle_lib):
    """(rows, log) of the case replayed on the checker, made once, shared and left unchanged"""
    _, states, rngs = _world(game, ENVS, BATCH_FRAMES[game], hip_lib, oracle_lib)
    rows, log, _ = expected_tree(oracle_lib, game, states, rngs, case_tree(game, name))
    for v in rows.values():
        v.flags.writeable = False
    return rows, log


def _ask(g, tree, **more):
    """Engine.lookahead_tree with the keyword arguments of expected_tree"""
    kw = dict(tree, **more)
    rest = kw.pop("rest", -1)
    return g.lookahead_tree(kw.pop("frames"), kw.pop("depth"), kw.pop("simulations"), rest=None if np.ndim(rest) == 0 and rest == -1 else rest, **kw)


def _tree_dict(rows, n, L):
    rows = np.asarray(rows).reshape(n, L, 12)
    return {k: rows[..., i].astype(np.int64) for i, k in enumerate(TREE_FIELDS)}


# ---------------------------------------------------------------- 1. rows equal the replay

@pytest.mark.parametrize("name", ["tree", "tree_explore", "drawn", "deepest"])
@pytest.mark.parametrize("game", GAMES)
def test_tree_equals_replay(game, name, hip_lib, oracle_lib):
    tree = case_tree(game, name)
    L = len(LEGAL[game])
    g, _, _ = _world(game, ENVS, BATCH_FRAMES[game], hip_lib, oracle_lib)
    want, _ = _replay(game, name, hip_lib, oracle_lib)
    got = _ask(g, tree)
    assert got["samples"].shape == (ENVS, L) and got["code"].dtype == np.uint64 and tuple(got) == TREE_FIELDS
    assert_tree_equal(got, want, "%s %s" % (game, name))
    assert g.tree_ranges == 1 and (want["samples"] == tree["simulations"]).all() and (want["code"] % L == np.arange(L)).all()
    if name == "deepest":
        assert tree["depth"] == _abi.PLAN_MAX_DEPTH[game] and (want["pv_depth"] == tree["depth"]).any(), "a principal variation of the full depth"
    if name == "tree_explore":
        assert played_codes_differ(_replay(game, "tree", hip_lib, oracle_lib)[1], _replay(game, name, hip_lib, oracle_lib)[1]) > 0
        assert any(not np.array_equal(want[k], _replay(game, "tree", hip_lib, oracle_lib)[0][k]) for k in TREE_FIELDS), "explore changes no row"
    if name == "drawn":
        other = _ask(g, dict(tree, seed=tree["seed"] ^ (1 << 40)))
        assert any(not np.array_equal(other[k], got[k]) for k in TREE_FIELDS), "the upper half of the seed is not read"
    again = _ask(g, tree)                                     # (v) two equal calls with no step between them
    assert all(np.array_equal(again[k], got[k]) for k in TREE_FIELDS)


@pytest.mark.parametrize("game", GAMES)
def test_cuts_change_no_bit(game, hip_lib, oracle_lib):
    """TBX_OPT_BEAM_RANGE_ENVS = 7 on 24 envs and TBX_OPT_TREE_LAUNCH_SIMULATIONS = 5: four ranges, the last of three envs, the
    simulations in launches of five (M = 48 and 72: a shorter last one) -- the uncut rows and the replay's"""
    tree = case_tree(game, "tree_explore")
    g, _, _ = _world(game, ENVS, BATCH_FRAMES[game], hip_lib, oracle_lib)
    one = _ask(g, tree)
    assert g.tree_ranges == 1 and g.beam_range_envs == 0 and g.tree_launch_simulations == 0 and tree["simulations"] > 5
    g.beam_range_envs = 7
    g.tree_launch_simulations = 5
    try:
        cut = _ask(g, tree)
        assert g.get_option(_abi.OPT_TREE_RANGES) == 4 and g.tree_launch_simulations == 5
        with pytest.raises(ToyboxAmdError):
            g.set_option(_abi.OPT_TREE_LAUNCH_SIMULATIONS, _abi.TREE_MAX_SIMULATIONS + 1)
    finally:
        g.beam_range_envs = 0
        g.tree_launch_simulations = 0
    for k in TREE_FIELDS:
        assert np.array_equal(one[k], cut[k]), k
    assert_tree_equal(cut, _replay(game, "tree_explore", hip_lib, oracle_lib)[0], "%s cut" % game)


# ---------------------------------------------------------------- 2. the device equals itself: the consequences of the definition

@pytest.mark.parametrize("game", GAMES)
def test_the_consequences_hold_on_the_device(game, hip_lib, oracle_lib):
    n, L, hold = ENVS, len(LEGAL[game]), HOLD[game]
    g, _, _ = _world(game, n, BATCH_FRAMES[game], hip_lib, oracle_lib)
    sched = dict(frames=hold * 10, hold=hold, rest=None, seed=(9 << 32) | 3, t=9, env_offset=5)
    for objective in ("return", "survival"):
        # (i) depth 1: query 154's row from the same library, and [8 .. 10] = a, 1, M
        flat = g.lookahead_tree(sched["frames"], 1, 9, explore=50, salt=1000, objective=objective, **{k: sched[k] for k in ("hold", "rest", "seed", "t", "env_offset")})
        assert_samples_equal(flat, g.lookahead_samples(sched["frames"], 9, salt=1000, **{k: sched[k] for k in ("hold", "rest", "seed", "t", "env_offset")}), "%s (i)" % game)
        assert np.array_equal(flat["code"], np.tile(np.arange(L, dtype=np.uint64), (n, 1))) and (flat["pv_depth"] == 1).all() and (flat["pv_visits"] == 9).all()
        assert np.array_equal(flat["pv_value"], flat["ret_sum"] if objective == "return" else flat["safe_frames_sum"])
        # (ii) M = L at depth 2: simulation m is the plan query for code a + m L under the seed of future m -- summed, the root
        two = g.lookahead_tree(sched["frames"], 2, L, explore=50, objective=objective, **{k: sched[k] for k in ("hold", "rest", "seed", "t", "env_offset")})
        for a in range(L):
            plans = []
            for m in range(L):
                args, _ = plan_args(game, n, sched["frames"], hold=hold, depth=2, code=a + m * L, rest=None, seed=sample_seed(sched["seed"], m), t=9, env_offset=5)
                plans.append(Engine._lookahead_dict(g.reduce(_abi.QUERY_LOOKAHEAD_PLAN, args)))
            ret = np.stack([p["ret"] for p in plans]).astype(np.int64)
            safe = np.stack([np.where(p["life_lost_at"] < 0, p["frames_run"], p["life_lost_at"]) for p in plans])
            assert np.array_equal(two["ret_sum"][:, a], ret.sum(0)) and np.array_equal(two["ret_min"][:, a], ret.min(0)) and np.array_equal(two["ret_max"][:, a], ret.max(0))
            assert np.array_equal(two["safe_frames_sum"][:, a], safe.sum(0)) and np.array_equal(two["lives_sum"][:, a], np.stack([p["lives"] for p in plans]).sum(0))
            value = ret if objective == "return" else safe
            best = value.argmax(0)                            # one visit each: the larger v_sum, then the smaller k
            assert np.array_equal(two["code"][:, a].astype(np.int64), a + best * L) and np.array_equal(two["pv_value"][:, a], value.max(0)), (game, objective, a)
        assert (two["pv_depth"] == 2).all() and (two["pv_visits"] == 1).all() and (two["samples"] == L).all()
        # (iii) pv_depth >= 2 once there is a depth to go to
        deep = g.lookahead_tree(sched["frames"], 4, 3 * L + 1, explore=50, objective=objective, **{k: sched[k] for k in ("hold", "rest", "seed", "t", "env_offset")})
        assert (deep["pv_depth"] >= 2).all() and (deep["pv_depth"] <= 4).all() and (deep["pv_visits"] >= 1).all() and (deep["samples"] == 3 * L + 1).all()


# ---------------------------------------------------------------- 3. per-env rows with bad rows among them

@pytest.mark.parametrize("game", GAMES)
def test_per_env_rows_with_bad_rows_among_them(game, hip_lib, oracle_lib):
    """depth, simulations, explore and objective differing by env, one row per refusal reason; the host form (which scans its rows)
    and the device form on a caller's stream (which cannot, and runs every launch): refused rows are zeros, the others the
    replay's and those of shared arguments"""
    n = ENVS
    g, states, rngs = _world(game, n, BATCH_FRAMES[game], hip_lib, oracle_lib)
    L, top, hold = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game], HOLD[game]
    s = dict(frames=np.full(n, hold * 8), hold=np.resize([hold, 2 * hold, 1], n), depth=np.resize([1, 2, 3, 5], n), objective=np.resize([0, 1], n),
             rest=np.full(n, LEGAL[game][0]), simulations=np.resize([1, 5, 2 * L + 3, 20, 2], n), explore=np.resize([0, 30, 1000, 2 ** 20], n),
             salt=np.resize([0, 1000, 2 ** 32 - 20], n))
    s["simulations"][1] = 0
    s["simulations"][2] = 1025
    s["explore"][5] = -1
    s["explore"][8] = 2 ** 20 + 1
    s["salt"][10] = 2 ** 32
    s["salt"][11], s["simulations"][11] = 2 ** 32 - 3, 5      # salt + simulations - 1 leaves 32 bits
    s["depth"][13] = 0
    s["depth"][14] = top + 1
    s["objective"][16] = 2
    s["frames"][17] = 1025
    s["rest"][19] = 2 if game == "breakout" else 17
    bad = [1, 2, 5, 8, 10, 11, 13, 14, 16, 17, 19]
    good = np.setdiff1d(np.arange(n), bad)
    want, _, _ = expected_tree(oracle_lib, game, states, rngs, s)
    assert all((want[k][bad] == 0).all() for k in TREE_FIELDS) and np.array_equal(want["samples"][good], np.tile(s["simulations"][good][:, None], (1, L)))
    assert len(np.unique(s["depth"][good])) >= 3 and len(np.unique(s["simulations"][good])) >= 3 and len(np.unique(s["explore"][good])) >= 3
    args, per_env = tree_args(game, n, s["frames"], s["depth"], s["simulations"], s["explore"], s["salt"], hold=s["hold"], objective=s["objective"], rest=s["rest"])
    assert per_env and args.shape == (n, 12)
    before = _snapshot(g)
    assert_tree_equal(_tree_dict(g.reduce(TREE, args), n, L), want, "%s tree rows (host form)" % game)
    assert_tree_equal(_tree_dict(_device_reduce(g, TREE, args, 12 * L), n, L), want, "%s tree rows (device form)" % game)
    _assert_same_snapshot(_snapshot(g), before, "%s per-env rows" % game)
    keys = ("frames", "hold", "depth", "objective", "simulations", "explore", "salt")
    for i in good[:6]:                                        # the same envs asked alone, with shared arguments
        shared = _ask(g, {k: int(s[k][i]) for k in keys}, rest=LEGAL[game][0])
        for k in TREE_FIELDS:
            assert np.array_equal(np.asarray(shared[k][i], np.int64), want[k][i]), (game, i, k)


# ---------------------------------------------------------------- 4. forms

def test_breakout_wave_per_env_step_form(hip_lib, oracle_lib):
    """TBX_OPT_STEP_FORM = 2: the canonical wall through the wave form -- lane 0 walks the tree, depth and code are broadcast"""
    n, game = ENVS, "breakout"
    g = Engine(game, n, lib=hip_lib)
    g.set_option(_abi.OPT_STEP_FORM, _abi.STEP_FORM_WAVE_PER_ENV)
    o = batch(oracle_lib, game, n)
    g.set_states(0, o.get_states())
    for i, r in enumerate(sim_rngs(o)):
        g.set_sim_rng((int(r[0]), int(r[1])), env=i)
    _held_to_twin(g, o, "breakout, wave per env")
    states, rngs = g.get_states(), sim_rngs(g)
    for name in ("tree_explore", "drawn"):
        tree = case_tree(game, name)
        g.tree_launch_simulations = 7 if name == "drawn" else 0
        assert_tree_equal(_ask(g, tree), expected_tree(oracle_lib, game, states, rngs, tree)[0], "breakout, wave per env, %s" % name)
    _held_to_twin(g, o, "breakout, wave per env, after the queries")
    g.close(); o.close()


@pytest.mark.parametrize("cls", ["ToyboxVecEnv", "ToyboxPreprocVecEnv"])
def test_the_adapters(cls, hip_lib, oracle_lib):
    """tree_search: (agent) steps, action indices, the engine's rows, the winner among an env's rows and its plan; the next
    observation is untouched"""
    from sample_replay import best_action
    from toybox_amd import envs
    game, n, depth = "space_invaders", ENVS, 4
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
    for o, objective in enumerate(("return", "survival")):
        got = v.tree_search(10, depth, 20, explore=40, objective=objective, rest=0, seed=5, salt=9)
        assert v._in_flight is None and getattr(v, "_pending", None) is None
        tree = dict(frames=10 * skip, hold=skip, depth=depth, simulations=20, explore=40, rest=LEGAL[game][0], seed=5, salt=9, objective=o)
        want, _, _ = expected_tree(oracle_lib, game, v.engine.get_states(), sim_rngs(v.engine), tree)
        assert_tree_equal(got, want, "%s.tree_search %s" % (cls, objective))
        best = best_action(want, objective)
        assert np.array_equal(got["best_action"], best) and got["best_plan"].shape == (n, depth)
        for i in range(n):
            d, code = int(want["pv_depth"][i, best[i]]), int(want["code"][i, best[i]])
            assert got["best_plan"][i].tolist() == [code // L ** p % L for p in range(d)] + [-1] * (depth - d) and got["best_plan"][i, 0] == best[i]
    a = rng.integers(0, v.action_space.n, n)
    for x, y in zip(v.step(a)[:3], twin.step(a)[:3]):
        assert np.array_equal(np.asarray(x), np.asarray(y)), "%s: the step after the queries differs from an untouched twin's" % cls
    v.close(); twin.close()


# ---------------------------------------------------------------- 5. nothing written

@pytest.mark.parametrize("game", GAMES)
def test_the_query_leaves_the_engine_untouched(game, hip_lib, oracle_lib):
    """state records, both RNGs (the game's lies in the records), step outputs, scalars and TBX_BUF_PLAN_* are byte-equal before and
    after a query of several ranges and launches, and the next synthetic step gives what an untouched twin gives"""
    n = ENVS
    g, twin = batch(hip_lib, game, n), batch(hip_lib, game, n)
    g.step_synthetic(1337, 399, auto_reset=True); twin.step_synthetic(1337, 399, auto_reset=True)
    g.lookahead_act("search", frames=8, depth=1)              # (TBX_BUF_PLAN_ACTION / _CARRY exist from here on)
    before, plan_before = _snapshot(g), g.plan_buffers()
    g.beam_range_envs = 7
    g.tree_launch_simulations = 4
    out = g.lookahead_tree(HOLD[game] * 10, 5, 30, explore=64, salt=77, hold=HOLD[game], objective="survival")
    assert g.tree_ranges == 4 and (out["samples"] == 30).all()
    g.beam_range_envs = 0
    g.tree_launch_simulations = 0
    _assert_same_snapshot(_snapshot(g), before, game)
    assert all(np.array_equal(x, y) for x, y in zip(g.plan_buffers(), plan_before)), "%s: TBX_BUF_PLAN_* changed" % game
    for e in (g, twin):
        e.step_synthetic(1337, 400, auto_reset=True)
    _assert_same_snapshot(_snapshot(g), _snapshot(twin), "%s: the step after the query" % game)
    g.close(); twin.close()


# ---------------------------------------------------------------- 6. shared refusals

@pytest.mark.parametrize("game", GAMES)
def test_shared_refusals(game, hip_lib, oracle_lib):
    """TBX_E_INVALID before anything is launched: the message names the value, TBX_OPT_TREE_RANGES stands, a caller's output buffer
    keeps its bytes"""
    from toybox_amd import hip
    n = ENVS
    g, _, _ = _world(game, n, BATCH_FRAMES[game], hip_lib, oracle_lib)
    L, top = len(LEGAL[game]), _abi.PLAN_MAX_DEPTH[game]
    illegal = 2 if game == "breakout" else 17
    g.lookahead_tree(8, 2, 3)
    ranges, before = g.tree_ranges, _snapshot(g)
    assert ranges == 1
    tail = [8, 1, 2, 0, -1, 0, 0, 0, 0]
    bad = {"depth": [[8, 1, 0], [8, 1, top + 1]], "objective": [[8, 1, 2, 2]], "rest": [[8, 1, 2, 0, illegal]], "frames": [[0], [1025]], "hold": [[8, 0]],
           "simulations": [tail + [0], tail + [1025]], "explore": [tail + [4, -1], tail + [4, 2 ** 20 + 1]],
           "salt": [tail + [4, 1, -1], tail + [4, 1, 2 ** 32], tail + [4, 1, 2 ** 32 - 3]], "tree takes": [tail + [4, 1, 1, 0], []]}
    pattern = np.arange(n * 12 * L, dtype=np.float64) + 0.5
    o_dev = hip.malloc(pattern.nbytes)
    g.beam_range_envs = 5
    try:
        hip.memcpy_htod(o_dev, pattern, pattern.nbytes)
        for name, rows in bad.items():
            for args in rows:
                with pytest.raises(ToyboxAmdError) as ei:
                    g.reduce(TREE, args)
                assert ei.value.code == _abi.E_INVALID and name in str(ei.value), (name, args, str(ei.value))
                if args:
                    with pytest.raises(ToyboxAmdError) as ei:
                        g.reduce_device(TREE, o_dev, args)
                    assert ei.value.code == _abi.E_INVALID and name in str(ei.value), (name, args, str(ei.value))
                assert g.tree_ranges == ranges, "a refusal leaves TBX_OPT_TREE_RANGES standing"
        g.sync()
        back = np.empty_like(pattern)
        hip.memcpy_dtoh(back, o_dev, back.nbytes)
        assert np.array_equal(back, pattern), "a refused query wrote into the output buffer"
    finally:
        g.beam_range_envs = 0
        g.sync()
        hip.free(o_dev)
    _assert_same_snapshot(_snapshot(g), before, "%s after the refusals" % game)
    # the largest tree there is on the shortest horizon: the deepest plans, every simulation, the largest explore and salt
    out = g.reduce(TREE, [top, 1, top, 1, -1, 0, 0, 0, 0, 1024, 2 ** 20, 2 ** 32 - 1024])
    assert out.shape == (n, 12 * L) and (out.reshape(n, L, 12)[..., 0] == 1024).all()
    with pytest.raises(ToyboxAmdError):
        g.set_option(_abi.OPT_TREE_RANGES, 1)
    for name in GAMES:
        assert hip_lib.tbx_reduce_width(_abi.GAME_IDS[name], TREE) == 12 * len(LEGAL[name])
