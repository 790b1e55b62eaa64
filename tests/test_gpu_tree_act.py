"""Closed-loop tree search on the device (TBX_QUERY_LOOKAHEAD_TREE_ACT, TBX_EDIT_TREE_DROP, include/toybox_amd.h) against START TREES,
SEARCH, PICK, CARRY, STEP on the CPU checker (tests/tree_act_replay.py; its own checks are in tests/test_tree_act.py).  Every
comparison is exact: the rows, TBX_BUF_PLAN_ACTION and TBX_BUF_PLAN_TREE node by node after every call.

Loops: per game 24 envs behind 400 frames of synthetic play (GridWorld 40) -- 96 to 144 units, never a multiple of 64 -- depth 3,
6 L simulations, 5 periods queued on ONE caller's stream with no host synchronisation between them: the query, copies of its rows,
of the action buffer and of the store, then `hold` device steps that read the action buffer.  The loops are those of
tree_act_replay.loop_tree; tests/test_tree_act.py holds them to the coverage list on the checker.  The adapters: plan_rollout(3, "tree")
of ToyboxVecEnv against the replay with games ending inside the window, of ToyboxPreprocVecEnv against plan_step calls and the
engine's own calls AND the replay on a checker twin.  The device-mask drop cases end their games through the batch's WRITTEN lives
(lookahead_replay.batch sets lives = 1 in two envs of three with TBX_EDIT_SET_LIVES; GridWorld has none to write), asserted to happen
inside the window.  The module's 68 cases took 18 s on an MI355X box, the longest 0.9 s."""

import numpy as np
import pytest

import tree_act_replay as R
from fork_replay import sim_rngs
from lookahead_replay import clone
from support import LEGAL, read_buffer
from test_gpu_search import _assert_same_snapshot, _snapshot, _world
from toybox_amd import ToyboxAmdError, _abi, hip
from toybox_amd.engine import TREE_FIELDS, plan_pick, tree_store_units

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]


def _args(tree, reuse):
    """the shared row of a replay case, every column written out"""
    seed = int(tree.get("seed", 0))
    row = [tree["frames"], tree.get("hold", 1), tree.get("depth", 1), tree.get("objective", 0), tree.get("rest", -1), seed & 0xFFFFFFFF, seed >> 32, tree.get("t", 0),
           tree.get("env_offset", 0), tree.get("simulations", 1), tree.get("explore", 0), tree.get("salt", 0), reuse]
    assert len(row) == R.MOST_ARGUMENTS
    return [float(v) for v in row]


def _pair(game, n, hip_lib, oracle_lib):
    """a device engine and a checker engine that hold the same batch; both are stepped"""
    _, states, rngs = _world(game, n, R.BATCH_FRAMES[game], hip_lib, oracle_lib)
    return clone(hip_lib, game, states, rngs), clone(oracle_lib, game, states, rngs)


def _store(g, simulations):
    raw = read_buffer(g, R.BUF_PLAN_TREE, (g.device_buffer(R.BUF_PLAN_TREE)[1],), np.uint8)
    return raw, tree_store_units(g.game, raw, g.n_envs, simulations)


def _assert_call(g, got, want, simulations, what):
    assert got.shape == want["out"].shape and np.array_equal(got, want["out"]), "%s: rows differ in envs %r" % (what, np.flatnonzero((got != want["out"]).any(axis=1))[:8])
    assert np.array_equal(read_buffer(g, R.BUF_PLAN_ACTION, (g.n_envs,), np.int32), want["action"]), "%s: TBX_BUF_PLAN_ACTION" % what
    _assert_units(_store(g, simulations)[1], want["units"], what)


def _assert_units(units, want, what):
    for i, (a, b) in enumerate(zip(units, want)):
        for k, (x, y) in enumerate(zip(a, b)):
            assert x == y, "%s: carried tree (env %d, action %d) differs: %d nodes against %d, first at node %r" % (
                what, i, k, len(x), len(y), next((j for j, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y))))


class _DeviceLoop:
    """k periods queued on one caller's stream with no host synchronisation between them"""

    def __init__(self, g, k, simulations):
        self.g, self.k, self.n, self.simulations = g, k, g.n_envs, simulations
        self.stream = hip.Stream()
        L = len(LEGAL[g.game])
        self.store_bytes = self.n * L * (64 + 32 * ((simulations + 2) & ~1))
        self.rows, self.action, self.store = hip.malloc(k * self.n * 112), hip.malloc(k * self.n * 4), hip.malloc(k * self.store_bytes)

    def run(self, tree, reuse, drops=None, done_drops=False):
        n, g, s = self.n, self.g, self.stream
        for p in range(self.k):
            if drops and p in drops:
                g.tree_drop(drops[p])                                     # (a host form: it waits, the only wait of the loop)
            g.reduce_device(R.QUERY, self.rows + p * n * 112, _args(dict(tree, t=tree["t"] + p), reuse), stream=s.ptr)
            pa, (pt, nbytes) = g.device_buffer(R.BUF_PLAN_ACTION)[0], g.device_buffer(R.BUF_PLAN_TREE)
            assert nbytes == self.store_bytes
            hip.memcpy_dtod_async(self.action + p * n * 4, pa, n * 4, s)
            hip.memcpy_dtod_async(self.store + p * nbytes, pt, nbytes, s)
            for _ in range(tree["hold"]):
                g.step_device(pa, auto_reset=True, stream=s.ptr)
                if done_drops:
                    g.tree_drop_device(g.device_buffer(_abi.BUF_DONE)[0], stream=s.ptr)
        s.synchronize()
        rows, action, store = np.empty((self.k, n, 14)), np.empty((self.k, n), np.int32), np.empty((self.k, self.store_bytes), np.uint8)
        for dst, src in ((rows, self.rows), (action, self.action), (store, self.store)):
            hip.memcpy_dtoh(dst, src, dst.nbytes)
        return rows, action, store

    def close(self):
        self.g.sync()
        for p in (self.rows, self.action, self.store):
            hip.free(p)
        self.stream.close()


def _loop(game, name, hip_lib, oracle_lib, form=0, drops=None, done_drops=False, options=()):
    kw = R.loop_tree(game, name)
    tree, reuse = kw["tree"], kw["reuse"]
    g, o = _pair(game, R.ENVS, hip_lib, oracle_lib)
    loop = _DeviceLoop(g, R.PERIODS, tree["simulations"])
    try:
        if form:
            g.set_option(_abi.OPT_STEP_FORM, form)
        g.set_option(R.OPT_KEEP, kw.get("keep", 0))
        g.set_option(R.OPT_MAX_VISITS, kw.get("max_visits", 0))
        for option, value in options:
            g.set_option(option, value)
        rows, action, store = loop.run(tree, reuse, drops, done_drops)
        replay_drops = dict(drops or {})
        if done_drops:
            replay_drops.update({p: "done" for p in range(1, R.PERIODS)})
        want, _ = R.expected_loop(oracle_lib, game, o, R.PERIODS, tree, reuse, kw.get("keep", 0), kw.get("max_visits", 0), drops=replay_drops)
        what = "%s %s" % (game, name)
        for p, w in enumerate(want):
            assert np.array_equal(rows[p], w["out"]), "%s period %d: rows differ in envs %r" % (what, p, np.flatnonzero((rows[p] != w["out"]).any(axis=1))[:8])
            assert np.array_equal(action[p], w["action"]), "%s period %d: TBX_BUF_PLAN_ACTION" % (what, p)
            _assert_units(tree_store_units(game, store[p], R.ENVS, tree["simulations"]), w["units"], "%s period %d" % (what, p))
            assert (rows[p][:, 2] == tree["simulations"]).all(), "samples = M in every row"
        assert bytes(g.get_states()) == bytes(o.get_states()), "%s: state records after the last period" % what
        return want, rows, action, store
    finally:
        loop.close()
        g.close()
        o.close()


# ---------------------------------------------------------------- 1. the loops equal the replay

@pytest.mark.parametrize("name", ["reuse", "reuse_explore", "drawn", "long", "few"])
@pytest.mark.parametrize("game", GAMES)
def test_loop_equals_replay(game, name, hip_lib, oracle_lib):
    want, _, _, _ = _loop(game, name, hip_lib, oracle_lib, drops={2: R.DROP_MASK} if name in ("reuse", "reuse_explore") else None)
    assert sum(w["stats"]["used"] for w in want) > 0
    if name in ("reuse", "reuse_explore"):
        assert want[2]["stats"]["flag_drops"] == int(R.DROP_MASK.sum()) and want[3]["stats"]["flag_drops"] == 0, "the host mask, and the flags are consumed"
    if name == "few":
        assert sum(w["stats"]["start_absent"] for w in want) > 0


def test_breakout_wave_form(hip_lib, oracle_lib):
    _loop("breakout", "reuse_explore", hip_lib, oracle_lib, form=_abi.STEP_FORM_WAVE_PER_ENV)


@pytest.mark.parametrize("name", ["keep1", "keep2", "keep5", "halve1", "halve_mid"])
@pytest.mark.parametrize("game", GAMES)
def test_forced_truncation_and_halving(game, name, hip_lib, oracle_lib):
    want, _, _, _ = _loop(game, name, hip_lib, oracle_lib)
    if name.startswith("keep") and 1 + len(LEGAL[game]) > int(name[4:]):
        assert all(w["stats"]["truncated"] > 0 for w in want)
    if name.startswith("halve"):
        assert want[2]["stats"]["halved"] > 0


@pytest.mark.parametrize("game", ["breakout", "amidar"])
def test_drop_through_the_done_buffer(game, hip_lib, oracle_lib):
    """TBX_EDIT_TREE_DROP in the device form behind every frame's step, its mask the engine's own done buffer: the trees of games
    that ended are dead in the next call.  The states are written ones: the batch's recipe sets lives = 1 in two envs of three
    (TBX_EDIT_SET_LIVES), so in Breakout and Amidar the first lost life ends a game in the loop's first period (asserted);
    SpaceInvaders loses no life in these 5 periods and GridWorld has no lives to write, so they are not cases here."""
    want, _, _, _ = _loop(game, "reuse_explore", hip_lib, oracle_lib, done_drops=True)
    assert sum(w["stats"]["flag_drops"] for w in want) > 0 and sum(int(w["done"].sum()) for w in want) > 0


# ---------------------------------------------------------------- 2. reuse = 0 is query 160 and the host pick

@pytest.mark.parametrize("game", GAMES)
def test_reuse_0_is_the_tree_query_and_the_host_pick(game, hip_lib, oracle_lib):
    want, rows, action, _ = _loop(game, "plain", hip_lib, oracle_lib)
    tree = R.loop_tree(game, "plain")["tree"]
    L = len(LEGAL[game])
    g, o = _pair(game, R.ENVS, hip_lib, oracle_lib)
    try:
        assert g.reduce_width(R.QUERY) == 14
        for p in range(R.PERIODS):
            own = g.reduce(_abi.QUERY_LOOKAHEAD_TREE, _args(dict(tree, t=tree["t"] + p), 0)[:12]).reshape(R.ENVS, L, 12)
            best = plan_pick(np.concatenate([own[..., :8], own[..., 8:9]], axis=2), tree["objective"] if "objective" in tree else 0, sampled=True)
            assert np.array_equal(rows[p][:, 1], best.astype(np.float64)) and np.array_equal(rows[p][:, 2:], own[np.arange(R.ENVS), best]), "period %d" % p
            assert np.array_equal(rows[p][:, 0], np.asarray(LEGAL[game], np.float64)[best])
            for _ in range(tree["hold"]):
                g.step(action[p], auto_reset=True)
    finally:
        g.close()
        o.close()


# ---------------------------------------------------------------- 3. ranges and launch cuts change no bit

@pytest.mark.parametrize("game", GAMES)
def test_ranges_and_launch_cuts_change_nothing(game, hip_lib, oracle_lib):
    ref = None
    for options in ((), ((_abi.OPT_BEAM_RANGE_ENVS, 1),), ((_abi.OPT_BEAM_RANGE_ENVS, 7),), ((_abi.OPT_TREE_LAUNCH_SIMULATIONS, 1),), ((_abi.OPT_TREE_LAUNCH_SIMULATIONS, 5),),
                    ((_abi.OPT_BEAM_RANGE_ENVS, 7), (_abi.OPT_TREE_LAUNCH_SIMULATIONS, 5))):
        g, o = _pair(game, R.ENVS, hip_lib, oracle_lib)
        o.close()
        try:
            for option, value in options:
                g.set_option(option, value)
            tree = R.loop_tree(game, "reuse_explore")["tree"]
            got = []
            for p in range(2):                                            # the second call starts from carried trees
                got.append(g.reduce(R.QUERY, _args(dict(tree, t=tree["t"] + p), 1)))
                got.append(_store(g, tree["simulations"])[0])
            if options and options[0][0] == _abi.OPT_BEAM_RANGE_ENVS:
                assert g.tree_ranges == -(-R.ENVS // options[0][1])
            if ref is None:
                ref = got
            for x, y in zip(got, ref):
                assert np.array_equal(x, y), (game, options)
        finally:
            g.close()


# ---------------------------------------------------------------- 4. the carry kernel's block edges

@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("game", GAMES)
def test_block_edges(game, n, hip_lib, oracle_lib):
    L, hold = len(LEGAL[game]), R.HOLD[game]
    tree = dict(frames=hold, hold=hold, depth=2, simulations=L + 2, explore=R.EXPLORE[game], rest=-1, seed=9, t=1)
    g, o = _pair(game, n, hip_lib, oracle_lib)
    try:
        st = R.TreeActReplay(game, n)
        for reuse in (0, 1):
            want = st.call(oracle_lib, o.get_states(), sim_rngs(o), tree, reuse)
            want["units"] = st.units()
            _assert_call(g, g.reduce(R.QUERY, _args(tree, reuse)), want, tree["simulations"], "%s n=%d reuse=%d" % (game, n, reuse))
    finally:
        g.close()
        o.close()


# ---------------------------------------------------------------- 5. the drop edit, the key, refusals

def _sequence(game, hip_lib, oracle_lib, calls):
    """calls: ("call", tree, reuse) / ("drop", mask or None) in order, on one batch that is never stepped; every call is compared"""
    g, o = _pair(game, R.ENVS, hip_lib, oracle_lib)
    try:
        st = R.TreeActReplay(game, R.ENVS)
        states, rngs = o.get_states(), sim_rngs(o)
        used = []
        for i, c in enumerate(calls):
            if c[0] == "drop":
                assert st.drop(c[1])
                g.tree_drop(c[1])
                continue
            want = st.call(oracle_lib, states, rngs, c[1], c[2])
            want["units"] = st.units()
            _assert_call(g, g.reduce(R.QUERY, _args(c[1], c[2])), want, c[1]["simulations"], "%s step %d" % (game, i))
            used.append(want["stats"]["used"])
        return used
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("game", GAMES)
def test_drop_edit_and_key(game, hip_lib, oracle_lib):
    tree = R.loop_tree(game, "reuse_explore")["tree"]
    L = len(LEGAL[game])
    mask = np.arange(R.ENVS) % 4 == 1
    used = _sequence(game, hip_lib, oracle_lib, [("call", tree, 1), ("call", tree, 1), ("drop", mask), ("call", tree, 1), ("drop", None), ("call", tree, 1), ("call", tree, 1),
                                                 ("call", dict(tree, depth=2), 1), ("call", tree, 1), ("call", tree, 1), ("call", dict(tree, simulations=4 * L), 1), ("call", tree, 1),
                                                 ("call", tree, 0), ("call", tree, 1)])
    units = R.ENVS * L
    assert used == [0, units, units - int(mask.sum()) * L, 0, units, 0, 0, units, 0, 0, 0, units], used


def test_the_edit_before_the_first_call_is_refused(hip_lib, oracle_lib):
    g, o = _pair("gridworld", 5, hip_lib, oracle_lib)
    o.close()
    try:
        for call in (lambda: g.tree_drop(), lambda: g.tree_drop(np.ones(5, bool)), lambda: g.device_buffer(R.BUF_PLAN_TREE), lambda: g.edit_device(R.EDIT_DROP, ()), lambda: g.tree_drop_device()):
            with pytest.raises(ToyboxAmdError) as ei:
                call()
            assert ei.value.code == _abi.E_INVALID
        g.lookahead_tree_act(4, 2, 3)
        g.tree_drop()
        g.tree_drop_device()                                          # (mask NULL on the default stream: the device form, every env)
        g.sync()
        with pytest.raises(ToyboxAmdError) as ei:
            g.edit(R.EDIT_DROP, [1.0])
        assert ei.value.code == _abi.E_INVALID
    finally:
        g.close()


def test_refused_calls_change_nothing(hip_lib, oracle_lib):
    """per_env, 14 arguments, reuse = 2 and every value that query 160 refuses: the engine, both buffers and the store stay byte
    for byte; the flags are not readable, so a drop set BEFORE the refusals must still hold in the call after them"""
    game = "space_invaders"
    tree = R.loop_tree(game, "reuse_explore")["tree"]
    g, o = _pair(game, R.ENVS, hip_lib, oracle_lib)
    try:
        st = R.TreeActReplay(game, R.ENVS)
        states, rngs = o.get_states(), sim_rngs(o)
        st.call(oracle_lib, states, rngs, tree, 1)
        g.reduce(R.QUERY, _args(tree, 1))
        mask = np.arange(R.ENVS) % 5 == 2
        st.drop(mask)
        g.tree_drop(mask)
        before = (_snapshot(g), read_buffer(g, R.BUF_PLAN_ACTION, (R.ENVS,), np.int32), read_buffer(g, _abi.BUF_PLAN_CARRY, (R.ENVS,), np.uint32), _store(g, tree["simulations"])[0])
        good = _args(tree, 1)
        bad_rows = [good + [0.0], good[:12] + [2.0], good[:12] + [-1.0], good[:12] + [0.5]]
        for col, values in ((0, (0, 1025)), (1, (0,)), (2, (0, 13)), (3, (2, -1)), (4, (2, 7)), (9, (0, 1025)), (10, (-1, 2 ** 20 + 1)), (11, (-1, 2 ** 32, 2 ** 32 - 3))):
            for v in values:
                bad_rows.append(good[:col] + [float(v)] + good[col + 1:])
        for row in bad_rows:
            with pytest.raises(ToyboxAmdError) as ei:
                g.reduce(R.QUERY, row)
            assert ei.value.code == _abi.E_INVALID, row
        with pytest.raises(ToyboxAmdError) as ei:
            g.reduce(R.QUERY, np.tile(np.asarray(good), (R.ENVS, 1)))
        assert ei.value.code == _abi.E_INVALID, "per-env rows"
        with pytest.raises(ToyboxAmdError) as ei:
            g.reduce(R.QUERY, [])
        assert ei.value.code == _abi.E_INVALID
        after = (_snapshot(g), read_buffer(g, R.BUF_PLAN_ACTION, (R.ENVS,), np.int32), read_buffer(g, _abi.BUF_PLAN_CARRY, (R.ENVS,), np.uint32), _store(g, tree["simulations"])[0])
        _assert_same_snapshot(before[0], after[0], "refused calls")
        assert all(np.array_equal(x, y) for x, y in zip(before[1:], after[1:])), "a buffer or the store changed"
        want = st.call(oracle_lib, states, rngs, tree, 1)
        want["units"] = st.units()
        assert want["stats"]["flag_drops"] == int(mask.sum())
        _assert_call(g, g.reduce(R.QUERY, _args(tree, 1)), want, tree["simulations"], "the call after the refusals")
        _assert_same_snapshot(before[0], _snapshot(g), "nothing in the engine changes")
    finally:
        g.close()
        o.close()


def test_the_keyword_forms_ask_the_same(hip_lib, oracle_lib):
    game = "amidar"
    tree = R.loop_tree(game, "drawn")["tree"]
    g, o = _pair(game, R.ENVS, hip_lib, oracle_lib)
    try:
        st = R.TreeActReplay(game, R.ENVS)
        kw = dict(tree, rest=None, objective=("return", "survival")[tree["objective"]])
        for reuse in (False, True):
            want = st.call(oracle_lib, o.get_states(), sim_rngs(o), tree, int(reuse))
            got = g.lookahead_tree_act(reuse=reuse, **kw)
            assert np.array_equal(got["action"], want["action"]) and np.array_equal(got["action_index"], want["best"])
            for c, k in enumerate(TREE_FIELDS):
                assert np.array_equal(got[k].astype(np.int64), want["out"][:, 2 + c].astype(np.int64)), k
            assert g.plan_trees(tree["simulations"]) == st.units()
            assert g.plan_action_ptr == g.device_buffer(R.BUF_PLAN_ACTION)[0]
    finally:
        g.close()
        o.close()


# ---------------------------------------------------------------- 6. the adapters

def test_plan_rollout_tree_is_the_replay_and_drops_the_trees_of_ended_games(hip_lib, oracle_lib):
    """ToyboxVecEnv.plan_rollout(3, "tree") against the replay's loop with the done flags of every frame as drop masks: Breakout
    with one life left in most envs, so games end inside the window and the next step's trees of those envs start empty"""
    from toybox_amd.envs.vec_env import ToyboxVecEnv
    game, n, k, hold = "breakout", R.ENVS, 3, 8               # (chosen on the checker: 9 games end in the second step of the window)
    v = ToyboxVecEnv(game, n, seed=11, cache_terminal_state=False)
    try:
        v.reset()
        for t in range(68):
            v.step(np.full(n, t % 4))
        v.engine.edit(_abi.EDIT_SET_LIVES, [1])
        o = clone(oracle_lib, game, v.engine.get_states(), sim_rngs(v.engine))
        L = len(LEGAL[game])
        tree = dict(frames=3 * hold, hold=hold, depth=3, objective=0, rest=-1, seed=7, t=2, simulations=6 * L, explore=R.EXPLORE[game], salt=0)
        want, st = R.expected_loop(oracle_lib, game, o, k, tree, 1, drops={p: "done" for p in range(1, k)})
        obs, reward, done, _ = v.plan_rollout(k, "tree", steps=3, depth=3, hold=hold, seed=7, t=2, simulations=6 * L, explore=R.EXPLORE[game], reuse=True)
        assert np.array_equal(v.plan_actions(), np.stack([w["best"] for w in want])) and reward.shape == (k, n)
        assert np.array_equal(done, np.stack([w["done"] for w in want]))
        assert want[2]["stats"]["flag_drops"] == int(done[1].sum()) > 0, "games ended inside the window, and their trees started empty in the step after"
        assert v.engine.plan_trees(6 * L) == st.units()
        assert bytes(v.engine.get_states()) == bytes(o.get_states())
        o.close()
        with pytest.raises(TypeError):
            v.plan_rollout(1, "tree", steps=3, depth=3, width=2)
    finally:
        v.close()


def test_preproc_plan_rollout_tree_is_the_replay_and_plan_steps(hip_lib, oracle_lib):
    """ToyboxPreprocVecEnv.plan_rollout(3, "tree") against the replay's actions -- the replay searches on the records of a checker
    twin of the env, steps it with the checker's own agent step and drops by its episode-end flags -- and = k plan_step calls on a
    twin, and the same actions as the engine's own lookahead_tree_act with hold = skip.  No game of this batch ends inside the
    window: the drop edit on the agent path is queued and consumed, its effect is shown on the raw path above."""
    from toybox_amd import Engine
    from toybox_amd.envs.vec_env import ToyboxPreprocVecEnv
    n, k = 17, 3
    kw = dict(planner="tree", steps=3, depth=3, simulations=14, explore=64, t=2)
    a, b, c = (ToyboxPreprocVecEnv("space_invaders", n, seed=5) for _ in range(3))
    o = ToyboxPreprocVecEnv("space_invaders", n, seed=5, engine=Engine("space_invaders", n, lib=oracle_lib))
    try:
        for e in (a, b, c, o):
            e.reset()
            for t in range(10):
                e.step(np.full(n, t % 6))
        assert bytes(a.engine.get_states()) == bytes(o.engine.get_states())

        def agent_step(e, action):
            e.agent_step(action, tolerate_needs_reset=True)
            return read_buffer(e, _abi.BUF_AGENT_EP_DONE, (n,), np.uint8)
        tree = dict(frames=12, hold=4, depth=3, objective=0, rest=-1, seed=0, t=2, simulations=14, explore=64, salt=0)
        want, _ = R.expected_loop(oracle_lib, "space_invaders", o.engine, k, tree, 1, drops={p: "done" for p in range(1, k)}, step=agent_step)
        obs, reward, done, _ = a.plan_rollout(k, **kw)
        assert np.array_equal(a.plan_actions(), np.stack([w["best"] for w in want])), "the replay's actions"
        assert bytes(a.engine.get_states()) == bytes(o.engine.get_states())
        for i in range(k):
            o2, r2, d2, _ = b.plan_step(**dict(kw, t=kw["t"] + i))
            assert np.array_equal(b.plan_actions()[0], a.plan_actions()[i]) and np.array_equal(r2, reward[i]) and np.array_equal(d2, done[i]), i
            got = c.engine.lookahead_tree_act(3 * 4, 3, 14, explore=64, reuse=True, hold=4, t=kw["t"] + i)
            assert np.array_equal(got["action_index"], a.plan_actions()[i]), i
            c.engine.agent_step(got["action"].astype(np.int32), tolerate_needs_reset=True)
            c.engine.tree_drop(read_buffer(c.engine, _abi.BUF_AGENT_EP_DONE, (n,), np.uint8).astype(bool))
        assert np.array_equal(np.asarray(o2), np.asarray(obs)) and bytes(a.engine.get_states()) == bytes(b.engine.get_states()) == bytes(c.engine.get_states())
    finally:
        for e in (a, b, c, o):
            e.close()
