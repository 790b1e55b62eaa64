"""Closed-loop planning on the device (TBX_QUERY_LOOKAHEAD_ACT, include/toybox_amd.h) against PLAN ON A CLONE, PICK, STEP, SHIFT,
CARRY on the CPU checker (tests/act_replay.py; its own checks are in tests/test_act.py).  Every comparison is exact.

Rows: per game and planner one call from a batch behind 400 frames of synthetic play (GridWorld 40) at 1, 65 and 257 envs -- the
smaller batches are the first envs of the largest, so one replay serves the three; shapes in act_replay.row_case (frames 32, hold 4;
depth 2 for the searches, 6 at width 3 for the beam, 4 at width 2 with 2 samples for the sampled beam, 8 with P 8 / G 2 / E 2 for
the evolution, which is asked a second time from the carry the first call left).
Ties: 65 copies of env 0 of the 65-env batch under rest = the first legal action, depth 1, 8 frames: on the checker ALL 65 envs tie on
every key between two or more first actions, in every game, for both pick orders and both objectives (asserted below).
Closed loop: 6 periods of 65 envs, raw form hold 8 and agent form hold = skip = 4.  Measured on the checker for the raw form,
158 / 156: envs whose lives changed across a period 27 / 27 (Breakout), 4 / 4 (SpaceInvaders), 2 / 2 (Amidar), and 0 in GridWorld,
which has no lives to lose -- the condition is asserted for the three games that have; envs whose winner changed its first action
between consecutive periods 17 / 17, 45 / 44, 26 / 27, 54 / 63.  Agent form (250 agent steps of synthetic play behind it, frames 32):
lives changed 1 / 1, 3 / 3, 1 / 1, 0 / 0; first action changed 11 / 12, 45 / 44, 26 / 27, 34 / 33.  The 1 027-env Breakout loop in three
env ranges: 456 and 168 envs.  The module took 55 s on an MI355X box with 16 host threads, nearly all of it the checker's replays;
the longest case is that 1 027-env loop at 22 s (its six replayed evolutions), every other case under 3 s."""
import functools

import numpy as np
import pytest

from act_replay import (ACT, BEAM, BEAM_SAMPLES, BUF_PLAN_ACTION, BUF_PLAN_CARRY, EVOLVE, LOOP_ENVS, LOOP_FRAMES, LOOP_PERIODS, MOST_COLUMNS, PLANNERS, ROW_ENVS, SAMPLED,
                        SEARCH, SEARCH_SAMPLES, all_keys_tied, expected_act, expected_rollout, loop_case, loop_stats, row_case)
from fork_replay import Agent, sim_rngs
from lookahead_replay import clone
from support import LEGAL, read_buffer
from test_gpu_search import _assert_same_snapshot, _snapshot, _world
from toybox_amd import ToyboxAmdError, _abi, hip

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
NAMES = {SEARCH: "search", SEARCH_SAMPLES: "search_samples", BEAM: "beam", BEAM_SAMPLES: "beam_samples", EVOLVE: "evolve"}
WORLD_FRAMES = {"breakout": 400, "space_invaders": 400, "amidar": 400, "gridworld": 40}


def _args(planner, case):
    """the shared row {planner, the planner's columns} of a replay case, every column written out"""
    seed = int(case.get("seed", 0))
    row = [planner, case["frames"], case.get("hold", 1), case.get("depth", 1), case.get("objective", 0), case.get("rest", -1), seed & 0xFFFFFFFF, seed >> 32,
           case.get("t", 0), case.get("env_offset", 0)]
    if planner in (BEAM, BEAM_SAMPLES):
        row.append(case.get("width", 1))
    if planner in SAMPLED:
        row += [case.get("samples", 1), case.get("salt", 0)]
    if planner == EVOLVE:
        row += [case.get("population", 1), case.get("generations", 0), case.get("elite", 1), case.get("plan_seed", 0), case.get("mutation", 64), case.get("init", -1)]
    assert len(row) == 1 + MOST_COLUMNS[planner]
    return [float(v) for v in row]


def _buffers(g):
    return read_buffer(g, BUF_PLAN_ACTION, (g.n_envs,), np.int32), read_buffer(g, BUF_PLAN_CARRY, (g.n_envs,), np.uint32)


def _ask_device(g, args, stream):
    """tbx_reduce_device on a caller's stream -> rows [n, 11]"""
    out = hip.malloc(g.n_envs * 11 * 8)
    try:
        g.reduce_device(ACT, out, args, stream=stream.ptr)
        stream.synchronize()
        rows = np.empty((g.n_envs, 11), np.float64)
        hip.memcpy_dtoh(rows, out, rows.nbytes)
    finally:
        g.sync()
        hip.free(out)
    return rows


def _assert_act(got, buffers, want, what):
    out, action, carry = want[:3]
    assert got.shape == out.shape and np.array_equal(got, out), "%s: rows differ in envs %r" % (what, np.flatnonzero((got != out).any(axis=1))[:8])
    assert np.array_equal(buffers[0], action), "%s: TBX_BUF_PLAN_ACTION" % what
    assert np.array_equal(buffers[1], carry), "%s: TBX_BUF_PLAN_CARRY" % what


@functools.lru_cache(maxsize=None)
def _sub_world(game, n, hip_lib, oracle_lib):
    """a device engine that holds the first n envs of the largest rows batch; queried only"""
    g, states, rngs = _world(game, ROW_ENVS[-1], WORLD_FRAMES[game], hip_lib, oracle_lib)
    if n == ROW_ENVS[-1]:
        return g
    part = (states._type_ * n).from_buffer_copy(bytes(states)[:n * len(bytes(states)) // len(states)])
    return clone(hip_lib, game, part, rngs[:n])


@functools.lru_cache(maxsize=None)
def _row_replay(game, planner, hip_lib, oracle_lib):
    """the expected call(s) of the rows test at the largest batch, made once: [(case, (out, action, carry, rows)), ...]"""
    _, states, rngs = _world(game, ROW_ENVS[-1], WORLD_FRAMES[game], hip_lib, oracle_lib)
    case = row_case(game, planner)
    calls = [(case, expected_act(oracle_lib, game, states, rngs, planner, case))]
    if planner == EVOLVE:                                                 # ... and again, seeded with what the first call carried
        again = dict(case, init=-2, objective=1, plan_seed=5)
        calls.append((again, expected_act(oracle_lib, game, states, rngs, planner, again, carry=calls[0][1][2])))
    return calls


# ---------------------------------------------------------------- 1. rows, action and carry equal the replay

@pytest.mark.parametrize("n", ROW_ENVS)
@pytest.mark.parametrize("planner", PLANNERS, ids=[NAMES[p] for p in PLANNERS])
@pytest.mark.parametrize("game", GAMES)
def test_act_equals_replay(game, planner, n, hip_lib, oracle_lib):
    g = _sub_world(game, n, hip_lib, oracle_lib)
    assert g.reduce_width(ACT) == 11
    stream = hip.Stream()
    try:
        for case, want in _row_replay(game, planner, hip_lib, oracle_lib):
            want = tuple(w[:n] for w in want[:3])
            args = _args(planner, case)
            got = g.reduce(ACT, args)
            _assert_act(got, _buffers(g), want, "%s %s n=%d tbx_reduce" % (game, NAMES[planner], n))
            if case.get("init") == -2:                               # the device form starts from the same carry
                g.reduce(ACT, _args(planner, _row_replay(game, planner, hip_lib, oracle_lib)[0][0]))
            again = _ask_device(g, args, stream)
            _assert_act(again, _buffers(g), want, "%s %s n=%d tbx_reduce_device" % (game, NAMES[planner], n))
            L = len(LEGAL[game])
            code = got[:, 10 if planner in SAMPLED else 7].astype(np.uint64)
            assert np.array_equal(code % np.uint64(L), got[:, 1].astype(np.uint64)) and np.array_equal(got[:, 0], np.asarray(LEGAL[game])[got[:, 1].astype(int)])
            if planner not in SAMPLED:
                assert (got[:, 8:] == 0).all(), "a row of 6 is zero-padded to 9"
    finally:
        stream.close()


def test_the_keyword_forms_ask_the_same(hip_lib, oracle_lib):
    """Engine.lookahead_act / lookahead_act_device with the product's act_args: the dict names the row's columns"""
    game, n = "space_invaders", 65
    g = _sub_world(game, n, hip_lib, oracle_lib)
    for planner in PLANNERS:
        case = row_case(game, planner)
        kw = dict(case, rest=None if case["rest"] == -1 else case["rest"], objective=("return", "survival")[case["objective"]])
        out, action, carry, rows = (w[:n] if not isinstance(w, dict) else w for w in _row_replay(game, planner, hip_lib, oracle_lib)[0][1])
        got = g.lookahead_act(NAMES[planner], **kw)
        assert np.array_equal(got["action"], action) and np.array_equal(got["action_index"], out[:, 1].astype(np.int64))
        assert np.array_equal(got["plan"][:, 0], got["action_index"]) and got["plan"].shape == (n, case["depth"])
        for k in ("ret", "lives") if planner not in SAMPLED else ("ret_sum", "lost"):
            assert np.array_equal(got[k], rows[k][np.arange(n), got["action_index"]][:n]), k
        host_action, host_carry = g.plan_buffers()
        assert np.array_equal(host_action, action) and np.array_equal(host_carry, carry)


# ---------------------------------------------------------------- 2. ties go to the smaller code / the smaller index

@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("planner", [SEARCH, SEARCH_SAMPLES], ids=["search-order", "sampled-order"])
@pytest.mark.parametrize("game", GAMES)
def test_ties_are_the_replays(game, planner, objective, hip_lib, oracle_lib):
    n = LOOP_ENVS
    _, states, rngs = _world(game, n, LOOP_FRAMES[game], hip_lib, oracle_lib)
    g = clone(hip_lib, game, states, rngs)
    try:
        g.fork(np.zeros(n, np.int64))
        copies, copied_rngs = g.get_states(), sim_rngs(g)
        assert bytes(copies) == bytes(states)[:len(bytes(states)) // n] * n
        case = dict(frames=8, hold=4, depth=1, objective=objective, rest=LEGAL[game][0])
        if planner == SEARCH_SAMPLES:
            case.update(samples=2, salt=0)
        want = expected_act(oracle_lib, game, copies, copied_rngs, planner, case)
        tied = all_keys_tied(want[3], planner, objective)
        assert tied.sum() * 4 >= n, "%s: only %d of %d envs tie on every key" % (game, tied.sum(), n)
        got = g.reduce(ACT, _args(planner, case))
        _assert_act(got, _buffers(g), want, "%s ties" % game)
    finally:
        g.close()


# ---------------------------------------------------------------- 3. the closed loop

class _DeviceLoop:
    """k periods queued on one caller's stream with no host synchronisation between them: the query, the step(s) reading
    TBX_BUF_PLAN_ACTION, and copies of the rows, the action and the carry of the period queued behind them on the same stream"""

    def __init__(self, g, k):
        self.g, self.k, self.n = g, k, g.n_envs
        self.stream = hip.Stream()
        self.rows, self.action, self.carry = hip.malloc(k * self.n * 88), hip.malloc(k * self.n * 4), hip.malloc(k * self.n * 4)

    def run(self, planner, case, step):
        n = self.n
        for p in range(self.k):
            self.g.reduce_device(ACT, self.rows + p * n * 88, _args(planner, dict(case, t=case["t"] + p)), stream=self.stream.ptr)
            if p == 0:                                                    # (the engine's first call has made the two buffers: host calls, no wait)
                self.pa, self.pc = self.g.device_buffer(BUF_PLAN_ACTION)[0], self.g.device_buffer(BUF_PLAN_CARRY)[0]
            hip.memcpy_dtod_async(self.action + p * n * 4, self.pa, n * 4, self.stream)
            hip.memcpy_dtod_async(self.carry + p * n * 4, self.pc, n * 4, self.stream)
            step(self.g, self.pa, self.stream.ptr)
        self.stream.synchronize()
        rows, action, carry = np.empty((self.k, n, 11)), np.empty((self.k, n), np.int32), np.empty((self.k, n), np.uint32)
        for dst, src in ((rows, self.rows), (action, self.action), (carry, self.carry)):
            hip.memcpy_dtoh(dst, src, dst.nbytes)
        return rows, action, carry

    def close(self):
        self.g.sync()
        for p in (self.rows, self.action, self.carry):
            hip.free(p)
        self.stream.close()


def _assert_loop(got, periods, what):
    rows, action, carry = got
    for p, want in enumerate(periods):
        assert np.array_equal(action[p], want["action"]), "%s period %d: actions differ in envs %r" % (what, p, np.flatnonzero(action[p] != want["action"])[:8])
        assert np.array_equal(carry[p], want["carry"]), "%s period %d: carry" % (what, p)
        assert np.array_equal(rows[p], want["out"]), "%s period %d: rows" % (what, p)


def _raw_steps(hold):
    def step(g, actions, stream):
        for _ in range(hold):
            g.step_device(actions, auto_reset=True, stream=stream)
    return step


def _raw_loop(game, planner, n, frames, hip_lib, oracle_lib, range_envs=0):
    _, states, rngs = _world(game, n, frames, hip_lib, oracle_lib)
    g, o = clone(hip_lib, game, states, rngs), clone(oracle_lib, game, states, rngs)
    loop = _DeviceLoop(g, LOOP_PERIODS)
    try:
        case = loop_case(game, planner)
        if range_envs:
            g.beam_range_envs = range_envs
        got = loop.run(planner, case, _raw_steps(case["hold"]))
        ranges = g.evolve_ranges if planner == EVOLVE else g.beam_ranges
        periods = expected_rollout(oracle_lib, game, o, planner, LOOP_PERIODS, case)
        what = "%s %s raw loop n=%d" % (game, NAMES[planner], n)
        _assert_loop(got, periods, what)
        assert bytes(g.get_states()) == bytes(o.get_states()), "%s: state records (the game RNGs in them) after the last period" % what
        assert np.array_equal(sim_rngs(g), sim_rngs(o)), "%s: simulator RNGs" % what
        return loop_stats(periods, o.scalars()[1]), ranges
    finally:
        loop.close()
        g.close()
        o.close()


@pytest.mark.parametrize("planner", [EVOLVE, BEAM], ids=["evolve-from-carry", "beam"])
@pytest.mark.parametrize("game", GAMES)
def test_closed_loop_raw_form(game, planner, hip_lib, oracle_lib):
    (lost, changed), ranges = _raw_loop(game, planner, LOOP_ENVS, LOOP_FRAMES[game], hip_lib, oracle_lib)
    assert ranges == 1 and changed >= 1, "no env's winner ever changed its first action"
    if game != "gridworld":                                               # (GridWorld has no lives)
        assert lost >= 1, "no env lost a life in the loop"


def test_closed_loop_breakout_in_env_ranges(hip_lib, oracle_lib):
    """1 027 envs cut into three env ranges (TBX_OPT_BEAM_RANGE_ENVS = 400): the per-env rows of the carry meet every range"""
    (lost, changed), ranges = _raw_loop("breakout", EVOLVE, 1027, 400, hip_lib, oracle_lib, range_envs=400)
    assert ranges == 3 and lost >= 1 and changed >= 1


@pytest.mark.parametrize("planner", [EVOLVE, BEAM], ids=["evolve-from-carry", "beam"])
@pytest.mark.parametrize("game", GAMES)
def test_closed_loop_agent_form(game, planner, hip_lib, oracle_lib):
    """tbx_agent_step_device reads the picked actions; hold = skip = 4.  The checker's loop is its own tbx_agent_step."""
    n, warm = LOOP_ENVS, 250
    agent = Agent(game, n)
    g, o = agent.make(hip_lib), agent.make(oracle_lib)
    loop = _DeviceLoop(g, LOOP_PERIODS)
    try:
        for t in range(warm):
            a = agent.actions(t)
            g.agent_step(a, tolerate_needs_reset=True)
            o.agent_step(a, tolerate_needs_reset=True)
        assert bytes(g.get_states()) == bytes(o.get_states())
        case = dict(loop_case(game, planner, hold=4), frames=32)
        got = loop.run(planner, case, lambda e, actions, stream: e.agent_step_device(actions, stream=stream))
        periods = expected_rollout(oracle_lib, game, o, planner, LOOP_PERIODS, case, step=lambda e, a: e.agent_step(a, tolerate_needs_reset=True))
        what = "%s %s agent loop" % (game, NAMES[planner])
        _assert_loop(got, periods, what)
        assert bytes(g.get_states()) == bytes(o.get_states()), "%s: state records after the last period" % what
        assert np.array_equal(sim_rngs(g), sim_rngs(o)), "%s: simulator RNGs" % what
        assert np.array_equal(agent.observation(g), agent.observation(o)), "%s: observations" % what
        for buf, dt in ((_abi.BUF_AGENT_REWARD, np.float32), (_abi.BUF_AGENT_DONE, np.uint8)):
            assert np.array_equal(read_buffer(g, buf, (n,), dt), read_buffer(o, buf, (n,), dt)), what
        lost, changed = loop_stats(periods, o.scalars()[1])
        assert changed >= 1 and (lost >= 1 or game == "gridworld"), "%s: %d envs lost a life, %d changed their first action" % (what, lost, changed)
    finally:
        loop.close()
        g.close()
        o.close()


# ---------------------------------------------------------------- 4. the carry

def test_carry_semantics(hip_lib, oracle_lib):
    game, n = "breakout", LOOP_ENVS
    L = len(LEGAL[game])
    _, states, rngs = _world(game, n, LOOP_FRAMES[game], hip_lib, oracle_lib)
    g = clone(hip_lib, game, states, rngs)
    try:
        for which in (BUF_PLAN_ACTION, BUF_PLAN_CARRY):                   # like the rollout ids before the first chunk
            with pytest.raises(ToyboxAmdError) as ei:
                g.device_buffer(which)
            assert ei.value.code == _abi.E_INVALID
        with pytest.raises(ToyboxAmdError):
            g.reduce(ACT, [0.0, 8.0])                                     # (no planner: nothing is made)
        with pytest.raises(ToyboxAmdError):
            g.device_buffer(BUF_PLAN_CARRY)
        deep = dict(frames=64, hold=4, depth=16, objective=0, rest=0, population=8, generations=1, elite=2, mutation=128, plan_seed=9, init=-2)
        first = expected_act(oracle_lib, game, states, rngs, EVOLVE, deep)
        _assert_act(g.reduce(ACT, _args(EVOLVE, deep)), _buffers(g), first, "the carry is zero before the first call: it plays from the all-first-action plan")
        assert int(first[2].max()) >= L ** 12, "carries of a deep plan"
        kept = _buffers(g)
        # unchanged by a refused call, by a plain 158, by fork, checkpoint restore and new_game
        with pytest.raises(ToyboxAmdError):
            g.reduce(ACT, _args(EVOLVE, dict(deep, depth=17)))
        plain = dict(deep, init=-1)
        g.reduce(_abi.QUERY_LOOKAHEAD_EVOLVE, _args(EVOLVE, plain)[1:])
        with pytest.raises(ToyboxAmdError) as ei:
            g.reduce(_abi.QUERY_LOOKAHEAD_EVOLVE, _args(EVOLVE, deep)[1:])
        assert ei.value.code == _abi.E_INVALID, "the plain query keeps refusing init = -2"
        g.checkpoint_slots(1)
        g.checkpoint_save(0)
        g.fork(np.roll(np.arange(n), 1))
        g.new_game(np.ones(n, np.uint8))
        g.checkpoint_restore(0)
        for a, b in zip(kept, _buffers(g)):
            assert np.array_equal(a, b), "the buffers are not env state"
        assert bytes(g.get_states()) == bytes(states)
        # a shallower call is seeded with carry % L ** depth
        shallow = dict(deep, depth=5, frames=20)
        second = expected_act(oracle_lib, game, states, rngs, EVOLVE, shallow, carry=first[2])
        _assert_act(g.reduce(ACT, _args(EVOLVE, shallow)), _buffers(g), second, "depth 16 -> 5")
        assert (first[2].astype(np.int64) >= L ** 5).any(), "a carry that the modulus cuts"
        # (ii): not worse than the carried plan itself, whatever G is
        unseeded = dict(shallow, init=-1)
        left = expected_act(oracle_lib, game, states, rngs, EVOLVE, unseeded)
        seeded = expected_act(oracle_lib, game, states, rngs, EVOLVE, dict(shallow, population=1, generations=0), carry=left[2])
        for G in (0, 2):
            _assert_act(g.reduce(ACT, _args(EVOLVE, unseeded)), _buffers(g), left, "a call without an init leaves its own carry")
            got = g.reduce(ACT, _args(EVOLVE, dict(shallow, generations=G)))
            assert (got[:, 2] >= seeded[0][:, 2]).all(), "return objective: ret not below the carried plan's best first action"
    finally:
        g.close()


# ---------------------------------------------------------------- 5. nothing else in the engine is written

@pytest.mark.parametrize("game", GAMES)
def test_the_engine_is_untouched(game, hip_lib, oracle_lib):
    g, _, _ = _world(game, LOOP_ENVS, LOOP_FRAMES[game], hip_lib, oracle_lib)
    before = _snapshot(g)
    for planner in PLANNERS:
        g.reduce(ACT, _args(planner, row_case(game, planner)))
    g.reduce(ACT, _args(EVOLVE, dict(row_case(game, EVOLVE), init=-2)))
    _assert_same_snapshot(before, _snapshot(g), "%s after six act calls" % game)
    # (iii): equal arguments, no step between: equal rows and actions
    args = _args(BEAM, row_case(game, BEAM))
    one, a1 = g.reduce(ACT, args), _buffers(g)
    two, a2 = g.reduce(ACT, args), _buffers(g)
    assert np.array_equal(one, two) and all(np.array_equal(x, y) for x, y in zip(a1, a2))
    # (iv): env ranges change no bit
    g.beam_range_envs = 7
    try:
        cut = g.reduce(ACT, args)
        assert g.beam_ranges == 10 and np.array_equal(cut, one)
    finally:
        g.beam_range_envs = 0


def test_the_agent_layer_is_untouched(hip_lib, oracle_lib):
    game, n = "breakout", 33
    agent = Agent(game, n)
    g = agent.make(hip_lib)
    try:
        for t in range(20):
            g.agent_step(agent.actions(t), tolerate_needs_reset=True)
        obs, snap = agent.observation(g), _snapshot(g)
        agent_out = [read_buffer(g, b, (n,), dt) for b, dt in ((_abi.BUF_AGENT_REWARD, np.float32), (_abi.BUF_AGENT_DONE, np.uint8), (_abi.BUF_AGENT_EP_LENGTH, np.int32))]
        for planner in (EVOLVE, BEAM_SAMPLES):
            g.reduce(ACT, _args(planner, row_case(game, planner)))
        _assert_same_snapshot(snap, _snapshot(g), "agent layer on")
        assert np.array_equal(obs, agent.observation(g)), "the observation buffer"
        for a, (b, dt) in zip(agent_out, ((_abi.BUF_AGENT_REWARD, np.float32), (_abi.BUF_AGENT_DONE, np.uint8), (_abi.BUF_AGENT_EP_LENGTH, np.int32))):
            assert np.array_equal(a, read_buffer(g, b, (n,), dt))
    finally:
        g.close()


# ---------------------------------------------------------------- 6. refusals

BAD_COLUMNS = {SEARCH: [dict(frames=0), dict(frames=1025), dict(hold=0), dict(depth=0), dict(depth=7), dict(objective=2), dict(rest=2)],
               SEARCH_SAMPLES: [dict(frames=0), dict(hold=0), dict(depth=7), dict(objective=-1), dict(rest=5), dict(samples=0), dict(samples=4097), dict(salt=-1),
                                dict(salt=2 ** 32)],
               BEAM: [dict(frames=0), dict(hold=0), dict(depth=17), dict(objective=2), dict(rest=2), dict(width=0), dict(width=65)],
               BEAM_SAMPLES: [dict(frames=0), dict(hold=0), dict(depth=17), dict(objective=2), dict(rest=2), dict(width=0), dict(samples=0), dict(salt=2 ** 32),
                              dict(depth=16, width=64, samples=4096)],
               EVOLVE: [dict(frames=0), dict(hold=0), dict(depth=17), dict(objective=2), dict(rest=2), dict(population=0), dict(population=257), dict(generations=-1),
                        dict(generations=65), dict(elite=0), dict(elite=9), dict(plan_seed=-1), dict(plan_seed=2 ** 32), dict(mutation=-1), dict(mutation=257),
                        dict(init=-3), dict(init=4 ** 8), dict(init=-2, depth=17), dict(init=-2, population=0)]}


def test_refusals_launch_nothing(hip_lib, oracle_lib):
    game, n = "breakout", LOOP_ENVS
    g, _, _ = _world(game, n, LOOP_FRAMES[game], hip_lib, oracle_lib)
    good = _args(BEAM, row_case(game, BEAM))
    rows = g.reduce(ACT, good)
    kept, snap = _buffers(g), _snapshot(g)
    out = hip.malloc(n * 88)
    marker = np.full((n, 11), -7.0)
    hip.memcpy_htod(out, marker, marker.nbytes)

    def refused(args, per_env=0):
        with pytest.raises(ToyboxAmdError) as ei:
            if per_env:
                g.reduce(ACT, np.tile(np.asarray(args, np.float64), (n, 1)))
            else:
                g.reduce(ACT, args)
        assert ei.value.code == _abi.E_INVALID, args
        with pytest.raises(ToyboxAmdError) as ei:
            if per_env:
                per = np.tile(np.asarray(args, np.float64), (n, 1))
                dev = hip.malloc(per.nbytes)
                try:
                    hip.memcpy_htod(dev, per, per.nbytes)
                    g.reduce_device(ACT, out, per_env_ptr=dev, n_args=per.shape[1])
                finally:
                    g.sync()
                    hip.free(dev)
            else:
                g.reduce_device(ACT, out, args)
        assert ei.value.code == _abi.E_INVALID, args

    try:
        refused(good, per_env=1)
        for planner in (150, 151, 152, 154, 159, 0, -1, 153.5):
            refused([planner] + good[1:])
        refused([float(BEAM)])
        for planner, bad in BAD_COLUMNS.items():
            for change in bad:
                refused(_args(planner, dict(row_case(game, planner), **change)))
            refused(_args(planner, row_case(game, planner)) + [0.0])             # one column more than the planner takes
        refused(_args(EVOLVE, row_case(game, EVOLVE)) + [0.0])                   # 17 arguments
        assert len(_args(EVOLVE, row_case(game, EVOLVE))) == 16 == _abi.EDIT_MAX_ARGS
        g.sync()
        for a, b in zip(kept, _buffers(g)):
            assert np.array_equal(a, b), "a refused call wrote a buffer"
        _assert_same_snapshot(snap, _snapshot(g), "after the refusals")
        back = np.empty_like(marker)
        hip.memcpy_dtoh(back, out, back.nbytes)
        assert np.array_equal(back, marker), "a refused call wrote its output"
        assert np.array_equal(g.reduce(ACT, good), rows)
    finally:
        g.sync()
        hip.free(out)


# ---------------------------------------------------------------- 7. the adapters

def test_plan_rollout_is_plan_steps(hip_lib):
    """ToyboxVecEnv.plan_rollout(k) = k plan_step calls (the evolution from the carry from the second step on), and the actions
    it reports are those a host-driven controller picks with evolve_search + np.roll"""
    from toybox_amd.envs.vec_env import ToyboxVecEnv
    n, k = 33, 4
    kw = dict(planner="evolve", steps=4, depth=4, hold=2, population=8, generations=1, elite=2, plan_seed=3, t=5)
    a, b = (ToyboxVecEnv("breakout", n, seed=11, cache_terminal_state=False) for _ in range(2))
    try:
        for e in (a, b):
            e.reset()
            for t in range(30):
                e.step(np.full(n, t % 4))
        obs, reward, done, infos = a.plan_rollout(k, **kw)
        actions = a.plan_actions()
        assert obs.shape[0] == n and reward.shape == (k, n) and reward.dtype == np.float32 and done.shape == (k, n) and done.dtype == bool and actions.shape == (k, n)
        for i in range(k):
            o2, r2, d2, _ = b.plan_step(**dict(kw, t=kw["t"] + i))
            assert np.array_equal(b.plan_actions()[0], actions[i]) and np.array_equal(r2, reward[i]) and np.array_equal(d2, done[i]), i
        assert np.array_equal(o2, obs) and bytes(a.engine.get_states()) == bytes(b.engine.get_states())
        assert len(infos) == n and "lives" in infos[0]
    finally:
        a.close()
        b.close()


def test_preproc_plan_rollout_is_plan_steps(hip_lib):
    from toybox_amd.envs.vec_env import ToyboxPreprocVecEnv
    n, k = 17, 3
    kw = dict(planner="beam", steps=4, depth=3, width=2, t=2)
    a, b = (ToyboxPreprocVecEnv("space_invaders", n, seed=5) for _ in range(2))
    try:
        for e in (a, b):
            e.reset()
            for t in range(10):
                e.step(np.full(n, t % 6))
        obs, reward, done, _ = a.plan_rollout(k, **kw)
        for i in range(k):
            o2, r2, d2, _ = b.plan_step(**dict(kw, t=kw["t"] + i))
            assert np.array_equal(b.plan_actions()[0], a.plan_actions()[i]) and np.array_equal(r2, reward[i]) and np.array_equal(d2, done[i]), i
        assert np.array_equal(np.asarray(o2), np.asarray(obs)) and bytes(a.engine.get_states()) == bytes(b.engine.get_states())
    finally:
        a.close()
        b.close()
