"""The agent wrapper stack at every sub-frame of every reset phase: a lost life or a game over placed on raw frame f of the agent's own
step, of EpisodicLifeEnv's no-op step and of both of FireResetEnv's steps, in neighbouring envs at different frames, for every wrapper
combination of ROWS; and a game over inside NoopResetEnv's frames.  tests/wrapper_events.py holds the builders and a second formulation
of the stack in Python with an event log.

CPU cases (no mark): the oracle's tbx_agent_* against the Python restatement at 65 envs, every output of every env at the reset and at each
of the STEPS agent steps after the write, then every state record and simulator RNG; and, on the restatement's log, the conditions on the
inputs -- every cell reachable(game, row) names holds at least 2 envs, no cell of UNREACHABLE is met, every 64 consecutive envs hold at
least 4 different cells, the observation sources of sources_reached() are returned.  Three cases show the comparison has teeth, one per
game that the cell assertions fail once a builder is taken away.

Device cases (gpu): the HIP engine against the oracle, every env, at 65 and 257 envs, through tbx_agent_step (new_plane 0, 1, 2),
tbx_agent_step_device on a caller's stream, tbx_agent_step_begin / _end, both step forms where the game has two, Breakout on its brick
tables, and in every row the generic observation path (TBX_OPT_AGENT_GENERIC), whose documented difference is asserted in exactly
the envs the log names."""
import collections
import functools

import numpy as np
import pytest

import wrapper_events as we
from fork_replay import sim_rngs, states_bytes
from support import FrameChecker, agent_stack_frames, area_resize_exact, read_buffer
from test_gpu_agent_scale import code_of, host_step, run_blocks
from toybox_amd import Engine, _abi

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
SIZES = [65, 257]
SEED, STEPS = 11, 4
BASE = dict(skip=4, out_h=84, out_w=84, stack=4, clip_reward=False, episodic_life=True, fire_reset=True, noop_max=0, stack_fill=0)
# every wrapper on and off beside every other at skip 4; the short repeats (skip 1 never writes slot A, skip 2 writes it in frame 0);
# FrameStack's fill; ClipRewardEnv once, with one illegal action id in the last env at the last step; Breakout on its brick tables
ROWS = collections.OrderedDict([
    ("e1f1", {}), ("e1f0", dict(fire_reset=False)), ("e0f1", dict(episodic_life=False)), ("e0f0", dict(episodic_life=False, fire_reset=False)),
    ("noops", dict(noop_max=5, noop_seed=2024)), ("skip1", dict(skip=1)), ("skip2", dict(skip=2)), ("skip3", dict(skip=3)), ("fill1", dict(stack_fill=1)),
    ("clip", dict(clip_reward=True)), ("custom", dict(episodic_life=False, fire_reset=False)),
    ("noops_written", dict(noop_max=5, noop_seed=2024))])
# "noops": in SpaceInvaders and Amidar one life per game, no written states and counts around the game's end; in Breakout and GridWorld,
# where no game ends inside the no-op frames, default lives, the written states and small counts -- which is what "noops_written" is for
# the first two, so that the timed cells are held with NoopResetEnv on in every game
ONLY = {"custom": ("breakout",), "noops_written": ("space_invaders", "amidar")}
CASES = [(g, r) for g in GAMES for r in ROWS if g in ONLY.get(r, GAMES)]
HAS_LIVES = ("breakout", "space_invaders", "amidar")
NOOP_GAME_OVER = ("space_invaders", "amidar")      # a game over inside NoopResetEnv's frames: see UNREACHABLE

Scenario = collections.namedtuple("Scenario", "game row n config agent noops records actions")


@functools.lru_cache(maxsize=None)
def scenario(game, row, n, lib):
    """the inputs of one case: config, agent options, injected no-op counts, the records written after the reset, int32[STEPS][n] actions"""
    agent = dict(BASE, **ROWS[row])
    config = noops = records = None
    if row in ("noops", "noops_written"):
        if row == "noops" and game in NOOP_GAME_OVER:
            config, noops = we.build_noop_game_over(game, n, SEED, lib)
        else:
            noops = (np.arange(n) % 7).astype(np.int32)               # (0: that env keeps the default rule, 1 + hash % noop_max)
    if config is None:
        with Engine(game, n, config=config, lib=lib) as o:
            prepare(o, Scenario(game, row, n, config, agent, noops, None, None), 0)
            records = we.BUILDERS[game](o.get_states_np(), n, agent["skip"])
        if row == "custom":
            records["bricks"]["points"][:, 0] += 1                  # no canonical wall has this brick: the engine goes to its tables
    actions = np.stack([we.event_actions(game, n)] * STEPS)
    if row == "clip":
        actions[STEPS - 1, n - 1] = 18
    for a in (noops, records, actions):
        if a is not None:
            a.flags.writeable = False
    return Scenario(game, row, n, config, agent, noops, records, actions)


def prepare(e, sc, new_plane):
    e.seed(SEED)
    e.agent_init(new_plane=new_plane, **sc.agent)
    if sc.noops is not None:
        e.agent_set_noops(sc.noops)
    e.agent_reset()


def fetch(e, rec):
    """the stack (through the ring's head where there is a ring), the newest plane and the ring head into rec"""
    n, oh, ow, st = e._agent_shape
    obs = np.empty((n, oh, ow, st), np.uint8)
    agent_stack_frames(e)(0, n, obs)
    rec["obs"] = obs
    if e._agent_ring or rec.get("want_plane"):
        rec["plane"] = read_buffer(e, _abi.BUF_AGENT_PLANE, (n, oh, ow))
    if e._agent_ring:
        rec["head"] = e.agent_ring_head()
    return rec


def abi_run(e, sc, new_plane):
    """reset, write, STEPS host-form steps on an engine of either library -> [record of the reset, records of the steps], end state"""
    prepare(e, sc, new_plane)
    e.sync()
    recs = [fetch(e, {"want_plane": new_plane == 1})]
    if sc.records is not None:
        e.set_states_np(0, sc.records)
    for t in range(STEPS):
        rc, out = host_step(e, sc.actions[t])
        out["code"] = rc
        out["want_plane"] = new_plane == 1
        recs.append(fetch(e, out))
    return recs, (states_bytes(e), sim_rngs(e), e.scalars())


@functools.lru_cache(maxsize=3)
def oracle_run(game, row, n, lib):
    sc = scenario(game, row, n, lib)
    with Engine(game, n, config=sc.config, lib=lib) as o:
        return abi_run(o, sc, 1)


def compare(got, want, where, obs_override=None):
    """one record against another: every field both hold, every env.  obs_override = (envs, obs, plane): what these envs show instead"""
    for name in ("reward", "done", "ep_done", "ep_return", "ep_length", "obs", "plane"):
        g, w = got.get(name), want.get(name)
        if g is None or w is None:
            continue
        if name in ("obs", "plane") and obs_override is not None:
            w = w.copy()
            w[obs_override[0]] = obs_override[1 if name == "obs" else 2][obs_override[0]]
        ne = (np.asarray(g) != np.asarray(w)).reshape(len(w), -1).any(axis=1)
        if name in ("ep_return", "ep_length"):
            ne &= want["ep_done"] != 0                               # (valid only where an episode ended)
        if ne.any():
            i = int(np.flatnonzero(ne)[0])
            raise AssertionError("%s: %s differs in %d envs, first env %d" % (where, name, int(ne.sum()), i))
    for name in ("code", "head"):
        if name in got and name in want and got[name] is not None and want[name] is not None:
            assert got[name] == want[name], "%s: %s is %r, expected %r" % (where, name, got[name], want[name])


def compare_runs(got, want, what, overrides=None):
    for t, (g, w) in enumerate(zip(got, want)):
        compare(g, w, "%s %s" % (what, "reset" if t == 0 else "step %d" % (t - 1)), overrides[t] if overrides else None)


def compare_end(got, want, what):
    for name, g, w in zip(("state record", "simulator RNG"), got[:2], want[:2]):
        ne = (g != w).reshape(len(w), -1).any(axis=1)
        assert not ne.any(), "%s: the %s of %d envs differs, first env %d" % (what, name, int(ne.sum()), int(np.flatnonzero(ne)[0]))
    for name, g, w in zip(("score", "lives", "level", "game_over"), got[2], want[2]):
        assert np.array_equal(g, w), "%s: %s differs, first env %d" % (what, name, int(np.flatnonzero(g != w)[0]))


def expected_head(t):
    """include/toybox_amd.h: every tbx_agent_reset / agent step writes slot head = (head + 1) % stack; record t is call t + 1"""
    return (t + 1) % BASE["stack"]


def restatement_run(sc, lib, fault=None, resize=we.area_resize_int):
    """the same calls on the Python restatement over a raw engine of `lib` -> records, end state, the Stack (for its log)"""
    with Engine(sc.game, sc.n, config=sc.config, lib=lib) as raw:
        raw.seed(SEED)
        st = we.Stack(raw, noops=sc.noops, fault=fault, resize=resize, **sc.agent)
        recs = [st.reset()]
        if sc.records is not None:
            st.write_states(sc.records)
        for t in range(STEPS):
            recs.append(st.step(sc.actions[t]))
        return recs, (states_bytes(raw), sim_rngs(raw), raw.scalars()), st


# ================================================================ what the oracle can reach, and what it cannot

def step_calls(agent):
    return ["step"] + (["lost_life_noop_step"] + (["fire_step_1", "fire_step_2"] if agent["fire_reset"] else []) if agent["episodic_life"] else [])


def reachable(game, row):
    """the cells the builders must fill.  With EpisodicLifeEnv on, the written lives are below the remembered ones, the first step reports
    done and raw frame F of the builders falls into call F // skip of [step, lost_life_noop_step, fire_step_1, fire_step_2] (without
    FireResetEnv the frames past the no-op step are the next agent steps' own); with it off nothing resets before the life goes, and
    frame F is frame F % skip of agent step F // skip."""
    agent = dict(BASE, **ROWS[row])
    frames = range(agent["skip"])
    if row == "noops" and game in NOOP_GAME_OVER:
        return {("noop_frames", "in", "game_over")}
    if game == "gridworld":
        return {("step", f, "game_over") for f in frames}
    return {(c, f, w) for c in step_calls(agent) for f in frames for w in ("life_lost", "game_over")}


# (game or None for all, call or None, what or None, why the oracle cannot get there): a cell that matches must never appear in a log
UNREACHABLE = [
    ("breakout", "noop_frames", "game_over", "a new Breakout game has no ball in play until FIRE, and NoopResetEnv sends no-ops only"),
    ("gridworld", "noop_frames", "game_over", "a GridWorld player moves only on a direction button: no-op frames change nothing"),
    ("gridworld", None, "life_lost", "GridWorld has one life: reaching a goal cell is the game over"),
    ("gridworld", "lost_life_noop_step", None, "the call runs only after a lost life that is not a game over, and GridWorld has none"),
    ("gridworld", "fire_step_1", "game_over", "the step follows a real reset in GridWorld: the default board's goal is farther from the start than UP repeated"),
    ("gridworld", "fire_step_2", "game_over", "as fire_step_1: RIGHT repeated after UP ends at the wall of column 4"),
    (None, "noop_frames", "life_lost", "NoopResetEnv looks at done alone; the log files a life that is not the last under nothing here"),
]
# SpaceInvaders cannot lose a second life inside the get-ready time after one goes (oracle/orc_si.c phase A returns before anything can
# hit the ship, TBX_SI_NEW_LIFE_TIME = 128 frames > 4 calls of 4): asserted below as "nothing goes in an agent step once a life has".

# the observation sources returned by an agent step or the reset.  Never returned: "black" and "slot_a" -- a call of MaxAndSkipEnv that
# leaves a slot unwritten was cut short by a game over, so a real reset follows and what is returned is its raw frame or, with
# FireResetEnv, the buffer after two more whole steps; EpisodicLifeEnv's no-op step, whose cut-short buffer IS returned, is never the
# first call on a buffer (an agent step has run before a life can be remembered as lost).  "slot_b" is what skip 1 always has.
def sources_reached(game, row):
    agent = dict(BASE, **ROWS[row])
    both = "slot_b" if agent["skip"] == 1 else "max"
    if row == "noops" and game in NOOP_GAME_OVER:
        return {both}
    out = {both}
    if not agent["fire_reset"]:
        out.add("live")
    if agent["fire_reset"] and agent["episodic_life"] and game in HAS_LIVES:
        out.add("kept")
    return out


def assert_log_conditions(sc, st, recs):
    game, row, n = sc.game, sc.row, sc.n
    counts = we.cell_counts(st.log, t_first=-1 if sc.records is None else 0)
    for cell in sorted(reachable(game, row), key=str):
        assert len(counts.get(cell, ())) >= 2, "%s %s: cell %r holds %d envs" % (game, row, cell, len(counts.get(cell, ())))
    for g, call, what, why in UNREACHABLE:
        hit = [c for c in counts if (g in (None, game)) and call in (None, c[0]) and what in (None, c[2])]
        assert not hit, "%s %s: a cell listed as unreachable was reached: %r (%s)" % (game, row, hit, why)
    if sc.records is not None:
        first = we.first_event_cell(st.log, n)
        for lo in range(0, n - 63):
            assert len({c for c in first[lo:lo + 64] if c is not None}) >= min(4, len(reachable(game, row))), (game, row, lo)
    if game == "space_invaders":
        waiting = set()                                             # (env, agent step) in which a life that was not the last has gone
        for ev in st.log:
            if ev.what != "nothing" and ev.call != "noop_frames":
                assert (ev.env, ev.t) not in waiting, "a second life went inside the get-ready time: %r" % (ev,)
                if ev.what == "life_lost":
                    waiting.add((ev.env, ev.t))
    seen = {s for rec in recs for s in rec["source"]}
    assert sources_reached(game, row) <= seen <= {"slot_b", "max", "live", "kept"}, (game, row, seen)


# ================================================================ CPU cases

@pytest.mark.parametrize("game,row", CASES)
def test_oracle_equals_the_restatement_and_the_cells_are_filled(game, row, oracle_lib):
    n = 65
    sc = scenario(game, row, n, oracle_lib)
    want, want_end = oracle_run(game, row, n, oracle_lib)
    got, got_end, st = restatement_run(sc, oracle_lib)
    for t, rec in enumerate(got):
        assert rec["head"] == expected_head(t)
        del rec["head"]                                             # (the oracle's run keeps the rolled stack: it has no head)
    compare_runs(want, got, "%s %s oracle against restatement" % (game, row))
    compare_end(want_end, got_end, "%s %s" % (game, row))
    assert_log_conditions(sc, st, got)
    codes = [rec["code"] for rec in want[1:]]
    if row == "clip":
        assert codes[-1] in (_abi.E_ACTION, _abi.E_NEEDS_RESET), codes
    if row in ("e1f1", "e1f0") and game in HAS_LIVES:               # a game that ended inside the ignored no-op step is stepped on
        assert codes[0 if row == "e1f1" else 1] == _abi.E_NEEDS_RESET, codes


@pytest.mark.parametrize("row,env", [("e1f1", 22), ("e1f0", 0)])
@pytest.mark.parametrize("game", GAMES)
def test_the_fast_resize_is_the_exact_one_on_these_frames(game, row, env, oracle_lib):
    """the restatement warps with support.area_resize_int; on the frames of this module the rational-arithmetic definition,
    support.area_resize_exact, gives the same stacks: one env of the e1f1 row, whose game ends in FireResetEnv's first step (sources max
    and kept), and one of the e1f0 row, whose game ends in the first frame after the write (source live: a reset's raw frame)"""
    sc = scenario(game, row, 65, oracle_lib)
    small = Scenario(game, row, 1, sc.config, sc.agent, None, sc.records[[env]], sc.actions[:, :1])
    fast = restatement_run(small, oracle_lib)[0]
    exact = restatement_run(small, oracle_lib, resize=area_resize_exact)[0]
    assert "live" in {rec["source"][0] for rec in fast} or row == "e1f1"
    compare_runs(fast, exact, "%s %s exact resize" % (game, row))


@pytest.mark.parametrize("game", GAMES)
def test_the_cell_assertions_hold_each_builder(game, oracle_lib):
    """the e1f1 row with the game's builder replaced by the identity (the states of the reset written back as they are): the log no
    longer fills the cells and assert_log_conditions says so -- what holds every builder, game by game, where the branch ratchet of
    tests/test_wrapper_reach.py cannot (the wrapper functions are the same code for every game)"""
    sc = scenario(game, "e1f1", 65, oracle_lib)
    with Engine(game, 65, lib=oracle_lib) as o:
        prepare(o, sc, 0)
        plain = o.get_states_np()
    dull = sc._replace(records=plain)
    recs, _, st = restatement_run(dull, oracle_lib)
    with pytest.raises(AssertionError, match=r"cell \(.* holds 0 envs"):
        assert_log_conditions(dull, st, recs)


def first_difference(a, b):
    for t, (x, y) in enumerate(zip(a, b)):
        try:
            compare(x, y, "")
        except AssertionError as err:
            return t, int(str(err).rsplit("first env ", 1)[1])
    return None


TEETH = [("step_after_done", "space_invaders", "e1f0"), ("slot_a_late", "breakout", "e0f0"), ("rewritten_buffer", "breakout", "e1f1")]


@pytest.mark.parametrize("fault,game,row", TEETH)
def test_the_comparison_notices_one_wrong_reading_of_the_stack(fault, game, row, oracle_lib):
    """the restatement read wrongly in one way -- it keeps stepping after done, writes slot A one frame late, or takes the rewritten
    buffer after a life lost in step(2) -- fails the comparison with the oracle, at the step and in the env where that reading first
    changes the restatement's own outputs, and that place is one the log explains"""
    n = 65
    sc = scenario(game, row, n, oracle_lib)
    want, _ = oracle_run(game, row, n, oracle_lib)
    good, _, st = restatement_run(sc, oracle_lib)
    bad, _, _ = restatement_run(sc, oracle_lib, fault=fault)
    place = first_difference(bad, good)
    assert place is not None and place[0] >= 1, place
    t, env = place
    mine = [ev for ev in st.log if ev.env == env and ev.t == t - 1]
    if fault == "step_after_done":      # the cut-short no-op step whose stale buffer is the observation: the wrong reading rewrote it
        assert any(ev.call == "lost_life_noop_step" and ev.stopped and ev.f < sc.agent["skip"] - 1 for ev in mine), mine
    if fault == "slot_a_late":
        # Breakout, no reset-time wrapper: an env whose game ends inside the step returns a reset's raw frame, and one whose ball goes
        # before frame skip - 2 has the same picture in both slots.  The first env whose slots differ is the first whose life (not the
        # last) goes in frame skip - 1, slot 2 (skip - 1) + 1 of the builders, in the step that sees the write: slot A still shows the ball
        assert (t - 1, env) == (0, 2 * (sc.agent["skip"] - 1) + 1), place
        assert [(ev.call, ev.f, ev.what, ev.stopped) for ev in mine] == [("step", sc.agent["skip"] - 1, "life_lost", False)], mine
    if fault == "rewritten_buffer":
        assert good[t]["source"][env] == "kept" and any(ev.call == "fire_step_2" and ev.what == "life_lost" for ev in mine), mine
    with pytest.raises(AssertionError, match=r"step %d: \w+ differs in \d+ envs, first env %d$" % (t - 1, env)):
        compare_runs(want, bad, "teeth")


def reach(lib):
    """the oracle's side of every case of this module over `lib`, in the three observation forms (tests/test_wrapper_reach.py)"""
    for game, row in CASES:
        sc = scenario(game, row, 65, lib)
        for new_plane in ((0, 1, 2) if row in ("e1f1", "fill1") else (1,)):
            with Engine(game, 65, config=sc.config, lib=lib) as o:
                abi_run(o, sc, new_plane)
                if new_plane == 1 and row == "e1f1":
                    o.agent_reset()                                 # venv.reset() in the middle of an episode


# ================================================================ device cases

def kept_envs(st, t):
    """the envs whose observation of record t is FireResetEnv's step(2) buffer although a no-op STEP has rewritten it since"""
    out = []
    for ev in st.log:
        if ev.t == t - 1 and ev.call == "fire_step_2" and ev.what == "life_lost":
            out.append(ev.env)
    return np.asarray(sorted(out), np.int64)


def device_engine(game, n, sc, hip_lib, new_plane, options=()):
    g = Engine(game, n, config=sc.config, lib=hip_lib)
    for opt, v in options:
        g.set_option(opt, v)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("game,row", CASES)
def test_gpu_host_form_equals_oracle(game, row, n, hip_lib, oracle_lib):
    """tbx_agent_step with host actions for new_plane 0, 1 and 2 (the ring read through its head, TBX_BUF_AGENT_PLANE beside it), and
    under each step form where the game has two: every output of every env at the reset and every step, then every state record and RNG"""
    sc = scenario(game, row, n, oracle_lib)
    want, want_end = oracle_run(game, row, n, oracle_lib)
    forms = [()] + ([((_abi.OPT_STEP_FORM, f),) for f in (1, 2)] if game in ("breakout", "amidar") and row != "custom" else [])
    for new_plane, options in [(p, ()) for p in (0, 1, 2)] + [(0, o) for o in forms[1:]]:
        what = "%s %s n=%d new_plane=%d %r" % (game, row, n, new_plane, options)
        with device_engine(game, n, sc, hip_lib, new_plane, options) as g:
            got, got_end = abi_run(g, sc, new_plane)
            if new_plane == 2:
                for t, rec in enumerate(got):
                    assert rec["head"] == expected_head(t), (what, t)
                    del rec["head"]
            compare_runs(got, want, what)
            compare_end(got_end, want_end, what)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("game,row", CASES)
def test_gpu_device_form_on_a_callers_stream_equals_oracle(game, row, n, hip_lib, oracle_lib):
    """tbx_agent_step_device: the STEPS steps back to back on a caller's stream, readers queued between them, one tbx_sync at the end whose
    code is the oracle's (TBX_E_NEEDS_RESET where a game ended inside the ignored no-op step); ring form"""
    from toybox_amd import hip
    sc = scenario(game, row, n, oracle_lib)
    o, head, g = Engine(game, n, config=sc.config, lib=oracle_lib), Engine(game, 1, config=sc.config, lib=oracle_lib), device_engine(game, n, sc, hip_lib, 2)
    stream, dev = hip.Stream(), hip.malloc(sc.actions.nbytes)
    try:
        hip.memcpy_htod(dev, np.ascontiguousarray(sc.actions), sc.actions.nbytes)
        for e, mode in ((o, 0), (g, 2)):
            prepare(e, sc, mode)
            if sc.records is not None:
                e.set_states_np(0, sc.records)
        head.seed(SEED)
        head.agent_init(new_plane=2, **dict(sc.agent, episodic_life=False, fire_reset=False))      # (it is stepped for its head alone)
        head.agent_reset()

        def oracle_step(t):
            head.agent_step(np.zeros(1, np.int32), tolerate_needs_reset=True)
            return host_step(o, sc.actions[t])[0]

        what = "%s %s n=%d device form" % (game, row, n)
        _, codes, _ = run_blocks(o, head, [g], stream, STEPS, STEPS, lambda e, t, sp: e.agent_step_device(dev + t * n * 4, stream=sp),
                                 oracle_step, FrameChecker((84, 84, 4)), what)
        compare_end((states_bytes(g), sim_rngs(g), g.scalars()), (states_bytes(o), sim_rngs(o), o.scalars()), what)
        if row in ("e1f1", "e1f0") and game in HAS_LIVES:
            assert codes == [_abi.E_NEEDS_RESET], codes
    finally:
        g._lib.tbx_sync(g._h)
        stream.close()
        hip.free(dev)
        for e in (o, head, g):
            e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("game,row", CASES)
def test_gpu_begin_end_form_equals_oracle(game, row, n, hip_lib, oracle_lib):
    """tbx_agent_step_begin / _end with page-locked outputs, stack and newest plane among them (the chunked observation path)"""
    sc = scenario(game, row, n, oracle_lib)
    want, want_end = oracle_run(game, row, n, oracle_lib)
    what = "%s %s n=%d begin/end" % (game, row, n)
    with device_engine(game, n, sc, hip_lib, 1) as g:
        prepare(g, sc, 1)
        if sc.records is not None:
            g.set_states_np(0, sc.records)
        out = {"reward": g.host_array((n,), np.float32), "done": g.host_array((n,), np.uint8), "obs": g.host_array((n, 84, 84, 4)),
               "plane": g.host_array((n, 84, 84)), "ep_done": g.host_array((n,), np.uint8), "ep_return": g.host_array((n,), np.float32),
               "ep_length": g.host_array((n,), np.int32)}
        for t in range(STEPS):
            g.agent_step_begin(sc.actions[t], **out)
            out["code"] = code_of(g.agent_step_end)
            compare(out, want[t + 1], "%s step %d" % (what, t))
            del out["code"]
        compare_end((states_bytes(g), sim_rngs(g), g.scalars()), want_end, what)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("game,row", CASES)
def test_gpu_generic_path_equals_oracle_but_for_the_documented_envs(game, row, n, hip_lib, oracle_lib):
    """TBX_OPT_AGENT_GENERIC = 1, the cross-check path.  DESIGN.md section 8: it has no kept copy of MaxAndSkipEnv's buffer, so after a
    life lost inside FireResetEnv's step(2) it shows the buffer as the no-op step that followed rewrote it.  In exactly the envs the
    restatement's log puts there, that observation (the restatement produces it) is asserted; everywhere else the oracle's."""
    sc = scenario(game, row, n, oracle_lib)
    want, want_end = oracle_run(game, row, n, oracle_lib)
    overrides = None
    if sc.agent["fire_reset"] and sc.agent["episodic_life"] and game in HAS_LIVES:
        alt, _, st = restatement_run(sc, oracle_lib, fault="rewritten_buffer")
        kept = [kept_envs(st, t) for t in range(STEPS + 1)]
        if sc.records is not None:
            assert sum(len(k) for k in kept) >= 2
        # (the rewritten plane stays in the env's stack for the steps that follow: STEPS is no more than the stack's depth)
        overrides = [(np.unique(np.concatenate(kept[:t + 1])), alt[t]["obs"], alt[t]["plane"]) for t in range(STEPS + 1)]
    what = "%s %s n=%d generic" % (game, row, n)
    with device_engine(game, n, sc, hip_lib, 1, ((_abi.OPT_AGENT_GENERIC, 1),)) as g:
        got, got_end = abi_run(g, sc, 1)
        compare_runs(got, want, what, overrides)
        compare_end(got_end, want_end, what)
