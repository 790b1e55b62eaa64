"""The agent pipeline against the oracle at the size and in the loop form its benchmark number is taken in, and
tbx_agent_step_device (the policy loop's entry point: actions in HBM).

bench.py's agent rows run 65 536 envs with every baselines wrapper on, tbx_agent_step_synthetic back to back on a caller's
stream, nothing synchronised between the steps, for both observation forms (the rolled stack, the ring of the last planes) -- and
check no output.  Here the same engines, seeds and calls run beside the CPU oracle: every env's reward, done flag and episode record
at every step, every env's whole observation stack every fourth step (with a stack of 4: no plane a kernel wrote goes unread), from
mid-game states in which thousands of envs lose their last life inside the window, so that the in-kernel reset path compacts
thousands of envs per step.

The loop (run_blocks) is written against the C-ABI alone: the oracle-only cases drive it with the CPU checker in the device's
place -- at a smaller batch, without a GPU -- and assert the conditions on the inputs (how many games end inside the window, that
both error codes are reached) there too.
"""
import ctypes as C

import numpy as np
import pytest

from support import (FrameChecker, agent_stack_frames, amidar_edit_last_lives, donor_records, engine_is_oracle, queue_read_buffer,
                     read_buffer, synthetic_actions, write_mid_game_states)
from toybox_amd import Engine, _abi
from toybox_amd._lib import ToyboxAmdError
from toybox_amd.games import codec

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]

# ---------------------------------------------------------------- bench.py's agent workload, restated (the module is not imported)
BENCH_ENVS = 65536                # bench.py:1325-1346 agent_path_rates(hip, n = the headline batch); README's agent rows
BENCH_SEED = 1234                 # bench.py:94   SEED_BASE, eng.seed(SEED_BASE) at :498 and :1337
BENCH_ACTION_SEED = 1337          # bench.py:93   ACTION_SEED, eng.agent_step_synthetic(ACTION_SEED, t, stream=stream.ptr) at :505-509, :1342-1346
BENCH_AGENT = dict(skip=4, out_h=84, out_w=84, stack=4, clip_reward=True, episodic_life=True, fire_reset=True, noop_max=30,
                   noop_seed=2024)   # bench.py:500-501 with --deepmind, :1338-1339; new_plane = 0 and 2 (:501 --obs ring, :1339 mode)

# ---------------------------------------------------------------- mid-game states: the window is to be full of events
# From a fresh reset 48 agent steps end no game in Breakout, SpaceInvaders or Amidar: the no-op / fire reset path would never run
# after step 0.  So every env starts from the state of a donor env that has played for a while, and every second env is on its
# last life.  GridWorld ends games from a fresh reset by itself (DONOR_FRAMES 0: no donor, no edit).  The recipe (donor_records,
# write_mid_game_states: 1 024 donor envs, engine seed 99, action seed 7, 400 / 600 / 600 / 0 frames) lives in tests/support.py.
WINDOW, BLOCK = 32, 4
# The floor under the events, as a share of the batch with a real game over (TBX_BUF_AGENT_EP_DONE) inside the window -- asserted
# on the ORACLE's outputs: when it is missed the inputs are wrong, not the device.
EVENT_FLOOR = {"breakout": 0.25, "space_invaders": 0.01, "amidar": 0.01, "gridworld": 0.01}

OUTPUTS = (("reward", _abi.BUF_AGENT_REWARD, np.float32), ("done", _abi.BUF_AGENT_DONE, np.uint8),
           ("ep_done", _abi.BUF_AGENT_EP_DONE, np.uint8), ("ep_return", _abi.BUF_AGENT_EP_RETURN, np.float32),
           ("ep_length", _abi.BUF_AGENT_EP_LENGTH, np.int32))


def code_of(call):
    """the C-ABI return code behind a call of the Python host, which raises every code but 0"""
    try:
        call()
    except ToyboxAmdError as err:
        return err.code
    return _abi.OK


def block_code(step_codes):
    """what tbx_sync reports for steps that ran unsynchronised, from the codes of the same steps taken one at a time: the device
    keeps ONE error word, and a step on an env that needed a reset outranks an illegal action id (include/toybox_amd.h, tbx_sync)"""
    assert set(step_codes) <= {_abi.OK, _abi.E_ACTION, _abi.E_NEEDS_RESET}, step_codes
    if _abi.E_NEEDS_RESET in step_codes:
        return _abi.E_NEEDS_RESET
    return _abi.E_ACTION if _abi.E_ACTION in step_codes else _abi.OK


def compare_stacks(chk, e, o, n, what):
    chk.compare(agent_stack_frames(e), agent_stack_frames(o), n, what=what)


def compare_outputs(got, want, what):
    """one step's outputs of every env: reward (float32, exact), done, ep_done; ep_return / ep_length where ep_done is set (the
    header calls them valid only there)"""
    for name in ("reward", "done", "ep_done"):
        if not np.array_equal(got[name], want[name]):
            bad = np.flatnonzero(got[name] != want[name])
            raise AssertionError("%s: %s differs in %d envs, first env %d (got %r, want %r)"
                                 % (what, name, len(bad), bad[0], got[name][bad[0]], want[name][bad[0]]))
    ended = want["ep_done"] != 0
    for name in ("ep_return", "ep_length"):
        if not np.array_equal(got[name][ended], want[name][ended]):
            bad = np.flatnonzero(ended & (got[name] != want[name]))
            raise AssertionError("%s: %s differs in %d envs whose episode ended, first env %d (got %r, want %r)"
                                 % (what, name, len(bad), bad[0], got[name][bad[0]], want[name][bad[0]]))


def run_blocks(o, head_oracle, devices, stream, steps, block, device_step, oracle_step, chk, what):
    """`steps` agent steps in blocks of `block`.  Every engine of `devices` (the libraries under test) runs a block's steps back
    to back through device_step(e, t, stream_ptr) with no host synchronisation in between; behind each step and before the
    next, copies of the five per-env outputs are queued on the same stream into page-locked arrays of that step.  Meanwhile the
    oracle o takes the same steps one at a time, oracle_step(t) -> the step's return code.  At the block's end the stream and
    then the engine are synchronised and everything is compared: every step's outputs of every env, the code of tbx_sync, the
    ring head (head_oracle: a one-env oracle engine with the ring, stepped alongside by oracle_step) and every env's stack.
    Returns (envs with a real game over inside the window bool[n], the blocks' expected codes, their steps' codes)."""
    n = o.n_envs
    sp = stream.ptr if stream is not None else 0
    outs = {id(e): {name: e.host_array((block, n), dt) for name, _, dt in OUTPUTS} for e in devices}
    ended = np.zeros(n, bool)
    codes, step_codes = [], []
    for t0 in range(0, steps, block):
        for e in devices:
            for j in range(block):
                device_step(e, t0 + j, sp)
                for name, which, _ in OUTPUTS:
                    queue_read_buffer(e, which, outs[id(e)][name][j], stream)
        want, rcs = [], []
        for j in range(block):                                      # (the CPU steps run while the device's are in flight)
            rcs.append(oracle_step(t0 + j))
            want.append({name: read_buffer(o, which, (n,), dt) for name, which, dt in OUTPUTS})
            ended |= want[-1]["ep_done"] != 0
        expect = block_code(rcs)
        codes.append(expect)
        step_codes.append(rcs)
        if stream is not None:
            stream.synchronize()
        for e in devices:
            where = "%s %s steps %d..%d" % (what, "ring" if e._agent_ring else "stack", t0, t0 + block - 1)
            rc = e._lib.tbx_sync(e._h)
            for j in range(block):
                compare_outputs({name: a[j] for name, a in outs[id(e)].items()}, want[j], "%s step %d" % (where, t0 + j))
            assert rc == expect, "%s: tbx_sync returned %d, the oracle's steps %r" % (where, rc, rcs)
            if e._agent_ring:
                assert e.agent_ring_head() == head_oracle.agent_ring_head(), where
            compare_stacks(chk, e, o, n, where)
    return ended, codes, step_codes


def assert_same_end_state(o, devices, n, where):
    """the score / lives / level / game-over vectors of the whole batch, and the whole state record and simulator RNG of 96 envs:
    the ends of the batch, both sides of its middle (the edge of a 32 768-env launch) and a random sample"""
    want = o.scalars()
    sample = sorted({0, n // 2 - 1, n // 2, n - 1} | set(np.random.default_rng(3).choice(n, min(92, n), replace=False).tolist()))
    for e in devices:
        for name, x, y in zip(("score", "lives", "level", "game_over"), e.scalars(), want):
            assert np.array_equal(x, y), "%s: %s differs, first env %d" % (where, name, np.flatnonzero(x != y)[0])
        for i in sample:
            assert bytes(e.get_state(i)) == bytes(o.get_state(i)), "%s: the state record of env %d differs" % (where, i)
            assert e.get_sim_rng(i) == o.get_sim_rng(i), "%s: the simulator RNG of env %d differs" % (where, i)


def host_step(e, actions):
    """tbx_agent_step with host pointers and no observation output (the stacks are compared where they lie) -> (code, outputs)"""
    n = e.n_envs
    a = np.ascontiguousarray(actions, np.int32)
    reward, done = np.empty(n, np.float32), np.empty(n, np.uint8)
    rc = e._lib.tbx_agent_step(e._h, a.ctypes.data_as(C.c_void_p), reward.ctypes.data_as(C.c_void_p), done.ctypes.data_as(C.c_void_p), None)
    ep = e.agent_episodes()
    return rc, {"reward": reward, "done": done, "ep_done": ep[0].astype(np.uint8), "ep_return": ep[1], "ep_length": ep[2]}


# ================================================================ A. the bench's size, the bench's form

def bench_form_parity(game, n, o, head_oracle, devices, stream, oracle_lib, pinned):
    """the whole of part A for engines that exist already: returns the share of envs with a real game over inside the window"""
    chk = FrameChecker((84, 84, 4), pinned=pinned)
    for e, mode in [(o, 0), (head_oracle, 2)] + [(d, d.want_plane) for d in devices]:
        e.seed(BENCH_SEED)
        e.agent_init(new_plane=mode, **BENCH_AGENT)
        e._check(e._lib.tbx_agent_reset(e._h, None))               # (no host copy of the stacks: 1.85 GB each at the bench's size)
    write_mid_game_states([o] + devices, n, donor_records(game, oracle_lib))
    for e in devices:                                               # the state write did not disturb the observation
        compare_stacks(chk, e, o, n, "%s after the state write" % game)

    def oracle_step(t):
        head_oracle.agent_step_synthetic(BENCH_ACTION_SEED, t)
        o.agent_step_synthetic(BENCH_ACTION_SEED, t)
        return code_of(o.sync)

    ended, codes, _ = run_blocks(o, head_oracle, devices, stream, WINDOW, BLOCK,
                                 lambda e, t, sp: e.agent_step_synthetic(BENCH_ACTION_SEED, t, stream=sp), oracle_step, chk, game)
    assert_same_end_state(o, devices, n, game)
    # the next call in host form: program order across the caller's stream and the engine's own
    a = synthetic_actions(game, n, WINDOW, seed=BENCH_ACTION_SEED)
    head_oracle.agent_step_synthetic(BENCH_ACTION_SEED, WINDOW)
    rc_o, want = host_step(o, a)
    for e in devices:
        rc, got = host_step(e, a)
        compare_outputs(got, want, "%s host-form step %d" % (game, WINDOW))
        assert rc == rc_o, (game, rc, rc_o)
        if e._agent_ring:
            assert e.agent_ring_head() == head_oracle.agent_ring_head()
        compare_stacks(chk, e, o, n, "%s host-form step %d" % (game, WINDOW))
    share = float(ended.sum()) / n
    print("%s: %d envs, %d of them with a real game over inside %d agent steps (%.1f %%); tbx_sync codes of the blocks %r"
          % (game, n, int(ended.sum()), WINDOW, 100 * share, codes))
    return share


def _engine(game, n, lib, new_plane):
    e = Engine(game, n, lib=lib)
    e.want_plane = new_plane
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("game", GAMES)
def test_gpu_agent_pipeline_at_bench_size_in_bench_form(game, hip_lib, oracle_lib, monkeypatch):
    """bench.py's agent workload -- 65 536 envs, its seeds, every wrapper, tbx_agent_step_synthetic back to back on one caller's
    stream with asynchronous readers queued between the calls -- for both observation forms against ONE oracle run: every env's
    outputs at each of 32 steps, every env's whole stack (rolled; ring read through its head) before step 0 and after every
    fourth step, tbx_sync's code per block, then scalars, sampled state records and the next host-form step.

    First run, Breakout: the rolled stack of 838 of the 65 536 envs differed after steps 0..3, first at env 17, y 75, x 35,
    channel 0 (got 0, want 103: the paddle) -- envs that lost a life inside step(2) of FireResetEnv.reset, whose observation the
    fused kernels took from the buffer a later no-op step had rewritten (test_life_lost_inside_fire_reset_keeps_the_observation_
    of_step_2 below; the oracle alone counts 56 / 20 / 2 / 0 such resets per 4 096 envs in Breakout / SpaceInvaders / Amidar /
    GridWorld inside this window).

    Every env is compared, none sampled.  The oracle's share of envs with a real game over inside the window is asserted against
    EVENT_FLOOR; measured on the oracle alone at 65 536 envs: see EVENTS_SEEN below."""
    from toybox_amd import hip
    monkeypatch.setenv("TBX_ORACLE_THREADS", str(min(16, len(__import__("os").sched_getaffinity(0)))))
    n = BENCH_ENVS
    o, head = _engine(game, n, oracle_lib, 0), _engine(game, 1, oracle_lib, 2)
    devices = [_engine(game, n, hip_lib, 0), _engine(game, n, hip_lib, 2)]
    stream = hip.Stream()
    try:
        share = bench_form_parity(game, n, o, head, devices, stream, oracle_lib, pinned=True)
    finally:
        for e in devices:
            e._lib.tbx_sync(e._h)                                   # (the stream may only go once the engines have forgotten it)
        stream.close()
        for e in devices + [o, head]:
            e.close()
    assert share >= EVENT_FLOOR[game], (game, share)


# envs with a real game over inside the window, seen on the oracle alone with this recipe: at 65 536 envs, at 2 048 envs (GridWorld
# from a fresh reset, no pre-roll needed).  A record of what the floor stands on, not used by any assertion.
EVENTS_SEEN = {"breakout": (42371, 1339), "space_invaders": (9344, 284), "amidar": (3664, 131), "gridworld": (2588, 73)}


@pytest.mark.parametrize("game", GAMES)
def test_bench_form_loop_and_event_floor_on_the_checker(game, oracle_lib):
    """The same loop without a GPU, the CPU checker's ring form standing where the device does, 2 048 envs: the harness itself
    runs in `pytest -m "not gpu"` (readers, codes, ring head, stacks through the ring), and the recipe's event floor holds on
    the oracle's outputs."""
    n = 2048
    o, head = _engine(game, n, oracle_lib, 0), _engine(game, 1, oracle_lib, 2)
    devices = [_engine(game, n, oracle_lib, 2)]
    share = bench_form_parity(game, n, o, head, devices, None, oracle_lib, pinned=False)
    for e in devices + [o, head]:
        e.close()
    assert share >= EVENT_FLOOR[game], (game, share)


@pytest.mark.parametrize("what", ["plane", "reward"])
def test_the_loop_notices_one_wrong_value_in_the_last_env(what, oracle_lib):
    """the harness has teeth: the checker stands where the device does and, behind step 5 of 8, one byte of the last env's newest
    plane (or its reward) is changed as a wrong kernel would leave it.  The plane is found at the block's end, in that env, in the
    channel the ring's head puts it in (a plane written in the block's second step is the third newest by then); the reward
    by the reader queued behind that step."""
    game, n = "gridworld", 130
    o, head, d = _engine(game, n, oracle_lib, 0), _engine(game, 1, oracle_lib, 2), _engine(game, n, oracle_lib, 2)
    for e, mode in ((o, 0), (head, 2), (d, 2)):
        e.seed(BENCH_SEED)
        e.agent_init(new_plane=mode, **BENCH_AGENT)
        e.agent_reset()

    def device_step(e, t, sp):
        e.agent_step_synthetic(BENCH_ACTION_SEED, t, stream=sp)
        if t == 5:
            which = _abi.BUF_AGENT_PLANE if what == "plane" else _abi.BUF_AGENT_REWARD
            ptr, nbytes = e.device_buffer(which)
            last = (C.c_uint8 * 1).from_address(ptr + nbytes - 1)   # (the top byte of the float: 0 becomes 2, +-1 infinite)
            last[0] ^= 0x40

    def oracle_step(t):
        head.agent_step_synthetic(BENCH_ACTION_SEED, t)
        o.agent_step_synthetic(BENCH_ACTION_SEED, t)
        return code_of(o.sync)

    want = r"steps 4\.\.7: frames differ: first at frame j=0 env i=129 y=83 x=83 channel 1 " if what == "plane" else \
        r"steps 4\.\.7 step 5: reward differs in 1 envs, first env 129 "
    with pytest.raises(AssertionError, match=want):
        run_blocks(o, head, [d], None, 8, BLOCK, device_step, oracle_step, FrameChecker((84, 84, 4)), game)
    for e in (o, head, d):
        e.close()


def falling_ball_states(oracle_lib, n):
    """Breakout: n copies of one mid-game donor state (three lives, the ball below the paddle and falling one pixel per frame),
    the ball half a pixel higher from env to env -- so the frame in which the life goes walks through the whole reset
    procedure that the write triggers (the lives fell from 5 to 3: EpisodicLifeEnv reports done, and the reset is a no-op
    step, FIRE, then action 2, four frames each)"""
    rec = donor_records("breakout", oracle_lib)
    falling = np.flatnonzero((rec["lives"] == 3) & (rec["n_balls"] == 1) & (rec["ball_y"][:, 0] > rec["paddle_y"] + 4) & (rec["ball_vy"][:, 0] > 0.9))
    out = rec[np.full(n, falling[0])]
    out["ball_y"][:, 0] = 160.0 - 0.5 * np.arange(n)
    return out


@pytest.fixture(params=["oracle", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request, oracle_lib):
    if request.param == "oracle":
        return oracle_lib
    return request.getfixturevalue("hip_lib")


@pytest.mark.parametrize("new_plane", [0, 2])
def test_life_lost_inside_fire_reset_keeps_the_observation_of_step_2(new_plane, lib, oracle_lib):
    """What the bench-size case found in Breakout (838 of 65 536 envs, first at step 0, env 17, y 75, x 35): FireResetEnv.reset
    returns the observation of its step(2) even when that step lost a life and EpisodicLifeEnv's reset then ran a no-op STEP,
    which rewrites MaxAndSkipEnv's two-frame buffer (atari_wrappers.py:149-152, :186-187).  The fused observation kernel read the
    rewritten buffer.  Natural play cannot get there (a ball served by FIRE does not leave the screen eight frames later); a
    state written between agent steps can.  80 envs whose ball leaves the screen in consecutive half-frames: every env's stack
    against the oracle's over 6 steps, and on the oracle alone the condition that the lives fell inside the reset procedure in
    at least 16 envs (eight frames' worth of the forty the heights span)."""
    n = 80
    o, head, d = _engine("breakout", n, oracle_lib, 0), _engine("breakout", 1, oracle_lib, 2), _engine("breakout", n, lib, new_plane)
    for e, mode in ((o, 0), (head, 2), (d, new_plane)):
        e.seed(BENCH_SEED)
        e.agent_init(new_plane=mode, **BENCH_AGENT)
        e.agent_reset()
    rec = falling_ball_states(oracle_lib, n)
    for e in (o, d):
        e.set_states_np(0, rec)

    def oracle_step(t):
        head.agent_step_synthetic(BENCH_ACTION_SEED, t)
        o.agent_step_synthetic(BENCH_ACTION_SEED, t)
        rc = code_of(o.sync)
        if t == 0:
            done = read_buffer(o, _abi.BUF_AGENT_DONE, (n,))
            lost = (done != 0) & (o.scalars()[1] == 2)              # done by the write's drop in lives, and a life went since
            assert lost.sum() >= 16, lost.sum()
        return rc

    run_blocks(o, head, [d], None, 6, 1, lambda e, t, sp: e.agent_step_synthetic(BENCH_ACTION_SEED, t, stream=sp), oracle_step,
               FrameChecker((84, 84, 4)), "breakout falling balls")
    assert_same_end_state(o, [d], n, "breakout falling balls")
    for e in (o, head, d):
        e.close()


# ================================================================ B. tbx_agent_step_device

DEV_ENVS, DEV_STEPS, DEV_BLOCK = 1100, 120, 8     # 1 100: ragged for the 64-env thread form and for 256-thread blocks
DEV_AGENT = dict(skip=4, out_h=84, out_w=84, stack=4, clip_reward=True, episodic_life=True, fire_reset=True, noop_max=7, noop_seed=17)
DEV_SEED, DEV_ACTION_SEED = 4242, 21
# ids no game knows: the first one past the table, a negative one, and two beyond 16 bits whose low halves are legal ids (1 = FIRE,
# 0 = NOOP: an engine that narrowed the id would play them, and would not report them)
ILLEGAL_IDS = (18, -1, 65537, -65536)


def device_actions(game, n, steps):
    """int32[steps][n]: synthetic actions; the rows t % 16 == 5 and the last row carry the illegal ids, in envs that move with t
    (so every second block of 8 reports TBX_E_ACTION, the others nothing)"""
    a = np.stack([synthetic_actions(game, n, t, seed=DEV_ACTION_SEED) for t in range(steps)]).astype(np.int32)
    for t in [t for t in range(steps) if t % 16 == 5] + [steps - 1]:
        envs = [(t * 37) % n, n - 1, 64, (t * 37 + 255) % n]       # (a moving env, the last one, both sides of a wave's edge)
        assert len(set(envs)) == len(ILLEGAL_IDS)
        a[t, envs] = ILLEGAL_IDS
    return a


def noop_where_illegal(actions):
    """every ALE id 0..17 is an id of the ABI (envs/atari/constants.py:16-35); anything else is played as NOOP"""
    return np.where((actions >= 0) & (actions < 18), actions, 0).astype(np.int32)


def park_enemies_on_last_lives(engines):
    """Amidar: envs 0..7 get two lives, every enemy parked on the player and a jump that runs out 1..8 frames from now, the enemies
    coming back on the player's start tile (tests/test_preproc.py, test_game_over_inside_the_episodic_life_noop_step): the life
    goes, EpisodicLifeEnv's no-op step costs the last one, and the step after that is a step on an env that needs a reset"""
    cd = codec("amidar")
    for i in range(8):
        st = cd.state_from_json(amidar_edit_last_lives(cd.state_to_json(engines[0].get_state(i)), lives=2, jump_timer=i + 1,
                                                       perimeter_from_start=True))
        for e in engines:
            e.set_state(i, st)


def device_action_parity(game, o, head_oracle, dev, stream, upload, pinned):
    """part B for engines that exist: `upload(actions) -> address` puts int32[K][n] where the engine under test reads actions.
    Returns the blocks' step codes of the oracle."""
    n = DEV_ENVS
    chk = FrameChecker((84, 84, 4), pinned=pinned)
    for e, mode in ((o, 0), (head_oracle, 2), (dev, dev.want_plane)):
        e.seed(DEV_SEED)
        e.agent_init(new_plane=mode, **DEV_AGENT)
        e.agent_reset()
    if game == "amidar":
        park_enemies_on_last_lives([o, dev])
    actions = device_actions(game, n, DEV_STEPS)
    base = upload(actions)

    def oracle_step(t):
        head_oracle.agent_step(noop_where_illegal(actions[t, :1]), tolerate_needs_reset=True)
        rc, _ = host_step(o, actions[t])
        return rc

    _, codes, step_codes = run_blocks(o, head_oracle, [dev], stream, DEV_STEPS, DEV_BLOCK,
                                      lambda e, t, sp: e.agent_step_device(base + t * n * 4, stream=sp), oracle_step, chk,
                                      "%s device actions" % game)
    assert_same_end_state(o, [dev], n, game)
    return codes, step_codes


def assert_codes_reached(game, codes, step_codes):
    """conditions on the inputs, from the oracle's codes alone"""
    assert _abi.E_ACTION in codes and _abi.OK in codes, (game, codes)
    if game == "amidar":                                            # the precedence is exercised: one block holds both
        assert any(_abi.E_ACTION in rcs and _abi.E_NEEDS_RESET in rcs for rcs in step_codes), (game, step_codes)


DEV_CASES = [(g, p, 0) for g in GAMES for p in (0, 2)] + [("amidar", 0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("game,new_plane,step_form", DEV_CASES)
def test_gpu_agent_step_device_equals_oracle(game, new_plane, step_form, hip_lib, oracle_lib):
    """tbx_agent_step_device: 120 agent steps of 1 100 envs with every wrapper on, the actions of all steps uploaded once as
    int32[K][n] and row t handed to step t, back to back on a caller's stream with readers queued between the calls; outputs of
    every env at every step and stacks every 8 steps equal the oracle's tbx_agent_step on the same rows.  Rows with illegal ids
    (18, -1, +-65 536 and beyond) play NOOP in those envs and the block's tbx_sync reports TBX_E_ACTION -- TBX_E_NEEDS_RESET where
    the block also stepped an env that needed a reset (Amidar: built in, see park_enemies_on_last_lives).  step_form = 1: Amidar's
    thread-per-env agent kernel, which a batch this small does not choose by itself."""
    from toybox_amd import hip
    n = DEV_ENVS
    o, head, g = _engine(game, n, oracle_lib, 0), _engine(game, 1, oracle_lib, 2), _engine(game, n, hip_lib, new_plane)
    if step_form:
        g.set_option(_abi.OPT_STEP_FORM, step_form)
    stream = hip.Stream()
    dev_mem = []

    def upload(actions):
        dev_mem.append(hip.malloc(actions.nbytes))
        hip.memcpy_htod(dev_mem[0], actions, actions.nbytes)
        return dev_mem[0]

    try:
        codes, step_codes = device_action_parity(game, o, head, g, stream, upload, pinned=True)
    finally:
        g._lib.tbx_sync(g._h)
        stream.close()
        for e in (g, o, head):
            e.close()
        for p in dev_mem:
            hip.free(p)
    assert_codes_reached(game, codes, step_codes)


@pytest.mark.parametrize("game", ["amidar"])
def test_agent_step_device_loop_on_the_checker(game, oracle_lib):
    """the same loop with the CPU checker's ring form in the device's place (its tbx_agent_step_device reads host memory): the
    harness and the conditions on the inputs -- blocks with TBX_E_ACTION, blocks without, and in Amidar a block with both codes"""
    n = DEV_ENVS
    o, head, d = _engine(game, n, oracle_lib, 0), _engine(game, 1, oracle_lib, 2), _engine(game, n, oracle_lib, 2)
    keep = []

    def upload(actions):
        keep.append(np.ascontiguousarray(actions))
        return keep[0].ctypes.data

    codes, step_codes = device_action_parity(game, o, head, d, None, upload, pinned=False)
    for e in (o, head, d):
        e.close()
    assert_codes_reached(game, codes, step_codes)


@pytest.mark.parametrize("game", GAMES)
def test_agent_step_device_call_contract(game, lib):
    """tbx_agent_step_device / tbx_agent_step_synthetic before tbx_agent_init, and a NULL action pointer after it: TBX_E_INVALID
    on both libraries, and the engine goes on working"""
    n = 70
    e = Engine(game, n, lib=lib)
    e.seed(1)
    a = synthetic_actions(game, n, 0)
    if engine_is_oracle(e):
        ptr, release = a.ctypes.data, lambda: None
    else:
        from toybox_amd import hip
        ptr = hip.malloc(a.nbytes)
        hip.memcpy_htod(ptr, a, a.nbytes)
        release = lambda: hip.free(ptr)
    try:
        assert code_of(lambda: e.agent_step_device(ptr)) == _abi.E_INVALID
        assert code_of(lambda: e.agent_step_synthetic(1337, 0)) == _abi.E_INVALID
        e.agent_init(**DEV_AGENT)
        e.agent_reset()
        assert code_of(lambda: e.agent_step_device(0)) == _abi.E_INVALID
        assert e._lib.tbx_agent_step_device(None, C.c_void_p(ptr), None) == _abi.E_INVALID
        e.agent_step_device(ptr)                                    # a good call after the refused ones
        assert code_of(e.sync) == _abi.OK
        reward = read_buffer(e, _abi.BUF_AGENT_REWARD, (n,), np.float32)
        assert np.isfinite(reward).all()
    finally:
        e.sync()
        e.close()
        release()
