"""Checkpoints on the device (TBX_EDIT_CHECKPOINT_SLOTS / _SAVE / _RESTORE, TBX_QUERY_CHECKPOINT_VALID through tbx_edit,
tbx_edit_device and tbx_reduce; Engine.checkpoint_*; the VecEnv adapters) against the REPLAY ACROSS TIME of
tests/checkpoint_replay.py: restored envs must be a fresh CPU-checker engine's, made and driven to the SAVE step the way the
saved rows were, the others the original batch's at the current step.  Everything is compared byte for byte; every test here
fails on a library without the ops ("unknown edit", "unknown query") or a package without the methods."""
import numpy as np
import pytest

from checkpoint_replay import Solo, Twin, mixed_actions, pick_rows, replay_to, restore_map
from fork_replay import Agent, Raw, fork_maps, sim_rngs, snapshot, states_bytes
from fork_replay import assert_rows_equal as assert_rows, assert_snapshot_equal as assert_snapshot
from support import read_buffer, splitmix64
from test_gpu_fork import _pick_moment
from toybox_amd import Engine, ToyboxAmdError, _abi
from toybox_amd.engine import checkpoint_args

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]


def _device_edit(g, op, args, mask=None):
    """tbx_edit_device with one device row per env and a device mask on a stream of the caller's"""
    from toybox_amd import hip
    n = g.n_envs
    rows = np.ascontiguousarray(np.broadcast_to(np.asarray(args, np.float64).reshape(-1, np.shape(args)[-1]), (n, np.shape(args)[-1])))
    m = np.ascontiguousarray(np.ones(n, np.uint8) if mask is None else np.asarray(mask, np.uint8))
    d_rows, d_mask = hip.malloc(rows.nbytes), hip.malloc(n)
    s = hip.Stream()
    try:
        hip.memcpy_htod(d_rows, rows, rows.nbytes)
        hip.memcpy_htod(d_mask, m, n)
        g.edit_device(op, mask_ptr=d_mask, stream=s.ptr, per_env_ptr=d_rows, n_args=rows.shape[1])
        s.synchronize()
    finally:
        g.sync()            # the engine forgets the stream: one named in a call has to outlive the next call or tbx_sync (toybox_amd.h)
        hip.free(d_rows); hip.free(d_mask)
        s.close()


def _save(g, form, slot, mask=None):
    if form == "host":
        g.checkpoint_save(slot, mask=mask)
    else:
        _device_edit(g, _abi.EDIT_CHECKPOINT_SAVE, np.reshape(checkpoint_args(g.n_envs, slot), (-1, 1)), mask)


def _restore(g, form, slot, rows=None, mask=None, salt=None):
    if form == "host":
        g.checkpoint_restore(slot, rows=rows, mask=mask, salt=salt)
    else:
        a = checkpoint_args(g.n_envs, slot, rows, salt)
        _device_edit(g, _abi.EDIT_CHECKPOINT_RESTORE, np.reshape(a, (-1, np.shape(a)[-1])), mask)


# ---------------------------------------------------------------- 1. what save and restore mean, on the state records

@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("n", [1, 5, 700])
@pytest.mark.parametrize("game", GAMES)
def test_state_level_meaning(game, n, form, hip_lib):
    """slot 0 saved at step 20, slot 1 (odd envs only) at step 45, slot 0 restored through a random map with repeats: records and
    simulator RNG of every selected env are the saved row's as read from the device at step 20, the others untouched"""
    case = Raw(game, n)
    g = case.make(hip_lib)
    g.checkpoint_slots(2)
    assert np.array_equal(g.checkpoint_valid(0), np.zeros(n, np.int8)), "a fresh store is empty"
    case.run(g, 0, 20)
    at20 = snapshot(g)
    _save(g, form, 0)
    assert_snapshot(snapshot(g), at20, "a save changed the live engine")
    case.run(g, 20, 45)
    at45 = snapshot(g)
    odd = np.arange(n) % 2 == 1
    _save(g, form, 1, mask=odd)
    src, mask = fork_maps(n, seed=n)["random_repeats"]
    rows, eff = restore_map(n, src, mask)
    _restore(g, form, 0, rows=rows, mask=mask)
    want = tuple(pick_rows(mask, x[eff], y) for x, y in zip(at20, at45))
    assert_snapshot(snapshot(g), want, "%s n=%d %s" % (game, n, form))
    assert np.array_equal(g.checkpoint_valid(0), np.ones(n, np.int8))
    assert np.array_equal(g.checkpoint_valid(1), odd.astype(np.int8))
    assert np.array_equal(g.checkpoint_valid(1, rows=n - 1 - np.arange(n)), odd[::-1].astype(np.int8))
    assert np.array_equal(g.checkpoint_valid(2), np.full(n, -1, np.int8))
    assert g.reduce_width(_abi.QUERY_CHECKPOINT_VALID) == 1
    g.close()


# ---------------------------------------------------------------- 2. the raw layer continues like the replay

def _gpu_outputs(g, n):
    return (read_buffer(g, _abi.BUF_REWARD, (n,), np.int32), read_buffer(g, _abi.BUF_DONE, (n,), np.uint8).astype(bool),
            read_buffer(g, _abi.BUF_LIVES, (n,), np.int32), read_buffer(g, _abi.BUF_SCORE, (n,), np.int32))


def _advance(case, g, x, loop, t, channels, what):
    """one unit of loop form `loop` (1 frame, a chunk of 4) on the device engine and on the expected batch x (Solo / Twin):
    frames and step outputs compared; -> the next frame number"""
    n = case.n
    shape = (n, g.height, g.width, channels)
    if loop == "step":
        rg, rx = g.step(case.actions(t), auto_reset=True), x.step(case.actions(t))
        for k, (p, q) in enumerate(zip(rg, rx)):
            assert np.array_equal(p, q), "%s: output %d differs at frame %d" % (what, k, t)
        if t % 5 == 0:
            assert np.array_equal(g.render(channels), x.render(channels)), "%s: frame %d" % (what, t)
        return t + 1
    if loop == "render_step":
        g.render_step_synthetic(case.action_seed, t, channels=channels, auto_reset=True)
        assert np.array_equal(read_buffer(g, _abi.BUF_FRAME, shape), x.render(channels)), "%s: frame %d" % (what, t)
        rx = x.step(case.actions(t))
        for k, (p, q) in enumerate(zip(_gpu_outputs(g, n), rx)):
            assert np.array_equal(p, q), "%s: output %d differs at frame %d" % (what, k, t)
        return t + 1
    g.rollout_synthetic(case.action_seed, t, 4, channels=channels, auto_reset=True)
    frames = read_buffer(g, _abi.BUF_ROLLOUT_FRAMES, (4,) + shape)
    for j in range(4):
        assert np.array_equal(frames[j], x.render(channels)), "%s: frame %d of the chunk at %d" % (what, j, t)
        rx = x.step(case.actions(t + j))
    for k, (p, q) in enumerate(zip(_gpu_outputs(g, n), rx)):
        assert np.array_equal(p, q), "%s: output %d differs after the chunk at %d" % (what, k, t)
    return t + 4


def _raw_case(game, n, loop, hip_lib, oracle_lib, t_s=120, t_r=160, T2=24, channels=3, form="host", options=(), lead=8, frames=True, active=None):
    """G and O to t_s (the last `lead` frames in loop form `loop`), save, on to t_r in that form, restore a masked random map
    with repeats, replay O2 = the saved rows at t_s, then T2 more frames of G against Twin(O2, O)"""
    case = Raw(game, n)
    src, mask = fork_maps(n, seed=11)["random_repeats"]
    rows, eff = restore_map(n, src, mask)
    g, o = case.make(hip_lib), case.make(oracle_lib)
    for opt, val in options:
        g.set_option(opt, val)
    g.checkpoint_slots(1)
    what = "%s n=%d %s %s" % (game, n, loop, form)
    case.run(o, 0, t_s - lead)
    for t in range(t_s - lead):
        g.step_synthetic(case.action_seed, t, auto_reset=True)
    t = t_s - lead
    step = _advance if frames else _advance_outputs
    while t < t_s:
        t = step(case, g, Solo(o), loop, t, channels, what + " before the save")
    records = g.get_option(_abi.OPT_RECORDS_ACTIVE)
    if active is not None:
        assert g.get_option(active) == 1, "the overlapped loop form is not in force: the case does not test what it is meant to"
    if loop != "step" and game in ("breakout", "space_invaders"):
        assert records == 1, "the engine is not on its record path: the case does not test what it is meant to"
    _save(g, form, 0)
    assert g.get_option(_abi.OPT_RECORDS_ACTIVE) == records, "a save took the engine off its record path"
    while t < t_r:                                          # the frames after the save are the checker's: nothing was marked stale
        t = step(case, g, Solo(o), loop, t, channels, what + " after the save")
    _restore(g, form, 0, rows=rows, mask=mask)
    o2 = replay_to(case, oracle_lib, eff, t_s)
    x = Twin(o2, o, mask)
    assert_snapshot(snapshot(g), x.snapshot(), what + " right after the restore")
    while t < t_r + T2:
        t = step(case, g, x, loop, t, channels, what + " after the restore")
    assert_snapshot(snapshot(g), x.snapshot(), what + " at the end")
    g.close(); o.close(); o2.close()


def _advance_outputs(case, g, x, loop, t, channels, what):
    """_advance for batches whose frames are not compared: step outputs only"""
    assert loop == "step"
    rg, rx = g.step(case.actions(t), auto_reset=True), x.step(case.actions(t))
    for k, (p, q) in enumerate(zip(rg, rx)):
        assert np.array_equal(p, q), "%s: output %d differs at frame %d" % (what, k, t)
    return t + 1


@pytest.mark.parametrize("loop", ["step", "render_step", "rollout"])
@pytest.mark.parametrize("game", GAMES)
def test_raw_rollout_after_restore_equals_replay(game, loop, hip_lib, oracle_lib):
    """48 envs, lives edited to 1, auto-reset on: every env's outputs and frames after the save and after the restore;
    Breakout's and SpaceInvaders' record rasterisers must paint the restored state, not the records the last step wrote"""
    _raw_case(game, 48, loop, hip_lib, oracle_lib)


@pytest.mark.parametrize("loop", ["render_step", "rollout"])
@pytest.mark.parametrize("game", ["breakout", "space_invaders"])
def test_save_inside_an_overlapped_loop_form(game, loop, hip_lib, oracle_lib):
    """256 envs: rollout chunks / overlapped fused launches are in force when the save and the restore come (device forms, a
    stream of the caller's); TBX_OPT_RECORDS_ACTIVE stays 1 over the save and the frames that follow are the checker's"""
    _raw_case(game, 256, loop, hip_lib, oracle_lib, t_s=40, t_r=48, T2=8, form="device", lead=8,
              options=((_abi.OPT_FUSED_OVERLAP, _abi.FUSED_OVERLAP_ON),) if loop == "render_step" else (),
              active=_abi.OPT_ROLLOUT_CHUNKS_ACTIVE if loop == "rollout" else _abi.OPT_FUSED_OVERLAP_ACTIVE if game == "breakout" else None)


# ---------------------------------------------------------------- 3. the agent layer

AGENT_FORMS = {"rolled": {}, "new_plane_1": {"new_plane": 1}, "ring": {"new_plane": 2}, "stack_fill": {"stack_fill": 1}}


def _agent_case(game, hip_lib, oracle_lib, n=24, t_s=40, t_r=63, T2=60, src=None, sel=None, generic=False, need_done=True, **kw):
    case = Agent(game, n, **kw)
    if src is None:
        src = fork_maps(n, seed=5)["random_repeats"][0]
        sel = np.arange(n) % 3 != 0                         # a masked two thirds, through a map with repeats
    rows, eff = restore_map(n, src, sel)
    g = case.make(hip_lib, options=((_abi.OPT_AGENT_GENERIC, 1),) if generic else ())
    g.checkpoint_slots(1)                                   # (after agent_init: the store belongs to the arrays that exist now)
    o = case.make(oracle_lib)
    what = "%s agent layer %r generic=%s (saved at %d, restored at %d)" % (game, kw, generic, t_s, t_r)
    assert_rows(case.run(g, 0, t_s), case.run(o, 0, t_s), what + " before the save")
    g.checkpoint_save(0)
    assert_rows(case.run(g, t_s, t_r), case.run(o, t_s, t_r), what + " after the save")
    g.checkpoint_restore(0, rows=rows, mask=sel)
    o2 = replay_to(case, oracle_lib, eff, t_s)
    x = Twin(o2, o, sel)
    assert np.array_equal(case.observation(g), x.observation(case)), what + ": observation right after the restore"
    assert_snapshot(snapshot(g), x.snapshot(), what + " right after the restore")
    acts = [mixed_actions(case, sel, eff, t_s, t_r, k) for k in range(T2)]
    want = x.agent_rows(case, acts)
    assert_rows(case.rows(g, acts), want, what)
    assert_snapshot(snapshot(g), x.snapshot(), what + " at the end")
    if need_done:
        ended, done = np.stack([r[3] for r in want]), np.stack([r[2] for r in want])
        assert done.any() and (ended.any() or game == "amidar"), "no episode ended after the restore"   # (Amidar's games outlast the run)
    g.close(); o.close(); o2.close()


@pytest.mark.parametrize("form", list(AGENT_FORMS) + ["generic"])
@pytest.mark.parametrize("game", GAMES)
def test_agent_layer_after_restore_equals_replay(game, form, hip_lib, oracle_lib):
    """every wrapper on, 24 envs, saved at agent step 40, restored at 63 -- 23 steps on, so the plane ring's head stands 3 slots
    from where it stood at the save (a multiple of 4 would hide a byte-for-byte copy of the ring): the observation right after,
    then 60 agent steps of observation, reward, done and episode record of every env"""
    _agent_case(game, hip_lib, oracle_lib, generic=form == "generic", **AGENT_FORMS.get(form, {}))


# ---------------------------------------------------------------- 4. moments

@pytest.mark.parametrize("moment", ["life", "game"])
@pytest.mark.parametrize("game", GAMES)
def test_agent_layer_checkpoint_moments(game, moment, hip_lib, oracle_lib):
    """the save is taken on the step after an env lost a life under EpisodicLifeEnv / on the step its game ended; that env's
    cell is restored 30 steps later into a third of the batch"""
    if game == "gridworld" and moment == "life":
        moment = "game"                                     # GridWorld has no lives: its only `done` is the game's end
    n = 24
    kw = {"new_plane": 2} if moment == "game" else {}
    case = Agent(game, n, **kw)
    o = case.make(oracle_lib)
    t_s, star = _pick_moment(case.run(o, 0, 130), moment, 40)
    o.close()
    sel = np.arange(n) % 3 == 1
    _agent_case(game, hip_lib, oracle_lib, n=n, t_s=t_s, t_r=t_s + 30, T2=40, src=np.full(n, star), sel=sel, need_done=False, **kw)


# ---------------------------------------------------------------- 5. a strided grid, many rows per block

def test_breakout_8200_envs_strided_rows_grid(hip_lib, oracle_lib):
    """the rows kernel's grid is capped at 2 048 blocks x 4 waves = 8 192 envs: 8 200 is the smallest batch that strides"""
    _raw_case("breakout", 8200, "step", hip_lib, oracle_lib, t_s=20, t_r=30, T2=10, lead=2, frames=False)


def test_space_invaders_agent_1024_envs(hip_lib, oracle_lib):
    """1 024 SpaceInvaders envs x 40 + 40 agent steps: several env rows per block in the stack copy"""
    _agent_case("space_invaders", hip_lib, oracle_lib, n=1024, t_s=17, t_r=40, T2=40, need_done=False)


# ---------------------------------------------------------------- 6. two slots in one call

@pytest.mark.parametrize("game", GAMES)
def test_two_slots_in_one_restore(game, hip_lib, oracle_lib):
    """slot 0 saved at step 20, slot 1 at step 35; at step 50 ONE restore with per-env {slot, row}: evens from slot 0, odds from
    slot 1, rows reversed -- each half equals its replay, right away and over 30 more steps"""
    n = 32
    case = Raw(game, n)
    g = case.make(hip_lib)
    g.checkpoint_slots(2)
    case.run(g, 0, 20); g.checkpoint_save(0)
    case.run(g, 20, 35); g.checkpoint_save(1)
    case.run(g, 35, 50)
    even = np.arange(n) % 2 == 0
    rev = n - 1 - np.arange(n)
    g.checkpoint_restore(np.where(even, 0, 1), rows=rev)
    x = Twin(replay_to(case, oracle_lib, rev, 20), replay_to(case, oracle_lib, rev, 35), even)
    assert_snapshot(snapshot(g), x.snapshot(), game + " right after the restore")
    for t in range(50, 80):
        for k, (p, q) in enumerate(zip(g.step(case.actions(t), auto_reset=True), x.step(case.actions(t)))):
            assert np.array_equal(p, q), "%s: output %d differs at frame %d" % (game, k, t)
    assert_snapshot(snapshot(g), x.snapshot(), game + " at the end")
    g.close(); x.a.close(); x.b.close()


# ---------------------------------------------------------------- 7. errors change nothing

@pytest.mark.parametrize("game", GAMES)
def test_errors_change_nothing(game, hip_lib):
    n = 16
    case = Raw(game, n)
    g = case.make(hip_lib)
    case.run(g, 0, 10)
    before = snapshot(g)

    def refused(call, code=_abi.E_INVALID, names=None):
        with pytest.raises(ToyboxAmdError) as ei:
            call()
        assert ei.value.code == code, str(ei.value)
        if names is not None:
            assert names in str(ei.value), str(ei.value)
        assert_snapshot(snapshot(g), before, game + " after a refused call")

    refused(lambda: g.checkpoint_save(0))                   # no store
    refused(lambda: g.checkpoint_restore(0))
    assert np.array_equal(g.checkpoint_valid(0), np.full(n, -1, np.int8))
    # CHECKPOINT_SLOTS: host form only, no mask, no per-env rows
    refused(lambda: g.edit(_abi.EDIT_CHECKPOINT_SLOTS, [2], mask=np.ones(n, bool)))
    refused(lambda: g.edit(_abi.EDIT_CHECKPOINT_SLOTS, np.full((n, 1), 2.0)))
    refused(lambda: g.edit_device(_abi.EDIT_CHECKPOINT_SLOTS, [2]))
    g.sync()
    assert np.array_equal(g.checkpoint_valid(0), np.full(n, -1, np.int8)), "a refused CHECKPOINT_SLOTS made a store"
    g.checkpoint_slots(2)
    slots = np.zeros(n, np.int64)
    slots[5] = 2
    refused(lambda: g.checkpoint_save(slots), names="env 5")            # slot out of range
    slots[5] = -1
    refused(lambda: g.checkpoint_save(slots), names="env 5")
    assert np.array_equal(g.checkpoint_valid(0), np.zeros(n, np.int8)), "a refused save filled cells"
    refused(lambda: g.checkpoint_restore(0), names="env 0")             # empty cells
    g.checkpoint_save(0, mask=np.arange(n) != 3)
    refused(lambda: g.checkpoint_restore(0), names="env 3")             # one empty cell
    rows = np.arange(n)[::-1].copy()
    rows[7] = n
    refused(lambda: g.checkpoint_restore(0, rows=rows), names="env 7")  # row out of range (n - 1 - 7 != 3: not the empty cell)
    rows[7] = -2
    refused(lambda: g.checkpoint_restore(0, rows=rows), names="env 7")
    mask = np.ones(n, bool)
    mask[[7, n - 1 - 3]] = False
    g.checkpoint_restore(0, rows=rows, mask=mask)           # the same rows in unselected envs are accepted
    g.close()


@pytest.mark.parametrize("game", GAMES)
def test_device_form_leaves_bad_rows_untouched(game, hip_lib):
    """device forms cannot report: two bad rows among good ones (a slot and a row outside the store) and an empty cell are left
    untouched, the good ones go through, and tbx_sync reports nothing"""
    n = 16
    case = Raw(game, n)
    g = case.make(hip_lib)
    g.checkpoint_slots(1)
    case.run(g, 0, 10)
    at10 = snapshot(g)
    slots = np.zeros(n, np.int64)
    slots[2] = 1                                            # no such slot: env 2 is not saved
    _device_edit(g, _abi.EDIT_CHECKPOINT_SAVE, slots.reshape(-1, 1))
    assert np.array_equal(g.checkpoint_valid(0), (np.arange(n) != 2).astype(np.int8))
    case.run(g, 10, 25)
    at25 = snapshot(g)
    rows = np.arange(n)[::-1].copy()                        # env 13 names the empty cell (0, 2)
    rows[4] = n
    slots = np.zeros(n, np.int64)
    slots[9] = -3
    _device_edit(g, _abi.EDIT_CHECKPOINT_RESTORE, np.stack([slots, rows], axis=1))
    g.sync()                                                # raises if the engine's error word was set
    good = ~np.isin(np.arange(n), [4, 9, 13])
    eff = np.where(good, rows, 0)
    want = tuple(pick_rows(good, x[eff], y) for x, y in zip(at10, at25))
    assert_snapshot(snapshot(g), want, game + " device form with bad rows")
    g.close()


# ---------------------------------------------------------------- 8. the store belongs to the arrays it was made for

def _tweak_custom_brick(e, env):
    st = e.get_state(env)
    st.bricks[3].x, st.bricks[3].w = 30.5, 20.0
    st.bricks[17].points = 50
    e.set_state(env, st)


def test_signature_breakout_custom_brick_mode(hip_lib, oracle_lib):
    n, env = 24, 7
    case = Raw("breakout", n)
    g, o = case.make(hip_lib), case.make(oracle_lib)
    g.checkpoint_slots(1)
    case.run(g, 0, 30); case.run(o, 0, 30)
    g.checkpoint_save(0)
    _tweak_custom_brick(g, env); _tweak_custom_brick(o, env)     # the engine leaves the canonical wall: a per-env brick table appears
    before = snapshot(g)
    for call in (lambda: g.checkpoint_restore(0), lambda: g.checkpoint_save(0)):
        with pytest.raises(ToyboxAmdError) as ei:
            call()
        assert ei.value.code == _abi.E_UNSUPPORTED, str(ei.value)
        assert_snapshot(snapshot(g), before, "a refused call changed the engine")
    assert np.array_equal(g.checkpoint_valid(0), np.ones(n, np.int8))
    g.checkpoint_slots(1)                                   # a new store, for the arrays of the custom mode
    assert np.array_equal(g.checkpoint_valid(0), np.zeros(n, np.int8))
    g.checkpoint_save(0)
    case.run(g, 30, 55); case.run(o, 30, 55)
    sel = np.arange(n) % 4 == 1                             # the written env is the row of a quarter of the batch
    rows, eff = restore_map(n, np.full(n, env), sel)
    g.checkpoint_restore(0, rows=rows, mask=sel)
    o2 = case.make(oracle_lib, eff)
    case.run(o2, 0, 30, eff)
    for i in np.flatnonzero(eff == env):
        _tweak_custom_brick(o2, int(i))
    x = Twin(o2, o, sel)
    assert_snapshot(snapshot(g), x.snapshot(), "custom mode right after the restore")
    for t in range(55, 115):
        for k, (p, q) in enumerate(zip(g.step(case.actions(t), auto_reset=True), x.step(case.actions(t)))):
            assert np.array_equal(p, q), "custom mode: output %d differs at frame %d" % (k, t)
        if t % 10 == 0:
            assert np.array_equal(g.render(3), x.render(3)), "custom mode: frame %d" % t
    assert_snapshot(snapshot(g), x.snapshot(), "custom mode at the end")
    g.close(); o.close(); o2.close()


@pytest.mark.parametrize("game", GAMES)
def test_signature_agent_init_after_the_store(game, hip_lib):
    n = 8
    g = Engine(game, n, lib=hip_lib)
    g.seed_array(np.arange(n, dtype=np.uint32) + 5)
    g.new_game()
    g.checkpoint_slots(1)
    g.checkpoint_save(0)
    g.agent_init(skip=4, stack=4)
    g.agent_reset()
    before = snapshot(g)
    for call in (lambda: g.checkpoint_restore(0), lambda: g.checkpoint_save(0)):
        with pytest.raises(ToyboxAmdError) as ei:
            call()
        assert ei.value.code == _abi.E_UNSUPPORTED, str(ei.value)
        assert_snapshot(snapshot(g), before, "a refused call changed the engine")
    g.checkpoint_slots(1)
    g.checkpoint_save(0)
    g.checkpoint_restore(0)
    assert_snapshot(snapshot(g), before, "a restore of what was just saved")
    g.agent_init(skip=4, stack=4, new_plane=2)              # again, with another form of the observation
    with pytest.raises(ToyboxAmdError) as ei:
        g.checkpoint_restore(0)
    assert ei.value.code == _abi.E_UNSUPPORTED
    g.close()


# ---------------------------------------------------------------- 9. salt

@pytest.mark.parametrize("game", GAMES)
def test_salt(game, hip_lib):
    n = 64
    case = Raw(game, n)
    g = case.make(hip_lib)
    g.checkpoint_slots(1)
    case.run(g, 0, 50)
    saved = snapshot(g)
    g.checkpoint_save(0)
    case.run(g, 50, 60)
    src, mask = fork_maps(n, seed=2)["random_repeats"]
    rows, eff = restore_map(n, src, mask)
    has_rand = game != "gridworld"

    def expect(now, salts):
        st, rng = pick_rows(mask, saved[0][eff], now[0]).copy(), pick_rows(mask, saved[1][eff], now[1]).copy()
        for i in np.flatnonzero(mask & (salts != 0)):
            s = np.uint64(salts[i])
            rng[i] = splitmix64(rng[i] ^ s)
            if has_rand:
                st[i, :16] = splitmix64(st[i, :16].view(np.uint64) ^ s).view(np.uint8)
        return st, rng

    now = snapshot(g)
    g.checkpoint_restore(0, rows=rows, mask=mask)           # no salt and salt 0: the plain restore
    plain = snapshot(g)
    assert_snapshot(plain, expect(now, np.zeros(n, np.uint64)), game + " no salt")
    g.checkpoint_restore(0, rows=rows, mask=mask, salt=0)
    assert_snapshot(snapshot(g), plain, game + " salt 0")
    g.checkpoint_restore(0, rows=rows, mask=mask, salt=0xDEADBEEF)
    assert_snapshot(snapshot(g), expect(plain, np.full(n, 0xDEADBEEF, np.uint64)), game + " one salt")
    salts = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(2 ** 32)
    _restore(g, "device", 0, rows=rows, mask=mask, salt=salts)
    assert_snapshot(snapshot(g), expect(plain, salts), game + " per-env salts, device form")
    g.checkpoint_restore(0, mask=mask, salt=77)             # a salt without rows: the env's own row
    own = tuple(pick_rows(mask, x, y) for x, y in zip(saved, plain))
    st, rng = own[0].copy(), own[1].copy()
    for i in np.flatnonzero(mask):
        rng[i] = splitmix64(rng[i] ^ np.uint64(77))
        if has_rand:
            st[i, :16] = splitmix64(st[i, :16].view(np.uint64) ^ np.uint64(77)).view(np.uint8)
    assert_snapshot(snapshot(g), (st, rng), game + " salt without rows")
    g.close()


def test_two_salts_diverge(hip_lib):
    """two restores of one cell with different salts play the same actions and part ways within 200 frames (SpaceInvaders, 64
    envs: the enemies' shots are drawn from the game's own RNG); the RNG words themselves, bytes 0 .. 15 of a record, are left
    out of the comparison"""
    n, game = 64, "space_invaders"
    case = Raw(game, n)
    ends = []
    for salt in (1, 2):
        g = case.make(hip_lib)
        g.checkpoint_slots(1)
        case.run(g, 0, 50)
        g.checkpoint_save(0)
        g.checkpoint_restore(0, salt=salt)
        case.run(g, 50, 250)
        ends.append(states_bytes(g)[:, 16:])
        g.close()
    assert (ends[0] != ends[1]).any(axis=1).sum() > n // 2, "most envs should have parted ways"


# ---------------------------------------------------------------- 10. the outputs of the last step stay

def test_outputs_stay(hip_lib):
    n = 24
    case = Agent("breakout", n)
    g = case.make(hip_lib)
    g.checkpoint_slots(1)
    case.run(g, 0, 10)
    g.checkpoint_save(0)
    case.run(g, 10, 30)
    ids = [(_abi.BUF_REWARD, np.int32), (_abi.BUF_DONE, np.uint8), (_abi.BUF_LIVES, np.int32), (_abi.BUF_SCORE, np.int32),
           (_abi.BUF_PACKED, np.uint64), (_abi.BUF_AGENT_REWARD, np.float32), (_abi.BUF_AGENT_DONE, np.uint8),
           (_abi.BUF_AGENT_EP_DONE, np.uint8), (_abi.BUF_AGENT_EP_RETURN, np.float32), (_abi.BUF_AGENT_EP_LENGTH, np.int32)]
    before = [read_buffer(g, which, (n,), dt) for which, dt in ids]
    obs = case.observation(g)
    g.checkpoint_restore(0, rows=n - 1 - np.arange(n))
    for (which, dt), x in zip(ids, before):
        assert np.array_equal(read_buffer(g, which, (n,), dt), x), "buffer %d changed in a restore" % which
    assert not np.array_equal(case.observation(g), obs), "the restore did not move the observation"
    g.close()


# ---------------------------------------------------------------- 11. a pending host step ends first

def test_restore_between_step_begin_and_step_end_delivers_the_step_first(hip_lib, oracle_lib):
    n = 24
    case = Agent("breakout", n)
    g, o = case.make(hip_lib), case.make(oracle_lib)
    g.checkpoint_slots(1)
    case.run(g, 0, 20); case.run(o, 0, 20)
    g.checkpoint_save(0)
    case.run(g, 20, 30); want = case.run(o, 20, 31)[-1]
    out = {"reward": g.host_array((n,), np.float32), "done": g.host_array((n,), np.uint8), "obs": g.host_array((n, 84, 84, 4))}
    g.agent_step_begin(case.actions(30), **out)
    rev = n - 1 - np.arange(n)
    g.checkpoint_restore(0, rows=rev)
    g.agent_step_end()
    assert np.array_equal(out["obs"], want[0]) and np.array_equal(out["reward"], want[1]) and np.array_equal(out["done"].astype(bool), want[2])
    o2 = replay_to(case, oracle_lib, rev, 20)
    assert np.array_equal(case.observation(g), case.observation(o2))
    assert_snapshot(snapshot(g), snapshot(o2), "restore inside a pending step")
    g.close(); o.close(); o2.close()


# ---------------------------------------------------------------- 12. the VecEnv adapters

@pytest.mark.parametrize("layout", ["device_stack", "planes", "host_stack"])
@pytest.mark.parametrize("game", ["breakout", "space_invaders"])
def test_preproc_vec_env_checkpoint(game, layout, hip_lib, oracle_lib):
    """the batch restore_checkpoint returns and the next steps' equal the replay's; unselected envs go on as they were"""
    from toybox_amd.envs import ToyboxPreprocVecEnv
    n, t_s, t_r = 16, 30, 53
    kw = dict(seed=3, episode_life=True, fire_reset=True, noop_max=30)
    rng = np.random.default_rng(1)
    A = rng.integers(0, 4, (t_r + 40, n))
    envs = np.flatnonzero(np.arange(n) % 4 != 0)
    sel = np.zeros(n, bool)
    sel[envs] = True
    rows, eff = restore_map(n, rng.integers(0, n, n), sel)
    counts = (1 + (3 * np.arange(n)) % 30).astype(np.int32)

    def make(lib, lay, m):
        v = ToyboxPreprocVecEnv(game, n, obs_layout=lay, engine=Engine(game, n, lib=lib), **kw)
        v.engine.seed_array([((3 + int(i) + 1) * 2654435761) % 2 ** 31 for i in m])
        v.engine.agent_set_noops(counts[m])
        return v, np.asarray(v.reset()).copy()

    va, _ = make(hip_lib, layout, np.arange(n))
    vo, _ = make(oracle_lib, "device_stack", np.arange(n))
    vs, _ = make(oracle_lib, "device_stack", eff)
    va.checkpoint_slots(1)
    for t in range(t_s):
        va.step(A[t]); vo.step(A[t]); obs_s = np.asarray(vs.step(A[t][eff])[0]).copy()
    va.save_checkpoint(0)
    for t in range(t_s, t_r):
        va.step(A[t]); obs_o = np.asarray(vo.step(A[t])[0]).copy()
    if layout == "planes":
        va.step_async(A[t_r])                                # between step_async and step_wait: the step ends first
        obs_o = np.asarray(vo.step(A[t_r])[0]).copy()
        t_r += 1
    got = np.asarray(va.restore_checkpoint(0, rows=rows, envs=envs))
    assert np.array_equal(got, pick_rows(sel, obs_s, obs_o)), "the observation restore_checkpoint returns is not the replay's"
    vs.engine.agent_set_noops(counts)
    for k in range(30):
        a = np.where(sel, A[t_s + k][eff], A[t_r + k])
        oa, ra, da, ia = va.step(a)
        (ob, rb, db, ib), (oc, rc, dc, ic) = vs.step(a), vo.step(a)
        assert np.array_equal(np.asarray(oa), pick_rows(sel, np.asarray(ob), np.asarray(oc))), k
        assert np.array_equal(ra, pick_rows(sel, rb, rc)) and np.array_equal(da, pick_rows(sel, db, dc)), k
        ea, eb, ec = ia.with_key("episode"), ib.with_key("episode"), ic.with_key("episode")
        want = {i: (d["r"], d["l"]) for i, d in eb.items() if sel[i]}
        want.update({i: (d["r"], d["l"]) for i, d in ec.items() if not sel[i]})
        assert {i: (d["r"], d["l"]) for i, d in ea.items()} == want, k
    assert np.array_equal(va.engine.checkpoint_valid(0), np.ones(n, np.int8))
    va.checkpoint_slots(1)                                   # reallocating the store empties it
    assert np.array_equal(va.engine.checkpoint_valid(0), np.zeros(n, np.int8))
    va.checkpoint_slots(0)
    assert np.array_equal(va.engine.checkpoint_valid(0), np.full(n, -1, np.int8))
    va.close(); vo.close(); vs.close()


@pytest.mark.parametrize("grayscale", [True, False])
def test_vec_env_checkpoint(grayscale, hip_lib, oracle_lib):
    from toybox_amd.envs import ToyboxVecEnv
    game, n, t_s, t_r = "breakout", 12, 50, 80
    rng = np.random.default_rng(2)
    A = rng.integers(0, 4, (t_r + 40, n))
    sel = np.arange(n) % 3 != 0
    rows, eff = restore_map(n, rng.integers(0, n, n), sel)

    def make(lib, m):
        v = ToyboxVecEnv(game, n, grayscale=grayscale, engine=Engine(game, n, lib=lib), cache_terminal_state=False)
        v.engine.seed_array([1000 + 17 * int(i) for i in m])
        v.engine.new_game()
        v.engine.edit(_abi.EDIT_SET_LIVES, [1])
        return v

    va, vo, vs = make(hip_lib, np.arange(n)), make(oracle_lib, np.arange(n)), make(oracle_lib, eff)
    va.checkpoint_slots(1)
    for t in range(t_s):
        va.step(A[t]); vo.step(A[t]); obs_s = np.asarray(vs.step(A[t][eff])[0]).copy()
    va.save_checkpoint(0)
    for t in range(t_s, t_r):
        va.step(A[t]); obs_o = np.asarray(vo.step(A[t])[0]).copy()
    got = np.asarray(va.restore_checkpoint(0, rows=rows, envs=sel))
    assert np.array_equal(got, pick_rows(sel, obs_s, obs_o))
    for k in range(40):
        a = np.where(sel, A[t_s + k][eff], A[t_r + k])
        oa, ra, da, ia = va.step(a)
        (ob, rb, db, ib), (oc, rc, dc, ic) = vs.step(a), vo.step(a)
        assert np.array_equal(np.asarray(oa), pick_rows(sel, np.asarray(ob), np.asarray(oc))), k
        assert np.array_equal(ra, pick_rows(sel, rb, rc)) and np.array_equal(da, pick_rows(sel, db, dc)), k
        assert np.array_equal([d["score"] for d in ia], pick_rows(sel, [d["score"] for d in ib], [d["score"] for d in ic]))
    va.checkpoint_slots(1)
    assert np.array_equal(va.engine.checkpoint_valid(0), np.zeros(n, np.int8))
    va.checkpoint_slots(0)
    assert np.array_equal(va.engine.checkpoint_valid(0), np.full(n, -1, np.int8))
    va.close(); vo.close(); vs.close()
