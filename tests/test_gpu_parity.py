"""GPU parity: the HIP engine (through the C-ABI) against the CPU oracle on identical seeds and
action sequences.  The bar is bit-exact: integer fields, RNG words, binary64 positions/velocities
(compared as raw bytes of the POD records) and every frame byte."""
import ctypes as C

import numpy as np
import pytest

import rule_inputs
from rule_inputs import fuzz_amidar as _fuzz_amidar, fuzz_breakout as _fuzz_breakout, fuzz_si as _fuzz_si
from support import synthetic_actions
from toybox_amd import Engine, _abi
from toybox_amd.games import codec

pytestmark = pytest.mark.gpu


def _pair(game, n, hip_lib, oracle_lib, seed=1234):
    g = Engine(game, n, lib=hip_lib)
    o = Engine(game, n, lib=oracle_lib)
    for e in (g, o):
        e.seed(seed)
        e.new_game()
    return g, o


def _assert_states_equal(g, o, envs):
    for i in envs:
        a, b = bytes(g.get_state(int(i))), bytes(o.get_state(int(i)))
        if a != b:
            cd = codec(g.game)
            ja, jb = cd.state_to_json(g.get_state(int(i))), cd.state_to_json(o.get_state(int(i)))
            diff = {k: (ja[k], jb[k]) for k in ja if ja[k] != jb[k] and k not in ("bricks", "enemies", "shields", "board")}
            raise AssertionError("env %d differs: %r" % (i, diff))


def _check(ev, g, o):
    """one event of a tests/rule_inputs.py script played over (g, o): the two engines' results are equal"""
    kind = ev[0]
    if kind == "step":
        for x, y, name in zip(ev[2][0], ev[2][1], ("reward", "done", "lives", "score")):
            assert np.array_equal(x, y), "%s differs at step %d (envs %s)" % (name, ev[1], np.nonzero(x != y)[0][:8])
    elif kind == "frames":
        fg, fo = ev[2]
        assert np.array_equal(fg, fo), (ev[1], np.argwhere(fg != fo)[:3])
    elif kind == "states":
        _assert_states_equal(g, o, ev[1])
    elif kind == "agent":
        for p, q in zip(*ev[2]):
            assert np.array_equal(p, q), ev[1]


@pytest.mark.parametrize("game", ["breakout", "space_invaders", "amidar"])
def test_rollout_parity(game, hip_lib, oracle_lib):
    """4096 envs, seeds 1234+i, 1500 random-action frames with auto-reset: outputs equal every step,
    full state records equal at checkpoints and at the end."""
    n, steps = 4096, 1500
    g, o = _pair(game, n, hip_lib, oracle_lib)
    rng = np.random.default_rng(0)
    sample = rng.choice(n, 64, replace=False)
    _assert_states_equal(g, o, sample)
    n_done = 0
    for ev in rule_inputs.rollout([g, o], n, game, steps):
        _check(ev, g, o)
        t = ev[1]
        n_done += int(ev[2][0][1].sum())
        if t % 250 == 249:
            _assert_states_equal(g, o, sample)
    _assert_states_equal(g, o, range(n))
    assert n_done > 0, "the rollout never finished an episode; auto-reset path untested"
    sg, so = g.scalars(), o.scalars()
    for x, y in zip(sg, so):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("game", ["breakout", "space_invaders", "amidar"])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_frame_parity(game, channels, hip_lib, oracle_lib):
    n = 256
    g, o = _pair(game, n, hip_lib, oracle_lib, seed=99)
    for t in range(400):
        a = synthetic_actions(game, n, t, seed=5)
        g.step(a, auto_reset=True)
        o.step(a, auto_reset=True)
        if t in (0, 1, 57, 199, 399):
            fg, fo = g.render(channels), o.render(channels)
            assert fg.shape == (n, g.height, g.width, channels)
            if not np.array_equal(fg, fo):
                bad = np.argwhere(fg != fo)
                raise AssertionError("frames differ at step %d: %d bytes, first %s" % (t, len(bad), bad[:5]))
    assert np.array_equal(g.render_env(3, channels), o.render_env(3, channels))


@pytest.mark.parametrize("game", ["breakout", "space_invaders", "amidar"])
def test_synthetic_device_path(game, hip_lib, oracle_lib):
    """tbx_step_synthetic (actions generated in-kernel) == host-generated actions with the same rule."""
    n = 1024
    g, o = _pair(game, n, hip_lib, oracle_lib)
    for ev in rule_inputs.synthetic_path([g, o], n, game):
        g.sync()
        _check(ev, g, o)
    # the packed {reward, done, lives} record of the last step
    p, nbytes = g.device_buffer(_abi.BUF_PACKED)
    assert p and nbytes == 8 * n


def test_illegal_action_is_reported(hip_lib, oracle_lib):
    for lib in (hip_lib, oracle_lib):
        with Engine("breakout", 4, lib=lib) as e:
            with pytest.raises(Exception) as ei:
                e.step([0, 1, 99, 3])
            assert ei.value.code == _abi.E_ACTION
            e.step([0, 1, 3, 4])   # flag is cleared; engine keeps working


def test_breakout_interventions_parity(hip_lib, oracle_lib):
    """State writes the reference's tests perform (test/interventions/test_breakout_interventions.py): a second
    ball, bricks toggled, a recoloured brick, moved paddle -- plus non-canonical brick geometry, which flips the
    device engine into its per-env brick-table mode."""
    n = 8
    g, o = _pair("breakout", n, hip_lib, oracle_lib)
    for ev in rule_inputs.breakout_interventions([g, o], n):
        _check(ev, g, o)


def test_breakout_config_change_parity(hip_lib, oracle_lib):
    """write_config_json + new_game (interventions/base.py:401-403): 8 rows, other scores/speeds."""
    n = 64
    g, o = _pair("breakout", n, hip_lib, oracle_lib)
    for ev in rule_inputs.breakout_config_change([g, o], n):
        if ev[0] == "config":
            assert g.get_state(0).n_bricks == 18 * 8
        _check(ev, g, o)


@pytest.mark.parametrize("game", ["breakout", "space_invaders", "amidar"])
def test_full_size_properties(game, hip_lib):
    """BASELINE size (65536 envs), every game: properties that need no oracle -- determinism of two identically seeded
    engines' frames and outputs (host actions on one, device-generated ones on the other), reward == max(delta score, 0),
    done == (lives <= 0)."""
    n = 65536
    a_eng = Engine(game, n, lib=hip_lib)
    a_eng.seed(1234)
    a_eng.new_game()
    prev = np.zeros(n, np.int64)
    total = np.zeros(n, np.int64)
    for t in range(300):
        r, d, l, s = a_eng.step(synthetic_actions(game, n, t), auto_reset=False)
        assert np.array_equal(r, np.maximum(s - prev, 0))
        assert np.array_equal(d, l <= 0)
        prev = s.astype(np.int64)
        total += r
    assert total.sum() > 0
    # a second engine, same seeds/actions, rendered in chunks: checksums must agree
    b_eng = Engine(game, n, lib=hip_lib)
    b_eng.seed(1234)
    b_eng.new_game()
    for t in range(300):
        b_eng.step_synthetic(1337, t, auto_reset=False)
    b_eng.sync()
    sa, sb = a_eng.scalars(), b_eng.scalars()
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y)
    for i in (0, 1, 4095, 40000, 65535):
        assert bytes(a_eng.get_state(i)) == bytes(b_eng.get_state(i))
        assert np.array_equal(a_eng.render_env(i, 3), b_eng.render_env(i, 3))
    a_eng.close()
    b_eng.close()


def test_amidar_protocols_parity(hip_lib, oracle_lib):
    """Every enemy movement protocol of interventions/amidar.py:101-112 (incl. EnemyRandomMvmt, which draws from the
    state RNG in enemy order), a 6th enemy, chase / jump modes and painted boxes, stepped on both engines."""
    n = 16
    g, o = _pair("amidar", n, hip_lib, oracle_lib)
    for ev in rule_inputs.amidar_protocols([g, o], n):
        _check(ev, g, o)


@pytest.mark.parametrize("game", ["breakout", "space_invaders", "amidar"])
def test_full_size_batch_parity(game, hip_lib, oracle_lib, monkeypatch):
    """BASELINE's batch size (65 536 envs, seeds 1234+i): every per-step output of every env equals the CPU restatement for
    1200 auto-resetting frames; full state records and frames are compared on a sample (the records alone would be ~1 GB),
    and the score / lives / level vectors of the whole batch at the end."""
    monkeypatch.setenv("TBX_ORACLE_THREADS", str(min(16, len(__import__("os").sched_getaffinity(0)))))
    n, steps = 65536, 1200
    g, o = _pair(game, n, hip_lib, oracle_lib)
    sample = np.random.default_rng(1).choice(n, 96, replace=False)
    acc = np.zeros(n, np.int64)
    dones = 0
    for t in range(steps):
        a = synthetic_actions(game, n, t)
        rg, ro = g.step(a, auto_reset=True), o.step(a, auto_reset=True)
        for x, y, name in zip(rg, ro, ("reward", "done", "lives", "score")):
            assert np.array_equal(x, y), "%s differs at step %d (envs %s)" % (name, t, np.nonzero(x != y)[0][:8])
        acc += rg[0]
        dones += int(rg[1].sum())
    _assert_states_equal(g, o, sample)
    for x, y in zip(g.scalars(), o.scalars()):
        assert np.array_equal(x, y)
    for i in sample[:24]:
        assert np.array_equal(g.render_env(int(i), 3), o.render_env(int(i), 3)), i
    assert acc.sum() > 0 and (game != "breakout" or dones > 0)      # rewards flowed; Breakout games ended and restarted
    # the bench's own launches at the bench's size: the batched RGB render of all 65 536 envs (Breakout: two parts), then the
    # fused rollout call (Breakout: rasteriser + step in one launch), frames read back through device-side sampling
    from toybox_amd import hip
    H, W = g.height, g.width
    fb = H * W * 3
    picks = [0, 1, 1023, 1024, 1025, n - 1] + [int(i) for i in sample[:34]]
    one = np.empty((H, W, 3), np.uint8)
    for fused in (False, True):
        want = [o.render_env(i, 3) for i in picks]
        if fused:
            g.render_step_synthetic(1337, steps, channels=3, auto_reset=True)
            o.step(synthetic_actions(game, n, steps, seed=1337), auto_reset=True)
        else:
            g.render_device(0, 3)
        g.sync()
        p, nbytes = g.device_buffer(_abi.BUF_FRAME)
        assert nbytes >= n * fb
        for i, w in zip(picks, want):
            hip.memcpy_dtoh(one, p + i * fb, fb)
            assert np.array_equal(one, w), (game, fused, i)
    _assert_states_equal(g, o, sample[:32])


@pytest.mark.parametrize("game", ["breakout", "space_invaders", "amidar", "gridworld"])
def test_big_batch_launch_frames_parity(game, hip_lib, oracle_lib, monkeypatch):
    """The batched RGB launch at a size where the big-launch forms are in force -- Breakout's render in two parts (1 024 envs,
    then the rest), SpaceInvaders' staggered first waves, GridWorld's five waves per frame, Amidar's six waves per SIMD --
    against the oracle's frames: the envs on both sides of the part boundary, the ends of the batch and a random sample, after
    a mid-game pre-roll, and again after more steps: every env's frame (tests/support.py FrameChecker)."""
    from support import FrameChecker, device_frames, oracle_frames
    monkeypatch.setenv("TBX_ORACLE_THREADS", str(min(16, len(__import__("os").sched_getaffinity(0)))))
    n = 16384
    g, o = _pair(game, n, hip_lib, oracle_lib, seed=77)
    H, W = g.height, g.width
    chk = FrameChecker((H, W, 3), pinned=True)
    t = 0
    for rounds in (120, 40):
        for _ in range(rounds):
            a = synthetic_actions(game, n, t, seed=5)
            g.step(a, auto_reset=True), o.step(a, auto_reset=True)
            t += 1
        g.render_device(0, 3)
        g.sync()
        p, nbytes = g.device_buffer(_abi.BUF_FRAME)
        assert nbytes >= n * H * W * 3
        chk.compare(device_frames(p, H * W * 3), oracle_frames(o, 3), n, what="%s t=%d" % (game, t))


def test_space_invaders_interventions_parity(hip_lib, oracle_lib):
    """Hand-written SpaceInvaders states: enemies stacked on top of each other (paint order, the multi-candidate path of the
    rasteriser), eight enemy lasers over shields and ship, a chewed shield, a visible ufo, an exploding ship, out-of-frame
    objects -- frames in every format, the fused observation, and the dynamics from there."""
    n = 24
    g, o = _pair("space_invaders", n, hip_lib, oracle_lib, seed=8)
    for ev in rule_inputs.si_interventions([g, o], n):
        _check(ev, g, o)


def test_amidar_interventions_parity(hip_lib, oracle_lib):
    """Hand-written Amidar states: movers on top of each other and of the player, at the board's edges and between tiles,
    painted boxes (interior fill), repainted track, chase and jump modes, a caught enemy -- frames in every format, the
    fused observation (movers differ between the two sub-frames, the board usually does not), and the dynamics from there."""
    n = 24
    g, o = _pair("amidar", n, hip_lib, oracle_lib, seed=8)
    for ev in rule_inputs.amidar_interventions([g, o], n):
        _check(ev, g, o)


def test_level_transitions_parity(hip_lib, oracle_lib):
    """Level completion is out of reach of short random rollouts, so it is set up by hand in every game: the last brick / the
    last invader / the last unpainted track, then the frames in which the level changes and the new wall / formation / board
    appears -- identical on both sides, and the level counter really moves."""
    n = 8
    # Breakout: one brick left, a ball right under it flying up
    g, o = _pair("breakout", n, hip_lib, oracle_lib, seed=3)
    for ev in rule_inputs.breakout_level_transition([g, o], n):
        if ev[0] == "written":
            lv0 = o.scalars()[2].copy()
        _check(ev, g, o)
    assert (o.scalars()[2] == lv0 + 1).all() and np.array_equal(g.render(3), o.render(3))
    assert all(sum(b.alive for b in list(o.get_state(i).bricks)[:108]) >= 95 for i in range(n))     # the wall is back (the ball keeps eating)

    # SpaceInvaders: one invader left with the ship's laser right under it
    g, o = _pair("space_invaders", n, hip_lib, oracle_lib, seed=3)
    for ev in rule_inputs.si_level_transition([g, o], n):
        if ev[0] == "written":
            lv0 = o.scalars()[2].copy()
        _check(ev, g, o)
    assert (o.scalars()[2] == lv0 + 1).all() and np.array_equal(g.render(3), o.render(3))
    assert all(sum(en.alive for en in list(o.get_state(i).enemies)[:36]) >= 30 for i in range(n))       # a fresh formation

    # Amidar: every piece of track painted except the stretch of the right-hand column the player is about to close
    g, o = _pair("amidar", n, hip_lib, oracle_lib, seed=3)
    for ev in rule_inputs.amidar_level_transition([g, o], n):
        if ev[0] == "written":
            lv0 = o.scalars()[2].copy()
        _check(ev, g, o)
    assert (o.scalars()[2] > lv0).sum() >= n // 2 and np.array_equal(g.render(3), o.render(3))


@pytest.mark.parametrize("fuzz_seed", rule_inputs.FUZZ_SEEDS)
@pytest.mark.parametrize("game,fuzz", [pytest.param("breakout", _fuzz_breakout, id="breakout-_fuzz_breakout"),
                                       pytest.param("space_invaders", _fuzz_si, id="space_invaders-_fuzz_si"),
                                       pytest.param("amidar", _fuzz_amidar, id="amidar-_fuzz_amidar")])
def test_fuzzed_states_parity(game, fuzz, fuzz_seed, hip_lib, oracle_lib):
    """Randomised hand-written states -- out-of-frame and overlapping objects, degenerate sizes, odd counters, scores
    beyond the HUD's digits -- written to both libraries: every frame format, then 120 frames of dynamics (auto-reset on)
    and the agent pipeline, all equal to the CPU restatement."""
    n = 96
    g, o = _pair(game, n, hip_lib, oracle_lib, seed=21)
    assert fuzz is rule_inputs.FUZZ[game]
    for ev in rule_inputs.fuzzed_states([g, o], n, game, fuzz_seed):
        _check(ev, g, o)


def _fuzz_si_on_the_grid(st, rng, extreme):
    """everything the record rasteriser digests, with the formation left on its grid (moved as a whole): sprites half off every
    edge, rectangles far outside the frame, coordinates at the ends of int32"""
    _fuzz_si(st, rng)
    x0 = int(rng.integers(-130, 330)); y0 = int(rng.integers(-120, 215))
    for j in range(st.n_enemies):
        st.enemies[j].x, st.enemies[j].y = x0 + 32 * (j % 6), y0 + 18 * (j // 6)
    big = 2 ** 30 - 1
    if extreme == 1:
        st.ship_x, st.ufo_x = -big, big
        for k in range(st.n_enemy_lasers):
            st.enemy_lasers[k].x, st.enemy_lasers[k].w = -big + k, big       # far left, reaching back onto the screen
        for k in range(st.n_shields):
            st.shield_x[k] = int(rng.choice([-big, big, -17, 318]))
    elif extreme == 2:
        for j in range(st.n_enemies):
            st.enemies[j].x, st.enemies[j].y = big - 200 + 32 * (j % 6), -big + 18 * (j // 6)
        st.ship_y, st.ufo_y = int(rng.integers(-30, 230)), int(rng.integers(-30, 230))
        for k in range(st.n_enemy_lasers):
            st.enemy_lasers[k].y, st.enemy_lasers[k].h = -5, big
        for k in range(st.n_shields):
            st.shield_y[k] = int(rng.choice([-9, 200, big]))


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [6, 10])
def test_space_invaders_record_rasteriser_fuzz(n_rows, hip_lib, oracle_lib):
    """SpaceInvaders' rasteriser paints from records the step kernel leaves behind (formation origin + alive / exploding masks,
    clipped laser rectangles, clamped sprite positions) as long as the enemies sit on the formation grid.  Fuzzed states ON the
    grid, frames in every format: straight after the write (records rebuilt from state), after steps (records written by the step
    kernel), with the steps running beside the rasteriser (pipelined mode), and back to the state-reading rasteriser when one
    env leaves the grid."""
    from toybox_amd import hip
    n = 120
    with Engine("space_invaders", 1, lib=oracle_lib) as e0:
        cfg = e0.get_config()
    cfg.n_rows = n_rows
    for i in range(n_rows):
        cfg.row_scores[i] = 5 * (n_rows - i)
    g, o = Engine("space_invaders", n, lib=hip_lib, config=cfg), Engine("space_invaders", n, lib=oracle_lib, config=cfg)
    for e in (g, o):
        e.seed(4); e.new_game()
    assert g.get_option(_abi.OPT_RECORDS_ACTIVE) == 1
    assert np.array_equal(g.render(3), o.render(3))                      # straight after a new game
    for t in range(150):
        a = synthetic_actions("space_invaders", n, t, seed=2)
        g.step(a); o.step(a)
    rng = np.random.default_rng(77 + n_rows)
    recs = o.get_states(0, n)
    for i in range(n):
        _fuzz_si_on_the_grid(recs[i], rng, i % 4 if i % 4 < 3 else 0)
    for e in (g, o):
        e.set_states(0, recs)
    assert g.get_option(_abi.OPT_RECORDS_ACTIVE) == 1                    # still on the grid
    _assert_states_equal(g, o, range(n))
    for ch in (1, 3, 4):
        assert np.array_equal(g.render(ch), o.render(ch)), ch
    for i in (0, 1, 2, n - 1):
        assert np.array_equal(g.render_env(i, 3), o.render_env(i, 3)), i
    for t in range(120):                                                # records now come from the step kernel
        a = synthetic_actions("space_invaders", n, t, seed=9)
        rg, ro = g.step(a, auto_reset=True), o.step(a, auto_reset=True)
        for x, y in zip(rg, ro):
            assert np.array_equal(x, y), t
        if t % 17 == 0:
            assert np.array_equal(g.render(3), o.render(3)), t
    g.set_option(_abi.OPT_PIPELINE, 2)                                  # steps beside the previous frame's rasteriser
    assert g.get_option(_abi.OPT_PIPELINE_ACTIVE) == 2
    st = hip.Stream()
    H, W = g.height, g.width
    one = np.empty((H, W, 3), np.uint8)
    for t in range(120, 200):
        g.step_synthetic(1337, t, auto_reset=True, stream=st.ptr)
        g.render_device(0, 3, stream=st.ptr)
        o.step(synthetic_actions("space_invaders", n, t, seed=1337), auto_reset=True)
        if t % 13 == 0:
            st.synchronize()
            p, _ = g.device_buffer(_abi.BUF_FRAME)
            for i in (0, 7, n - 1):
                hip.memcpy_dtoh(one, p + i * H * W * 3, H * W * 3)
                assert np.array_equal(one, o.render_env(i, 3)), (t, i)
    g.sync()
    _assert_states_equal(g, o, range(n))
    s5 = o.get_state(5)
    s5.enemies[3].x += 1                                                 # one enemy off the grid: records can no longer describe it
    for e in (g, o):
        e.set_state(5, s5)
    assert g.get_option(_abi.OPT_RECORDS_ACTIVE) == 0 and g.get_option(_abi.OPT_PIPELINE_ACTIVE) == 0
    for t in range(200, 230):
        g.step_synthetic(1337, t, auto_reset=True, stream=st.ptr)
        o.step(synthetic_actions("space_invaders", n, t, seed=1337), auto_reset=True)
    g.sync()
    for ch in (1, 3, 4):
        assert np.array_equal(g.render(ch), o.render(ch)), ch
