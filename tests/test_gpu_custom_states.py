"""Written states at batch scale: Breakout's per-env brick tables (the CUSTOM = true kernels) and SpaceInvaders' off-grid formations
(the state-reading rasteriser, the step kernel that loads every row), held to the CPU oracle bit for bit -- every output of every env
at every step, the raw state bytes of every env, every byte of every frame.

* generators, vectorised over the numpy view of the state records (Engine.get_states_np / set_states_np), seeded from TBX_FUZZ_SEED;
* a batch of 1 027 envs (no multiple of a block, of four waves or of 64) through every frame format and split factor, the batch step,
  and the loop entry points, which fall back to stream order on such an engine;
* the write of one non-canonical state INTO a running overlapped loop form (pipelined mode, fused render + step, rollout chunks);
* the agent layer on custom Breakout, which leaves the fused observation kernels for the generic render-and-warp path -- also on an
  engine whose agent layer was initialised while the wall was canonical;
* directed Amidar states for enemy-AI arms random play does not reach.

The tests without the gpu mark are the twins: the same generators and loops over the checker alone, with the conditions that say the
generated states still reach the code (bricks are hit, levels change, games end), so a generator that has gone dull fails where no GPU
is."""
import os

import numpy as np
import pytest

from fork_replay import effective, sim_rngs, states_bytes
import rule_inputs
from rule_inputs import BRK_H, BRK_N_BRICKS, BRK_RADII, BRK_W, SI_N_ENEMIES, _random_colors, gen_breakout, gen_si
from support import FrameChecker, device_frames, oracle_frames, read_buffer, synthetic_actions
from rule_inputs import fuzz_si as _fuzz_si
from toybox_amd import Engine, ToyboxAmdError, _abi

ACTIVE_OPTIONS = {"records": _abi.OPT_RECORDS_ACTIVE, "pipeline": _abi.OPT_PIPELINE_ACTIVE, "fused overlap": _abi.OPT_FUSED_OVERLAP_ACTIVE,
                  "rollout chunks": _abi.OPT_ROLLOUT_CHUNKS_ACTIVE}


@pytest.fixture
def fuzz_seed():
    seed = int(os.environ.get("TBX_FUZZ_SEED", 2024))
    print("TBX_FUZZ_SEED=%d" % seed)                # (captured output is shown for a failing test only)
    return seed


# ---------------------------------------------------------------- generators

def generate(game, o, rng, kind=None):
    """the generated states of the whole batch, from the oracle engine's current ones"""
    return gen_breakout(o.get_states_np(), rng, kind) if game == "breakout" else gen_si(o.get_states(), rng, kind)


def one_generated_state(game, o, seed):
    """one non-canonical state as a ctypes record: a random brick table / a formation of another size"""
    src = o.get_states(0, 4)
    rng = np.random.default_rng(seed)
    st = gen_breakout(np.frombuffer(src, dtype=np.dtype(o.state_type)).copy(), rng, [1] * 4) if game == "breakout" else gen_si(src, rng, [0] * 4)
    if game == "space_invaders":
        st["n_enemies"][1] = 37
    return o.state_type.from_buffer_copy(st[1].tobytes())


# ---------------------------------------------------------------- shared loops (one engine: the checker alone; two: device, checker)

_engines = rule_inputs.custom_batch_engines


def _close(es):
    for e in es:
        e.close()


def _write_all(es, st):
    for e in es:
        e.set_states_np(0, st)


def _same_states(es, what):
    if len(es) < 2:
        return
    a, b = (states_bytes(e) for e in es)
    if not np.array_equal(a, b):
        bad = np.flatnonzero((a != b).any(axis=1))
        i = int(bad[0])
        raise AssertionError("%s: state records differ in %d envs, first env %d at byte %d" % (what, len(bad), i, int(np.flatnonzero(a[i] != b[i])[0])))


def _same_rngs(es, what):
    if len(es) == 2:
        assert np.array_equal(sim_rngs(es[0]), sim_rngs(es[1])), what


def _assert_stream_order(g, what):
    for name, opt in ACTIVE_OPTIONS.items():
        assert g.get_option(opt) == 0, "%s: %s still active" % (what, name)


def _device_frames_equal(g, o, chk, channels, what):
    g.render_device(0, channels)
    g.sync()
    p, nbytes = g.device_buffer(_abi.BUF_FRAME)
    fb = g.height * g.width * channels
    assert nbytes >= g.n_envs * fb
    chk.compare(device_frames(p, fb), oracle_frames(o, channels), g.n_envs, what=what)


def run_steps(es, game, steps, action_seed=2, frames_every=0, watch=None):
    """`steps` frames of tbx_step with auto-reset on every engine of `es`: outputs compared at every step, every env's frame (formats
    in turn) every `frames_every`-th step; watch(t, outputs, engine) sees the last engine's (the checker's) every step"""
    n = es[0].n_envs
    chks = {}
    for t in range(steps):
        a = synthetic_actions(game, n, t, seed=action_seed)
        outs = [e.step(a, auto_reset=True) for e in es]
        for x, y, name in zip(outs[0], outs[-1], ("reward", "done", "lives", "score")):
            assert np.array_equal(x, y), "%s differs at step %d (envs %s)" % (name, t, np.flatnonzero(x != y)[:8])
        if watch:
            watch(t, outs[-1], es[-1])
        if frames_every and t % frames_every == frames_every - 1 and len(es) == 2:
            ch = (3, 1, 4)[(t // frames_every) % 3]
            chk = chks.setdefault(ch, FrameChecker((es[0].height, es[0].width, ch)))
            _device_frames_equal(es[0], es[1], chk, ch, "%s step %d channels %d" % (game, t, ch))


def agent_observation(e, obs, stream=None):
    """the current observation: the rolled stack tbx_agent_step returned (uint8[N, h, w, stack]), or -- new_plane = 2 -- the plane ring
    read in head order (uint8[stack, N, h, w], oldest first: slot (head + 1 + c) % stack is channel c); stream: the ring is read
    behind the producing call on that stream (read_buffer) instead of behind tbx_sync"""
    if obs is not None:
        return obs
    n, oh, ow, stack = e._agent_shape
    ring = read_buffer(e, _abi.BUF_AGENT_RING, (stack, n, oh, ow), stream=stream)
    return ring[(e.agent_ring_head() + 1 + np.arange(stack)) % stack]


def run_agent(es, game, t0, t1, action_seed=7, env_map=None, tolerate_needs_reset=False):
    """agent steps t0 .. t1-1 on every engine of `es` (env i takes env env_map[i]'s action): observation, reward, done and the episode
    monitor compared at every step; -> (done count, episode count, the last engine's rows).  tolerate_needs_reset: a step on an env
    whose game ended inside EpisodicLifeEnv's no-op step is carried out and compared like any other (Engine.agent_step)"""
    n = es[0].n_envs
    dones = episodes = 0
    rows = []
    for t in range(t0, t1):
        a = synthetic_actions(game, n, t, seed=action_seed)
        a = a if env_map is None else a[env_map]
        outs = []
        for e in es:
            obs, reward, done = e.agent_step(a, tolerate_needs_reset=tolerate_needs_reset)
            ended, ret, length = e.agent_episodes()
            outs.append((agent_observation(e, obs), reward, done, ended, np.where(ended, ret, 0), np.where(ended, length, 0)))
        for x, y, name in zip(outs[0], outs[-1], ("observation", "reward", "done", "episode end", "episode return", "episode length")):
            if not np.array_equal(x, y):
                diff = np.moveaxis(x != y, 1, 0) if x.shape[0] != n else x != y       # (the ring is [stack][N]...)
                bad = np.flatnonzero(diff.reshape(n, -1).any(axis=1))
                raise AssertionError("agent step %d: %s differs in %d envs, first %s" % (t, name, len(bad), bad[:8]))
        dones += int(outs[-1][2].sum())
        episodes += int(outs[-1][3].sum())
        rows.append(outs[-1])
    return dones, episodes, rows


AGENT = dict(skip=4, out_h=84, out_w=84, stack=4, clip_reward=False, episodic_life=False, fire_reset=False, noop_max=0)


def half_custom(o, rng):
    """the batch's current states with a generated table and 1-3 lives in every second env"""
    cur = o.get_states_np()
    gen = gen_breakout(cur, rng)
    cur[1::2] = gen[1::2]
    cur["lives"][1::2] = rng.integers(1, 4, len(cur[1::2]))
    return cur


def agent_on_custom_breakout(es, variant, new_plane, seed, steps=400):
    """(a) tbx_agent_init after the custom write; (b) on the canonical engine, 20 agent steps, then the custom write into every second
    env -- which takes a device engine off its fused observation path with the agent layer already sized"""
    rng = np.random.default_rng(seed)
    o = es[-1]
    t = 0
    if variant == "a":
        _write_all(es, gen_breakout(o.get_states_np(), rng))
    for e in es:
        e.agent_init(new_plane=new_plane, **AGENT)
    if variant == "b":
        run_agent(es, "breakout", 0, 20)
        t = 20
        _write_all(es, half_custom(o, rng))
    _same_states(es, "after the write")
    dones, episodes, _ = run_agent(es, "breakout", t, t + steps)
    _same_states(es, "after %d agent steps" % steps)
    _same_rngs(es, "simulator RNG after %d agent steps" % steps)
    assert dones > 0 and episodes > 0, (dones, episodes)
    return dones, episodes


# ---------------------------------------------------------------- 2. batch-scale parity in custom mode

@pytest.mark.gpu
@pytest.mark.parametrize("game", ["breakout", "space_invaders"])
def test_custom_batch_parity(game, fuzz_seed, hip_lib, oracle_lib):
    """1 027 generated states (a ragged last block for the wave-per-env step kernel, both Breakout render kernel families and the
    state-reading SpaceInvaders rasteriser): the records read back, every frame in every format at the engine's own split and at forced
    ones, 300 batch steps with auto-reset, then the loop entry points, which such an engine runs in stream order."""
    from toybox_amd import hip
    n = 1027
    es = g, o = _engines(game, n, (hip_lib, oracle_lib))
    H, W = g.height, g.width
    chks = {}
    for ev in rule_inputs.custom_batch(es, n, game, fuzz_seed, steps=300):
        if ev[0] == "written":
            _assert_stream_order(g, "after the write")
            _same_states(es, "records read back")                            # (a)
        elif ev[0] == "frames":                                              # (b)
            ch, want = ev[1], ev[2][0]
            chk = FrameChecker((H, W, ch))
            for split in (0, 1, 2, 7, 16):
                g.set_option(_abi.OPT_RENDER_SPLIT, split)
                g.render_device(0, ch)
                g.sync()
                p, nbytes = g.device_buffer(_abi.BUF_FRAME)
                assert nbytes >= n * H * W * ch
                chk.compare(device_frames(p, H * W * ch), lambda lo, hi, out: np.copyto(out, want[lo:hi]), n,
                            what="%s channels %d split %d" % (game, ch, split))
            g.set_option(_abi.OPT_RENDER_SPLIT, 0)
        elif ev[0] == "step":                                                # (c)
            t = ev[1]
            for x, y, name in zip(ev[2][0], ev[2][-1], ("reward", "done", "lives", "score")):
                assert np.array_equal(x, y), "%s differs at step %d (envs %s)" % (name, t, np.flatnonzero(x != y)[:8])
            if t % 50 == 49:
                ch = (3, 1, 4)[(t // 50) % 3]
                chk = chks.setdefault(ch, FrameChecker((H, W, ch)))
                _device_frames_equal(g, o, chk, ch, "%s step %d channels %d" % (game, t, ch))
    _same_states(es, "after 300 steps")
    _assert_stream_order(g, "after 300 steps")
    s = hip.Stream()                                                         # (d)
    fb = H * W * 3
    chk = FrameChecker((H, W, 3))
    t = 300

    def step_oracle(t, got_packed, what):
        o.step_synthetic(1337, t, auto_reset=True)
        assert np.array_equal(got_packed, read_buffer(o, _abi.BUF_PACKED, (n,), np.uint64)), what

    for _ in range(20):
        g.step_synthetic(1337, t, auto_reset=True, stream=s.ptr)
        step_oracle(t, read_buffer(g, _abi.BUF_PACKED, (n,), np.uint64, stream=s), "step_synthetic t=%d" % t)
        t += 1
    for _ in range(6):
        g.render_step_synthetic(1337, t, channels=3, auto_reset=True, stream=s.ptr)
        s.synchronize()
        p, nbytes = g.device_buffer(_abi.BUF_FRAME)
        assert nbytes >= n * fb
        chk.compare(device_frames(p, fb), oracle_frames(o, 3), n, what="render_step_synthetic t=%d" % t)
        step_oracle(t, read_buffer(g, _abi.BUF_PACKED, (n,), np.uint64, stream=s), "render_step_synthetic t=%d" % t)
        t += 1
    for _ in range(2):
        g.rollout_synthetic(1337, t, 3, channels=3, auto_reset=True, stream=s.ptr)
        s.synchronize()
        f, nbytes = g.device_buffer(_abi.BUF_ROLLOUT_FRAMES)
        assert nbytes == 3 * n * fb
        packed = read_buffer(g, _abi.BUF_ROLLOUT_PACKED, (3, n), np.uint64, stream=s)
        for j in range(3):
            chk.compare(device_frames(f + j * n * fb, fb), oracle_frames(o, 3), n, n=n, frame0=j * n, what="rollout_synthetic t=%d" % (t + j))
            step_oracle(t + j, packed[j], "rollout_synthetic t=%d" % (t + j))
        t += 3
    _assert_stream_order(g, "after the loop entry points")
    g.sync()
    _same_states(es, "at the end")
    s.close()
    _close(es)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [13106, 13107])
def test_custom_breakout_rgb_render_at_the_two_part_threshold(n, fuzz_seed, hip_lib, oracle_lib):
    """Custom brick tables on both sides of the size from which Breakout's RGB launch goes out in two parts (32 768 blocks): one part
    with staggered first waves, and two parts with the seam between envs 1 023 and 1 024; records written by the wave-per-env step
    kernel over a 40-step pre-roll."""
    es = g, o = _engines("breakout", n, (hip_lib, oracle_lib), preroll=0)
    _write_all(es, generate("breakout", o, np.random.default_rng(fuzz_seed)))
    for t in range(40):
        for e in es:
            e.step_synthetic(1337, t, auto_reset=True)
    _assert_stream_order(g, "n=%d" % n)
    _device_frames_equal(g, o, FrameChecker((g.height, g.width, 3), pinned=True), 3, "custom breakout n=%d" % n)
    _close(es)


# ---------------------------------------------------------------- 3. the flip inside a running loop form

FLIP_CASES = [("breakout", 4099, form) for form in ("pipeline", "fused", "chunks3", "chunks4")] + \
             [("space_invaders", 2051, form) for form in ("pipeline", "chunks3", "chunks4")]       # (SpaceInvaders has no fused form)


@pytest.mark.gpu
@pytest.mark.parametrize("game,n,form", FLIP_CASES)
def test_flip_inside_a_running_loop_form(game, n, form, fuzz_seed, hip_lib, oracle_lib):
    """An overlapped loop form on a caller's stream: four calls, then -- without a sync -- one non-canonical state written into env
    n - 2, which ends the form; four more of the same calls, a new game for every env (the engine stays in its written-state mode), two
    more.  Each call's whole frame buffer and step records are copied device-side right behind it (addresses re-queried after every
    call); all of it, and the states at the end, against the oracle."""
    from toybox_amd import hip
    es = g, o = _engines(game, n, (hip_lib, oracle_lib), seed=33)
    one = one_generated_state(game, o, fuzz_seed)
    k = 3 if form.startswith("chunks") else 1
    if form == "pipeline":
        g.set_option(_abi.OPT_PIPELINE, _abi.PIPELINE_OVERLAP_RENDERS)
        own, active = _abi.OPT_PIPELINE_ACTIVE, _abi.PIPELINE_OVERLAP_RENDERS
    elif form == "fused":
        g.set_option(_abi.OPT_FUSED_OVERLAP, _abi.FUSED_OVERLAP_ON)
        own, active = _abi.OPT_FUSED_OVERLAP_ACTIVE, 1
    else:
        g.set_option(_abi.OPT_ROLLOUT_CHUNKS, int(form[-1]))
        own, active = _abi.OPT_ROLLOUT_CHUNKS_ACTIVE, 1
    assert g.get_option(own) == active
    H, W = g.height, g.width
    fb = H * W * 3
    calls, t0 = 10, 30
    s = hip.Stream()
    hold_f, hold_p = hip.malloc(calls * k * n * fb), hip.malloc(calls * k * n * 8)
    try:
        for c in range(calls):
            t = t0 + c * k
            if c == 4:
                g.set_state(n - 2, one)
                _assert_stream_order(g, "after the write")
            if c == 8:
                g.new_game()
                _assert_stream_order(g, "after the new game")
            if form == "pipeline":
                g.step_synthetic(1337, t, auto_reset=True, stream=s.ptr)
                g.render_device(0, 3, stream=s.ptr)
            elif form == "fused":
                g.render_step_synthetic(1337, t, channels=3, auto_reset=True, stream=s.ptr)
            else:
                g.rollout_synthetic(1337, t, k, channels=3, auto_reset=True, stream=s.ptr)
            f, nbytes = g.device_buffer(_abi.BUF_ROLLOUT_FRAMES if k > 1 else _abi.BUF_FRAME)
            assert nbytes >= k * n * fb
            hip.memcpy_dtod_async(hold_f + c * k * n * fb, f, k * n * fb, s)
            p, nbytes = g.device_buffer(_abi.BUF_ROLLOUT_PACKED if k > 1 else _abi.BUF_PACKED)
            assert nbytes == k * n * 8
            hip.memcpy_dtod_async(hold_p + c * k * n * 8, p, k * n * 8, s)
        s.synchronize()
        g.sync()
        packed = np.empty((calls * k, n), np.uint64)
        hip.memcpy_dtoh(packed, hold_p, packed.nbytes)
        chk = FrameChecker((H, W, 3), pinned=True)
        for c in range(calls):
            if c == 4:
                o.set_state(n - 2, one)
            if c == 8:
                o.new_game()
            for j in range(k):
                q = c * k + j

                def frames():
                    chk.compare(device_frames(hold_f + q * n * fb, fb), oracle_frames(o, 3), n, n=n, frame0=q * n,
                                what="%s n=%d %s, call %d frame %d" % (game, n, form, c, j))
                if form != "pipeline":
                    frames()                                                 # (the frame of the state the step starts from)
                o.step_synthetic(1337, t0 + q, auto_reset=True)
                assert np.array_equal(packed[q], read_buffer(o, _abi.BUF_PACKED, (n,), np.uint64)), (c, j)
                if form == "pipeline":
                    frames()
    finally:
        hip.free(hold_f)
        hip.free(hold_p)
    _same_states(es, "at the end")
    for x, y in zip(g.scalars(), o.scalars()):
        assert np.array_equal(x, y)
    s.close()
    _close(es)


# ---------------------------------------------------------------- 4. the agent layer on custom Breakout

@pytest.mark.gpu
@pytest.mark.parametrize("new_plane", [0, 2])
@pytest.mark.parametrize("variant", ["a", "b"])
def test_agent_layer_on_custom_breakout(variant, new_plane, fuzz_seed, hip_lib, oracle_lib):
    """No reset-time wrappers, 1 027 envs, 400 agent steps through the generic path (single-frame steps with snapshots, the render
    kernels with CUSTOM = true and a per-env choice of record array, agent_warp_kernel, the monitor kernel's plain new game)."""
    es = _engines("breakout", 1027, (hip_lib, oracle_lib))
    agent_on_custom_breakout(es, variant, new_plane, fuzz_seed)
    _close(es)


@pytest.mark.gpu
@pytest.mark.parametrize("new_plane", [0, 2])
def test_fork_of_a_custom_env_after_the_flip_equals_replay(new_plane, fuzz_seed, hip_lib, oracle_lib):
    """TBX_EDIT_COPY_ENV on an engine whose agent layer was initialised canonical and then left the fused path: the selected envs become
    copies of custom envs.  The yardstick is replay (tests/fork_replay.py): a checker engine whose env i was seeded, written and driven
    like env src[i]."""
    game, n, t_flip, t_fork, t_end = "breakout", 130, 6, 30, 42
    seeds = (99 + 11 * np.arange(n)).astype(np.uint32)
    src = (7 * np.arange(n) + 1) % n | 1                                     # odd envs: the ones with a written table
    src[src >= n] = 1
    mask = np.arange(n) % 3 != 0
    eff = effective(src, mask)

    def make(lib, env_map):
        e = Engine(game, n, lib=lib)
        e.seed_array(seeds[env_map])
        e.new_game()
        e.agent_init(new_plane=new_plane, **AGENT)
        return e

    ident = np.arange(n)
    g, o, r = make(hip_lib, ident), make(oracle_lib, ident), make(oracle_lib, eff)
    run_agent([g, o], game, 0, t_flip)
    run_agent([r], game, 0, t_flip, env_map=eff)
    written = half_custom(o, np.random.default_rng(fuzz_seed))
    _write_all([g, o], written)
    _write_all([r], written[eff])
    run_agent([g, o], game, t_flip, t_fork)
    run_agent([r], game, t_flip, t_fork, env_map=eff)
    g.fork(src, mask)
    assert np.array_equal(states_bytes(g), states_bytes(r)) and np.array_equal(sim_rngs(g), sim_rngs(r))
    run_agent([g, r], game, t_fork, t_end, env_map=eff)
    _same_states([g, r], "after the fork and %d steps" % (t_end - t_fork))
    _same_rngs([g, r], "simulator RNG after the fork")
    _close([g, o, r])


@pytest.mark.gpu
@pytest.mark.parametrize("new_plane", [0, 2])
def test_flip_under_reset_time_wrappers_is_refused_and_changes_nothing(new_plane, fuzz_seed, hip_lib, oracle_lib):
    """With episodic-life / fire-reset / no-op resets configured, the agent step after a custom write returns TBX_E_UNSUPPORTED and
    leaves the states and the observation buffers as they were."""
    game, n = "breakout", 64
    g, o = _engines(game, n, (hip_lib, oracle_lib), preroll=0)
    g.agent_init(skip=4, out_h=84, out_w=84, stack=4, episodic_life=True, fire_reset=True, noop_max=4, new_plane=new_plane)
    g.agent_reset()
    for t in range(5):
        g.agent_step(synthetic_actions(game, n, t, seed=7))
    g.set_state(3, one_generated_state(game, o, fuzz_seed))
    which, shape = (_abi.BUF_AGENT_RING, (4, n, 84, 84)) if new_plane == 2 else (_abi.BUF_AGENT_OBS, (n, 84, 84, 4))

    def snapshot():
        return states_bytes(g), sim_rngs(g), read_buffer(g, which, shape), read_buffer(g, _abi.BUF_AGENT_PLANE, (n, 84, 84)) if new_plane else None

    before = snapshot()
    with pytest.raises(ToyboxAmdError) as ei:
        g.agent_step(synthetic_actions(game, n, 5, seed=7))
    assert ei.value.code == _abi.E_UNSUPPORTED
    for x, y in zip(before, snapshot()):
        assert x is y or np.array_equal(x, y)
    _close([g, o])


# ---------------------------------------------------------------- 5. directed Amidar states

def run_directed_amidar(es):
    """rule_inputs.directed_amidar_run on one engine or two; -> (the directed states, the checker's states after 6 frames)"""
    early = []
    for ev in rule_inputs.directed_amidar_run(es, es[0].n_envs):
        if ev[0] == "written":
            start = ev[1]
            _same_states(es, "records read back")
        elif ev[0] == "step":
            for x, y, name in zip(ev[2][0], ev[2][-1], ("reward", "done", "lives", "score")):
                assert np.array_equal(x, y), "%s differs at step %d (envs %s)" % (name, ev[1], np.flatnonzero(x != y)[:8])
            if ev[1] == 5:
                early.append(es[-1].get_states_np())
        elif ev[0] == "states":
            _same_states(es, "after 200 frames")
        elif ev[0] == "frames":
            assert np.array_equal(ev[2][0], ev[2][-1]), ev[1]
    return start, early[0]


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2])
def test_directed_amidar_enemy_arms(form, hip_lib, oracle_lib):
    """64 envs on either form of the step kernel (thread per env, wavefront per env)"""
    es = g, o = _engines("amidar", 64, (hip_lib, oracle_lib), preroll=0, options=[(_abi.OPT_STEP_FORM, form)])
    run_directed_amidar(es)
    chk = FrameChecker((g.height, g.width, 3))
    _device_frames_equal(g, o, chk, 3, "directed amidar form %d" % form)
    _close(es)


# ---------------------------------------------------------------- the twins: generators and loops over the checker alone

def test_breakout_generator_reaches_the_brick_code(fuzz_seed, oracle_lib):
    """192 envs (48 of each kind), 400 frames: in kinds 0 and 1 at least 12 envs score from a brick of their table, in kind 2 no score
    moves, in kind 3 at least 5 envs level up, and at least one game finishes.  (A finished game restarts on the canonical wall: an
    env counts for its kind up to there.)"""
    n = 192
    o, = _engines("breakout", n, (oracle_lib,))
    rng = np.random.default_rng(fuzz_seed)
    st = gen_breakout(o.get_states_np(), rng)
    o.set_states_np(0, st)
    back = o.get_states_np()
    past = np.arange(_abi.BRK_MAX_BRICKS)[None, :] >= back["n_bricks"][:, None]
    assert (st["n_bricks"] < 256).any() and not back["bricks"][past].tobytes().strip(b"\0")      # slots past n_bricks read back as zeros
    kind = np.arange(n) % 4
    own = np.ones(n, bool)                         # still on the written table
    scored, levelled = np.zeros(n, bool), np.zeros(n, bool)
    moved = np.zeros(n, bool)
    finished = [0]
    level = [o.scalars()[2].copy()]
    score0 = st["score"].copy()
    score = [score0]

    def watch(t, out, e):
        _, done, _, sc = out                       # (the first reward after a write is the written score minus the one before: not a hit)
        lv = e.scalars()[2]
        scored[:] |= own & ~done & (sc > score[0])
        levelled[:] |= own & ~done & (lv > level[0])
        moved[:] |= own & ~done & (sc != score0)
        level[0], score[0] = lv.copy(), sc.copy()
        own[:] &= ~done
        finished[0] += int(done.sum())

    run_steps([o], "breakout", 400, watch=watch)
    per_kind = lambda flags: [int(flags[kind == k].sum()) for k in range(4)]
    print("scored %s, levelled %s, finished %d" % (per_kind(scored), per_kind(levelled), finished[0]))
    assert per_kind(scored)[0] >= 12 and per_kind(scored)[1] >= 12, per_kind(scored)
    assert own[kind == 2].all() and not moved[kind == 2].any(), "an all-indestructible table scored or ended its game"
    assert per_kind(levelled)[3] >= 5, per_kind(levelled)
    assert finished[0] >= 1
    o.close()


def test_si_generator_reaches_the_written_state_code(fuzz_seed, oracle_lib):
    """The run of test_custom_batch_parity (1 027 envs, 300 frames) on the checker: an env written with n_enemies == 0 levels up, and
    an enemy laser flying LEFT or RIGHT leaves the frame."""
    game, n = "space_invaders", 1027
    o, = _engines(game, n, (oracle_lib,))
    st = generate(game, o, np.random.default_rng(fuzz_seed))
    o.set_states_np(0, st)
    assert set(SI_N_ENEMIES) <= set(st["n_enemies"].tolist()) and (st["n_shields"] < 3).any()
    empty = st["n_enemies"] == 0
    own = np.ones(n, bool)
    prev = {"st": o.get_states_np()}
    seen = {"level": 0, "left": 0, "right": 0}

    def watch(t, out, e):
        cur, was = e.get_states_np(), prev["st"]
        seen["level"] += int((own & empty & ~out[1] & (cur["level"] > was["level"])).sum())
        # a laser that moved this frame (the world is not frozen: no get-ready phase, no explosion, the ship alive) and whose new
        # rectangle lies outside the 320 columns
        ran = (was["life_display_timer"] == 0) & (was["ship_death_counter"] < 0) & (was["ship_alive"] != 0)
        L = was["enemy_lasers"]
        slot = np.arange(_abi.SI_MAX_LASERS)[None, :] < was["n_enemy_lasers"][:, None]
        seen["left"] += int((ran[:, None] & slot & (L["movement"] == 2) & (L["x"] - L["speed"] + L["w"] <= 0)).sum())
        seen["right"] += int((ran[:, None] & slot & (L["movement"] == 3) & (L["x"] + L["speed"] >= 320)).sum())
        own[:] &= ~out[1]
        prev["st"] = cur

    run_steps([o], game, 300, watch=watch)
    print(seen)
    assert seen["level"] >= 1, "no env written with n_enemies == 0 levelled up"
    assert seen["left"] + seen["right"] >= 1, "no sideways laser left the frame"
    o.close()


@pytest.mark.parametrize("variant", ["a", "b"])
def test_agent_loop_on_custom_breakout_ends_games_on_the_checker(variant, fuzz_seed, oracle_lib):
    es = _engines("breakout", 64, (oracle_lib,))
    print("dones %d, episodes %d" % agent_on_custom_breakout(es, variant, 0, fuzz_seed))
    _close(es)


def test_directed_amidar_states_take_their_arms_on_the_checker(oracle_lib):
    """after six frames: the bottom-row walker went LEFT, the left-column one UP, the one off the perimeter moved (LEFT: the first open
    direction of its fallback order between two junctions of row 12), and every dead-end enemy turned back"""
    es = _engines("amidar", 64, (oracle_lib,), preroll=0)
    start, early = run_directed_amidar(es)
    calm = start["chase_timer"] == 0
    x0, y0, x1, y1 = (s["enemies"][f][calm] for s in (start, early) for f in ("x", "y"))
    assert (x1[:, 0] < x0[:, 0]).all() and (y1[:, 0] == y0[:, 0]).all()
    assert (y1[:, 1] < y0[:, 1]).all() and (x1[:, 1] == x0[:, 1]).all()
    assert ((x1[:, 2] != x0[:, 2]) | (y1[:, 2] != y0[:, 2])).all()
    assert (x1[:, 3] < x0[:, 3]).all()
    assert (x1[:, 4] > x0[:, 4]).all()
    assert (y1[:, 5] < y0[:, 5]).all()
    _close(es)
