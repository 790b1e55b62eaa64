"""Every picture path under palettes other than the default one, and in states in which the draw order shows.

The default colours hide most of what a painter can get wrong: every background is black, Breakout's paddle and ball share one
colour, the HUD's colour is the frame's, every alpha is 255, SpaceInvaders' per-env ship and shield colours are never written.
tests/palettes.py builds two palettes per game (DISTINCT: every field a colour of its own in r, g, b and gray, no channel 0 or
255, alphas from {0, 1, 128, 254}; GRAY_TIES: pairs that differ in RGB and share a gray byte, one pair equal in RGB) and, on
mid-game records, the overlaps that make the draw order visible (a ball on the paddle, on a side wall, in a brick row, on another
ball; Amidar's player on an enemy, two enemies, a mover on a painted tile and on a painted box's interior; SpaceInvaders' lasers in a
shield and in the ship, the ship dying).  257 envs (ragged for 64 and 256), one for the resident kernel.  The expectation is the
CPU oracle under the same config and calls, every byte of every env's frame (support.FrameChecker).

Paths (the letters of the cases below):
 a  tbx_render_device, channels 1, 3, 4: all four games; Breakout on the canonical wall and on per-env brick tables; SpaceInvaders
    through the record painter (records rebuilt after the write, then step-written) and through the state-reading rasteriser
    (off-grid formations) -- and, g, tbx_set_config with another palette between the calls, without a new game
 b  tbx_render_step_synthetic, channels 3 and 4, Breakout, in stream order and with TBX_OPT_FUSED_OVERLAP
 c  tbx_rollout_synthetic, Breakout and SpaceInvaders, in both forced chunk forms; TBX_OPT_PIPELINE 2 and 3
 d  tbx_step_begin with a frame, tbx_render into host memory, tbx_render_env
 e  tbx_step1_frame on a one-env engine (the resident kernel), channels 1, 3, 4, across a restart of the kernel and a tbx_set_config
 f  the agent step: new_plane 0 and 2, TBX_OPT_AGENT_GENERIC 0 and 1 (the ALT instantiations of the rasterisers), 84 x 84 and
    50 x 97, every wrapper on, 12 steps -- and, g, another palette between the steps, 4 more.  Breakout keeps its ROWS across that
    switch: other rows under running games put a device engine on per-env brick tables, where the reset-time wrappers are not
    available (include/toybox_amd.h, tbx_set_config); the rows' switch has cases of its own -- without wrappers, with a new game
    behind it under every wrapper, and the refusal itself (TBX_E_UNSUPPORTED, nothing changed, a new game recovers)

Launch forms folded, because they share the call that carries the palette:
 * Breakout's two-part RGB launch from 13 107 envs: both parts are the same instantiation with the same BrkPalette argument,
   `BRK_LAUNCH` inside `launch_part` (toybox_amd/csrc/breakout.hip, `if (two_parts) { launch_part(0, HEAD_ENVS); launch_part(HEAD_ENVS,
   count - HEAD_ENVS); }`); they differ in bit 16 of split_arg (no staggered first waves) alone;
 * TBX_OPT_RENDER_SPLIT: the palette goes through pix_of<C>() once per wave whatever the split (breakout.hip `c_bg = pix_of<C>(pal.bg)`,
   amidar.hip and space_invaders.hip alike); tests/test_gpu_custom_states.py walks the splits;
 * the rollout chunk's span launch and its per-frame launches end in the same launch_render<C> / launch_rec_render as path a
   (breakout.hip rollout_render / rollout_render_span, space_invaders.hip alike); both forms are run all the same (path c);
 * a custom Breakout wall under b and c: such an engine runs those entry points in stream order, i.e. as path a's launches
   (BreakoutOps::pipeline_ok, `!custom && ...`).

The cases without the gpu mark are the twins: the same drivers with the CPU checker standing where the device does, plus the
conditions on the inputs (every palette entry on the screen of at least 8 envs at every compared step, every overlap in at least 4
envs at the first) and a second formulation in numpy over the oracle alone (remap onto the default palette, gray = luma of RGB,
RGBA = RGB + 255, observation = area average of the maximum of two gray frames, the pixel on top of each overlap).

What the first run found is in profiles/palettes.md.
"""
import ctypes as C

import numpy as np
import pytest

import palettes as P
from support import (FrameChecker, agent_stack_frames, area_resize_int, device_frames, engine_is_oracle, host_frames,
                     oracle_frames, read_buffer, synthetic_actions)
from toybox_amd import Engine, _abi
from toybox_amd._lib import ToyboxAmdError

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
N = P.N_ENVS
SHOWN_FLOOR, OVERLAP_FLOOR = 8, 4


@pytest.fixture(params=["oracle", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request, oracle_lib):
    if request.param == "oracle":
        return oracle_lib
    return request.getfixturevalue("hip_lib")


def hip_only(cases):
    """parameters for (lib, ...) through the lib fixture: the device alone (cases whose twin would repeat another twin)"""
    return [pytest.param("hip", *c, marks=pytest.mark.gpu) for c in cases]


def both(cases):
    return [pytest.param("oracle", *c) for c in cases] + hip_only(cases)


_CHK = {}


def checker(e, ch):
    key = (e.height, e.width, ch)
    if key not in _CHK:
        _CHK[key] = FrameChecker(key)
    return _CHK[key]


def buffer_frames(e, ptr, fb):
    return host_frames(ptr, fb) if engine_is_oracle(e) else device_frames(ptr, fb)


def array_frames(a):
    return lambda lo, hi, out: np.copyto(out, a[lo:hi])


def code_of(call):
    try:
        call()
    except ToyboxAmdError as err:
        return err.code
    return _abi.OK


def close(es):
    for e in es:
        e.close()


class Hold:
    """frames copied aside right behind the call that produced them (device-side on the caller's stream; plain memory for the
    checker), so that calls go out back to back and everything is compared afterwards"""

    def __init__(self, e, nbytes):
        self.oracle = engine_is_oracle(e)
        if self.oracle:
            self.keep = np.empty(nbytes, np.uint8)
            self.ptr = self.keep.ctypes.data
        else:
            from toybox_amd import hip
            self.ptr = hip.malloc(nbytes)

    def copy(self, offset, src, nbytes, stream):
        if self.oracle:
            C.memmove(self.ptr + offset, src, nbytes)
        else:
            from toybox_amd import hip
            hip.memcpy_dtod_async(self.ptr + offset, src, nbytes, stream)

    def close(self):
        if not self.oracle:
            from toybox_amd import hip
            hip.free(self.ptr)


class Run:
    """the engine under test g beside the oracle o under one palette; as a twin (g is the checker too) it also asserts the
    conditions on the inputs, on the oracle's frames"""

    def __init__(self, game, name, variant, lib, oracle_lib, options=(), n=N):
        self.game, self.name, self.oracle_lib = game, name, oracle_lib
        self.pal = P.palette(game, name)
        self.g, self.o = self.es = P.palette_engines(game, name, variant, (lib, oracle_lib), oracle_lib, n=n, options=options)
        self.twin = engine_is_oracle(self.g)
        self.n = n
        self.stream = None
        self.first = True

    def open_stream(self):
        if not self.twin:
            from toybox_amd import hip
            self.stream = hip.Stream()
        return self.stream.ptr if self.stream else 0

    def wait(self):
        if self.stream:
            self.stream.synchronize()
        self.g.sync()

    def close(self):
        if self.stream:
            self.g._lib.tbx_sync(self.g._h)
            self.stream.close()
        close(self.es)

    def conditions(self, what):
        """on the oracle's state as it stands: every entry of the palette in force (after a switch: palettes.palette_in_force) in
        at least 8 envs' frames; at the first compared frame every overlap in at least 4 envs"""
        if not self.twin:
            return
        shown = P.shown_counts(self.game, self.pal, self.o.render(3))
        low = {r: c for r, c in shown.items() if c < min(SHOWN_FLOOR, self.n)}
        assert not low, "%s: palette entries on too few envs' frames: %r" % (what, low)
        if self.first and self.n == N:
            counts = P.OVERLAP_COUNTS[self.game](self.o.get_states_np())
            assert set(counts) == set(P.OVERLAPS[self.game])
            low = {k: c for k, c in counts.items() if c < OVERLAP_FLOOR}
            assert not low, "%s: overlaps in too few envs: %r" % (what, low)
        self.first = False

    def compare(self, ptr, ch, what, nbytes=None):
        """n frames at ptr (memory of g's library) against the oracle's frames of its current state"""
        fb = self.g.height * self.g.width * ch
        if nbytes is not None:
            assert nbytes >= self.n * fb, (what, nbytes)
        checker(self.g, ch).compare(buffer_frames(self.g, ptr, fb), oracle_frames(self.o, ch), self.n, what=what)

    def render_device(self, what, channels=(1, 3, 4)):
        for ch in channels:
            self.g.render_device(0, ch, stream=self.stream.ptr if self.stream else 0)
            self.wait()
            p, nbytes = self.g.device_buffer(_abi.BUF_FRAME)
            self.compare(p, ch, "%s channels %d" % (what, ch), nbytes)
        self.conditions(what)

    def step_both(self, t):
        for e in self.es:
            e.step_synthetic(P.ACTION_SEED, t, auto_reset=True)

    def same_packed(self, got, what):
        want = read_buffer(self.o, _abi.BUF_PACKED, (self.n,), np.uint64)
        assert np.array_equal(got, want), "%s: step records differ in envs %s" % (what, np.flatnonzero(got != want)[:8])

    def switch_palette(self, keep_wall=False):
        """another palette between calls, no new game: tbx_set_config (SpaceInvaders, whose colours are per-env state: a state
        write of the colour fields alone)"""
        if self.game == "space_invaders":
            st = self.o.get_states_np()
            P.si_write_palette(st, P.palette(self.game, "OTHER"))
            for e in self.es:
                e.set_states_np(0, st)
            self.pal = P.palette(self.game, "OTHER")
            return
        for e in self.es:
            e.set_config(P.other_config(e, self.game, keep_wall))
        self.pal = P.palette_in_force(self.game, self.pal, keep_wall)      # (the conditions go on, against what is in force now)


# ================================================================ the palettes themselves

@pytest.mark.parametrize("game", GAMES)
def test_palettes_have_their_properties(game):
    """DISTINCT: pairwise distinct in r, g, b and gray, no channel 0 or 255, no black, alphas from {0, 1, 128, 254} (asserted where
    the palette is built); SpaceInvaders: the ship's and the shields' colours differ from each other and from env to env.
    GRAY_TIES: the named pairs differ in RGB and share a gray byte, one pair is equal in RGB."""
    d, t = P.palette(game, "DISTINCT"), P.palette(game, "GRAY_TIES")
    flat = np.stack([np.asarray(c).reshape(-1, 4)[0] for c in d.values()])
    P.assert_distinct(flat)
    assert 255 not in np.concatenate([np.asarray(c).reshape(-1, 4)[:, 3] for pal in (d, t) for c in pal.values()])
    pairs = {"breakout": (("paddle_color", "ball_color"), ("frame_color", "bg_color"), ("row0", "row1")),
             "amidar": (("painted_color", "inner_painted_color"), ("player_color", "enemy_color"), ("bg_color", "unpainted_color")),
             "gridworld": (("tile0", "player_color"), None, ("tile2", "tile3")),
             "space_invaders": (("ship", "shield0"), ("shield1", "enemy_laser0"), ("shield1", "shield2"))}[game]
    for tie in pairs[:2]:
        if tie:
            a, b = (np.asarray(t[r]).reshape(-1, 4) for r in tie)
            assert (P.luma(a[:, :3]) == P.luma(b[:, :3])).all() and (a[:, :3] != b[:, :3]).any(axis=1).all(), tie
    a, b = (np.asarray(t[r]).reshape(-1, 4) for r in pairs[2])
    assert np.array_equal(a[:, :3], b[:, :3]), pairs[2]


# ================================================================ a + g. tbx_render_device

CASES_A = [(g, v, name) for g in GAMES for v in P.VARIANTS[g] for name in ("DISTINCT", "GRAY_TIES")]


@pytest.mark.parametrize("game,variant,name", CASES_A)
def test_render_device_under_palettes(game, variant, name, lib, oracle_lib):
    """channels 1, 3, 4 of every env: at the written states (SpaceInvaders: records rebuilt from the state, or the state-reading
    rasteriser), after each of three steps (step-written records), then -- another palette through tbx_set_config, no new game --
    at once and after two more steps.  Breakout's bricks keep the colour they were made with until their env's next game, so
    the wall of a running game shows the old rows under the new frame, paddle and ball."""
    r = Run(game, name, variant, lib, oracle_lib)
    what = "%s %s %s" % (game, variant, name)
    r.render_device(what + " written")
    for t in range(3):
        r.step_both(t)
        r.render_device("%s step %d" % (what, t))
    r.switch_palette()
    r.render_device(what + " after the palette switch")
    for t in range(3, 5):
        r.step_both(t)
        r.render_device("%s step %d, switched" % (what, t))
    if not r.twin:
        assert np.array_equal(np.frombuffer(r.g.get_states(), np.uint8), np.frombuffer(r.o.get_states(), np.uint8)), what
    r.close()


# ================================================================ b. tbx_render_step_synthetic (Breakout)

@pytest.mark.parametrize("lib,channels,overlap", both([(3, _abi.FUSED_OVERLAP_OFF), (4, _abi.FUSED_OVERLAP_OFF)]) +
                         hip_only([(3, _abi.FUSED_OVERLAP_ON), (4, _abi.FUSED_OVERLAP_ON)]), indirect=["lib"])
def test_fused_render_step_under_palette(lib, channels, overlap, oracle_lib):
    """six fused render + step launches back to back on a caller's stream, in stream order and overlapped on two lanes; every
    call's frame (the state the step starts from) copied aside behind it, the step records read behind it"""
    r = Run("breakout", "DISTINCT", "canonical", lib, oracle_lib, options=[(_abi.OPT_FUSED_OVERLAP, overlap)])
    g, o, n = r.g, r.o, r.n
    if not r.twin:
        assert g.get_option(_abi.OPT_RENDER_STEP_FUSED) == 1
        assert g.get_option(_abi.OPT_FUSED_OVERLAP_ACTIVE) == (1 if overlap == _abi.FUSED_OVERLAP_ON else 0)
    sp = r.open_stream()
    calls, fb = 6, g.height * g.width * channels
    hold, packed = Hold(g, calls * n * fb), []
    try:
        for c in range(calls):
            g.render_step_synthetic(P.ACTION_SEED, c, channels=channels, auto_reset=True, stream=sp)
            p, nbytes = g.device_buffer(_abi.BUF_FRAME)
            assert nbytes >= n * fb
            hold.copy(c * n * fb, p, n * fb, r.stream)
            packed.append(read_buffer(g, _abi.BUF_PACKED, (n,), np.uint64, stream=r.stream))
        r.wait()
        for c in range(calls):
            what = "breakout fused channels %d overlap %d call %d" % (channels, overlap, c)
            r.compare(hold.ptr + c * n * fb, channels, what)
            r.conditions(what)
            o.step_synthetic(P.ACTION_SEED, c, auto_reset=True)
            r.same_packed(packed[c], what)
    finally:
        hold.close()
    r.render_device("breakout fused, at the end", channels=(channels,))
    r.close()


# ================================================================ c. tbx_rollout_synthetic and the pipelined loop

ROLLOUT_CASES = [(g, form, ch) for g in ("breakout", "space_invaders") for form in (_abi.ROLLOUT_CHUNKS_PER_FRAME, _abi.ROLLOUT_CHUNKS_SPAN)
                 for ch in (3, 4)]


@pytest.mark.parametrize("lib,game,form,channels", both(ROLLOUT_CASES[:1] + ROLLOUT_CASES[4:5]) + hip_only(ROLLOUT_CASES), indirect=["lib"])
def test_rollout_chunks_under_palette(lib, game, form, channels, oracle_lib):
    """two chunks of three frames in each forced chunk form (a rasteriser launch per frame on two lanes; one per chunk): every
    frame of the chunk and its step records"""
    r = Run(game, "DISTINCT", None, lib, oracle_lib, options=[(_abi.OPT_ROLLOUT_CHUNKS, form)])
    g, o, n = r.g, r.o, r.n
    if not r.twin:
        assert g.get_option(_abi.OPT_ROLLOUT_CHUNKS_ACTIVE) == 1
    sp = r.open_stream()
    k, fb = 3, g.height * g.width * channels
    for t0 in (0, k):
        g.rollout_synthetic(P.ACTION_SEED, t0, k, channels=channels, auto_reset=True, stream=sp)
        r.wait()
        f, nbytes = g.device_buffer(_abi.BUF_ROLLOUT_FRAMES)
        assert nbytes == k * n * fb
        packed = read_buffer(g, _abi.BUF_ROLLOUT_PACKED, (k, n), np.uint64)
        for j in range(k):
            what = "%s rollout form %d channels %d frame %d" % (game, form, channels, t0 + j)
            r.compare(f + j * n * fb, channels, what)
            r.conditions(what)
            o.step_synthetic(P.ACTION_SEED, t0 + j, auto_reset=True)
            r.same_packed(packed[j], what)
    r.render_device("%s rollout, at the end" % game, channels=(channels,))
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("game", ["breakout", "space_invaders"])
@pytest.mark.parametrize("mode", [_abi.PIPELINE_STEP_BESIDE_RENDER, _abi.PIPELINE_OVERLAP_RENDERS])
def test_pipelined_loop_under_palette(mode, game, hip_lib, oracle_lib):
    """step + render on a caller's stream in pipelined modes 2 and 3 (the step of frame t + 1 beside the rasteriser of frame t,
    records in two buffers): six frames, RGB, copied aside behind each call"""
    r = Run(game, "DISTINCT", None, hip_lib, oracle_lib, options=[(_abi.OPT_PIPELINE, mode)])
    g, o, n = r.g, r.o, r.n
    assert g.get_option(_abi.OPT_PIPELINE_ACTIVE) == mode
    sp = r.open_stream()
    calls, fb = 6, g.height * g.width * 3
    hold = Hold(g, calls * n * fb)
    try:
        for c in range(calls):
            g.step_synthetic(P.ACTION_SEED, c, auto_reset=True, stream=sp)
            g.render_device(0, 3, stream=sp)
            p, nbytes = g.device_buffer(_abi.BUF_FRAME)
            assert nbytes >= n * fb
            hold.copy(c * n * fb, p, n * fb, r.stream)
        r.wait()
        for c in range(calls):
            o.step_synthetic(P.ACTION_SEED, c, auto_reset=True)
            r.compare(hold.ptr + c * n * fb, 3, "%s pipeline %d frame %d" % (game, mode, c))
    finally:
        hold.close()
    r.close()


# ================================================================ d. frames delivered to the host

@pytest.mark.parametrize("game", GAMES)
def test_host_frames_under_palette(game, lib, oracle_lib):
    """tbx_step_begin with a frame (the picture of the state the step leaves) in each format, tbx_render into host memory,
    tbx_render_env of one env of every overlap class and the last env"""
    r = Run(game, "DISTINCT", None, lib, oracle_lib)
    g, o, n = r.g, r.o, r.n
    checker(g, 3).compare(array_frames(g.render(3)), oracle_frames(o, 3), n, what="%s tbx_render of the written states" % game)
    r.conditions("%s written" % game)
    for t, ch in enumerate((3, 1, 4)):
        a = synthetic_actions(game, n, t, seed=P.ACTION_SEED)
        frame = g.host_array((n, g.height, g.width, ch))
        g.step_begin(a, auto_reset=True, frame=frame, channels=ch)
        g.step_end()
        o.step(a, auto_reset=True)
        what = "%s step_begin frame, channels %d" % (game, ch)
        checker(g, ch).compare(array_frames(frame), oracle_frames(o, ch), n, what=what)
        r.conditions(what)
        checker(g, ch).compare(array_frames(g.render(ch)), oracle_frames(o, ch), n, what="%s tbx_render channels %d" % (game, ch))
        for i in list(range(P.CLASSES)) + [n - 1]:
            assert np.array_equal(g.render_env(i, ch), o.render_env(i, ch)), "%s tbx_render_env(%d) channels %d" % (game, i, ch)
    r.close()


# ================================================================ e. the resident kernel

@pytest.mark.parametrize("game", GAMES)
def test_resident_kernel_frames_under_palette(game, lib, oracle_lib):
    """tbx_step1_frame on a one-env engine: the states of all eight overlap classes written in turn (each write stops the
    resident kernel; the next call starts it again), three frames each in the three formats, another entry point between two of
    them (a restart without a write), and tbx_set_config with another palette between two calls of one running game"""
    cfg, st = P.prepared(game, "DISTINCT", None, oracle_lib)
    g, o = es = P.palette_engines(game, "DISTINCT", None, (lib, oracle_lib), oracle_lib, n=1)
    t = 0
    for k in range(P.CLASSES):
        for e in es:
            e.set_states_np(0, st[k:k + 1])
        for ch in (3, 1, 4):
            if k == 3 and ch == 1:                      # (the two frames that follow show the running game under the new config)
                for e in es:
                    e.set_config(P.other_config(e, game, keep_wall=False))
            a = int(synthetic_actions(game, 1, t, seed=P.ACTION_SEED + k)[0])
            got, want = g.step1_frame(0, a, ch, auto_reset=True), o.step1_frame(0, a, ch, auto_reset=True)
            assert got[:4] == want[:4], (game, k, t)
            assert np.array_equal(got[4], want[4]), "%s class %d frame %d channels %d: %d bytes differ" % (game, k, t, ch, (got[4] != want[4]).sum())
            if ch == 1:
                assert [list(x) for x in g.scalars()] == [list(x) for x in o.scalars()]           # (stops the kernel)
            t += 1
    close(es)


# ================================================================ f + g. the agent step

AGENT = dict(skip=4, stack=4, clip_reward=True, episodic_life=True, fire_reset=True, noop_max=7, noop_seed=17)
OUTPUTS = (("reward", _abi.BUF_AGENT_REWARD, np.float32), ("done", _abi.BUF_AGENT_DONE, np.uint8),
           ("ep_done", _abi.BUF_AGENT_EP_DONE, np.uint8))
GEOMETRIES = ((84, 84), (50, 97))
AGENT_CASES = [(g, plane, generic, geo, "DISTINCT") for g in GAMES for plane in (0, 2) for generic in (0, 1) for geo in GEOMETRIES] + \
              [(g, plane, 0, GEOMETRIES[0], "GRAY_TIES") for g in GAMES for plane in (0, 2)]


def agent_run(r, wrappers, geo, plane, steps, switch_at, keep_wall, what, t0=0):
    """agent steps t0 .. steps - 1 on both engines, another palette before step switch_at (-1: none)"""
    g, o, n = r.g, r.o, r.n
    chk = FrameChecker((geo[0], geo[1], 4))
    for t in range(t0, steps):
        if t == switch_at:
            r.switch_palette(keep_wall=keep_wall)
        for e in r.es:
            e.agent_step_synthetic(P.ACTION_SEED, t)
        rc, rc_o = code_of(g.sync), code_of(o.sync)
        where = "%s agent step %d" % (what, t)
        assert rc == rc_o, (where, rc, rc_o)
        for name, which, dt in OUTPUTS:
            x, y = read_buffer(g, which, (n,), dt), read_buffer(o, which, (n,), dt)
            assert np.array_equal(x, y), "%s: %s differs in envs %s" % (where, name, np.flatnonzero(x != y)[:8])
        chk.compare(agent_stack_frames(g), agent_stack_frames(o), n, what=where)
        r.conditions(where)


def agent_engines(game, name, plane, generic, geo, wrappers, lib, oracle_lib):
    """the agent layer first, then the mid-game states (a reset would play them away): tests/test_gpu_agent_scale.py's order.
    On the fused path the records go in as they are: most of them hold fewer lives than the reset left, EpisodicLifeEnv
    reports done, and some envs lose another life inside the reset procedure that follows -- the observation kernels then paint
    from the copies kept aside for that step ("A life lost inside FireResetEnv.reset's step(2)").  The generic path
    has no such copy and is documented there to show another picture in that case, which is no matter of colours: its cases
    write the same records with the lives the reset left, so that the write itself ends no life."""
    r = Run(game, name, None, lib, oracle_lib, options=[(_abi.OPT_AGENT_GENERIC, generic)])
    cfg, st = P.prepared(game, name, None, oracle_lib)
    for e, mode in ((r.g, plane), (r.o, 0)):
        e.agent_init(out_h=geo[0], out_w=geo[1], new_plane=mode, **wrappers)
        e.agent_reset()
    if generic and "lives" in st.dtype.names:
        st = st.copy()
        st["lives"] = r.o.scalars()[1]
    for e in r.es:
        e.set_states_np(0, st)
    # the conditions on the overlaps hold at the written states: an agent step's picture is the maximum of the frames three and
    # four frames later, which shows of them what the rules leave (a ball inside a brick has broken it by then)
    r.conditions("%s agent, written" % game)
    return r


@pytest.mark.parametrize("lib,game,plane,generic,geo,name", both([c for c in AGENT_CASES if c[2] == 0]) +
                         hip_only([c for c in AGENT_CASES if c[2] == 1]), indirect=["lib"])
def test_agent_step_under_palettes(lib, game, plane, generic, geo, name, oracle_lib):
    """every wrapper on, 12 agent steps from the prepared states, then another palette (tbx_set_config, no new game) and 4 more.
    Breakout switches the four colours the config alone holds and keeps its rows: other rows under running games take a device
    engine to its per-env brick tables, on which the reset-time wrappers are not available (include/toybox_amd.h, tbx_set_config)
    -- the device answers TBX_E_UNSUPPORTED where the oracle goes on.  That refusal is
    test_breakout_rows_switched_under_wrappers_is_refused_until_a_new_game, the rows' change without wrappers
    test_breakout_rows_switched_under_the_agent_layer, with a new game behind it test_breakout_rows_switched_with_a_new_game.  Compared:
    reward, done, episode end and the whole stack of every env at every step; the rolled stack and the ring of planes, the
    fused observation kernels and (TBX_OPT_AGENT_GENERIC) the two gray renders with the generic warp"""
    r = agent_engines(game, name, plane, generic, geo, AGENT, lib, oracle_lib)
    what = "%s %s plane %d generic %d %dx%d" % ((game, name, plane, generic) + geo)
    agent_run(r, AGENT, geo, plane, 16, 12, True, what)
    r.close()


@pytest.mark.parametrize("plane", [0, 2])
def test_breakout_rows_switched_under_the_agent_layer(plane, lib, oracle_lib):
    """tbx_set_config with other ROW colours between agent steps, no reset-time wrapper on: the bricks on the screen keep their
    colours (they are state), the next wall takes the new ones -- 4 steps before, 8 after"""
    wrappers = dict(AGENT, episodic_life=False, fire_reset=False, noop_max=0)
    r = agent_engines("breakout", "DISTINCT", plane, 0, GEOMETRIES[0], wrappers, lib, oracle_lib)
    agent_run(r, wrappers, GEOMETRIES[0], plane, 12, 4, False, "breakout rows switched, plane %d" % plane)
    r.close()


@pytest.mark.parametrize("plane", [0, 2])
def test_breakout_rows_switched_with_a_new_game(plane, lib, oracle_lib):
    """write_config_json + new_game under the training set-up: every wrapper on, 4 agent steps, tbx_set_config with other rows AND
    other config colours, tbx_new_game for every env, 6 agent steps, tbx_agent_reset, 4 more -- all held to the oracle.  (The
    device engine is on its brick tables between the two calls and canonical again behind the new game: with wrappers on, an
    agent step or reset on the tables would be refused.)"""
    r = agent_engines("breakout", "DISTINCT", plane, 0, GEOMETRIES[0], AGENT, lib, oracle_lib)
    what = "breakout rows switched + new game, plane %d" % plane
    agent_run(r, AGENT, GEOMETRIES[0], plane, 4, -1, False, what)
    for e in r.es:
        e.set_config(P.other_config(e, "breakout", keep_wall=False))
        e.new_game()
    r.pal = dict(P.palette("breakout", "OTHER"))                   # every wall on the screen is a new one
    agent_run(r, AGENT, GEOMETRIES[0], plane, 10, -1, False, what, t0=4)
    for e in r.es:
        e.agent_reset()
    FrameChecker((84, 84, 4)).compare(agent_stack_frames(r.g), agent_stack_frames(r.o), r.n, what=what + ", agent_reset")
    agent_run(r, AGENT, GEOMETRIES[0], plane, 14, -1, False, what, t0=10)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("plane", [0, 2])
def test_breakout_rows_switched_under_wrappers_is_refused_until_a_new_game(plane, hip_lib, oracle_lib):
    """Other rows under running games with a reset-time wrapper on: the device engine is on its per-env brick tables, where the
    in-kernel resets do not exist, so tbx_agent_step* and tbx_agent_reset return TBX_E_UNSUPPORTED and change nothing (the states
    and the stacks are the oracle's, which has not stepped) -- until a tbx_new_game for every env, after which the steps equal the
    oracle's again.  The header says so under tbx_set_config."""
    r = agent_engines("breakout", "DISTINCT", plane, 0, GEOMETRIES[0], AGENT, hip_lib, oracle_lib)
    what = "breakout rows switched under wrappers, plane %d" % plane
    agent_run(r, AGENT, GEOMETRIES[0], plane, 3, -1, False, what)
    for e in r.es:
        e.set_config(P.other_config(e, "breakout", keep_wall=False))
    g, o, n = r.g, r.o, r.n
    assert code_of(lambda: (g.agent_step_synthetic(P.ACTION_SEED, 3), g.sync())) == _abi.E_UNSUPPORTED
    assert code_of(g.agent_reset) == _abi.E_UNSUPPORTED
    assert np.array_equal(np.frombuffer(g.get_states(), np.uint8), np.frombuffer(o.get_states(), np.uint8)), what
    FrameChecker((84, 84, 4)).compare(agent_stack_frames(g), agent_stack_frames(o), n, what=what + ", after the refusals")
    r.render_device(what + ", old rows under the new colours", channels=(3,))
    for e in r.es:
        e.new_game()
    agent_run(r, AGENT, GEOMETRIES[0], plane, 9, -1, False, what, t0=3)
    r.close()


# ================================================================ the second formulation: numpy over the oracle alone

VARIANT_CASES = [(g, v) for g in GAMES for v in P.VARIANTS[g]]
SI_FIXED = ((0, 0, 0), (134, 134, 29), (151, 25, 122), (80, 89, 22), (50, 132, 50))


def _keys(rgb):
    c = rgb.astype(np.uint32)
    return c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16)


@pytest.mark.parametrize("game,variant", VARIANT_CASES)
def test_distinct_frame_remapped_equals_default_frame(game, variant, oracle_lib):
    """the RGB frame under DISTINCT, mapped colour by colour onto the default palette (many to one), is the frame of the same
    states under the default palette; colours no palette entry names (SpaceInvaders' enemies, UFO, ground and HUD, the black
    outside GridWorld's board) map to themselves"""
    pal = P.palette(game, "DISTINCT")
    (o,) = P.palette_engines(game, "DISTINCT", variant, (oracle_lib,), oracle_lib)
    got = o.render(3)
    o.close()
    cfg, st, rgb = P.default_twin(game, "DISTINCT", variant, oracle_lib)
    with Engine(game, N, lib=oracle_lib) as d:
        if cfg is not None:
            d.set_config(cfg)
        d.seed(P.SEED)
        d.new_game()
        d.set_states_np(0, st)
        want = d.render(3)
    keys = _keys(got)
    out = keys.copy()
    fixed = {r | (g << 8) | (b << 16) for r, g, b in SI_FIXED}
    for role, c in pal.items():
        c = np.broadcast_to(np.asarray(c, np.uint32), (N, 4))
        k = c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16)
        assert not set(k.tolist()) & fixed, role
        to = np.uint32(rgb[role][0] | (rgb[role][1] << 8) | (rgb[role][2] << 16))
        out[keys == k[:, None, None]] = to
    bad = np.flatnonzero((out != _keys(want)).reshape(N, -1).any(axis=1))
    assert not len(bad), "%s %s: the remapped frame differs in %d envs, first %s" % (game, variant, len(bad), bad[:8])


@pytest.mark.parametrize("name", ["DISTINCT", "GRAY_TIES"])
@pytest.mark.parametrize("game,variant", VARIANT_CASES)
def test_gray_is_luma_and_rgba_is_rgb_plus_255(game, variant, name, oracle_lib):
    """gray = (77 r + 150 g + 29 b + 128) >> 8 of the RGB frame; RGBA = RGB with 255 behind it, whatever alpha the palette holds --
    at the written states and two steps on"""
    (o,) = P.palette_engines(game, name, variant, (oracle_lib,), oracle_lib)
    for t in range(3):
        rgb, gray, rgba = o.render(3), o.render(1), o.render(4)
        assert np.array_equal(gray[..., 0], P.luma(rgb)), (game, variant, name, t)
        assert np.array_equal(rgba[..., :3], rgb) and (rgba[..., 3] == 255).all(), (game, variant, name, t)
        o.step_synthetic(P.ACTION_SEED, t, auto_reset=True)
    o.close()


@pytest.mark.parametrize("geo", GEOMETRIES)
@pytest.mark.parametrize("game", GAMES)
def test_observation_is_the_area_average_of_the_max_of_two_gray_frames(game, geo, oracle_lib):
    """skip 4, no reset-time wrapper, nobody near the end of their game: the newest plane of the observation is
    support.area_resize_int of the maximum of the gray frames after the third and the fourth frame of the step"""
    cfg, st = P.prepared(game, "DISTINCT", None, oracle_lib)
    a_eng, raw = P.palette_engines(game, "DISTINCT", None, (oracle_lib, oracle_lib), oracle_lib)
    a_eng.agent_init(skip=4, out_h=geo[0], out_w=geo[1], stack=4, clip_reward=False)
    for e in (a_eng, raw):
        if game != "gridworld":
            e.edit(_abi.EDIT_SET_LIVES, [5])
    for t in range(3):
        a = synthetic_actions(game, N, t, seed=P.ACTION_SEED)
        obs, _, done = a_eng.agent_step(a)
        gray = []
        over = np.zeros(N, bool)
        for f in range(4):
            over |= raw.step(a)[1]
            gray.append(raw.render(1)[..., 0])
        keep = ~over & ~done                                    # (GridWorld reaches its goal inside a step now and then)
        assert keep.sum() >= N // 2
        want = area_resize_int(np.maximum(gray[2], gray[3]), geo[0], geo[1])
        assert np.array_equal(obs[keep][..., 3], want[keep]), (game, geo, t)
        if over.any():
            break
    close([a_eng, raw])


def _at(rgb, env, x, y):
    return tuple(int(v) for v in rgb[env, y, x])


def _rgb(c):
    return tuple(int(v) for v in np.asarray(c)[:3])


def test_breakout_draw_order_on_the_oracle(oracle_lib):
    """bricks, then the paddle, then the balls, then the HUD in the frame's colour: the pixel on top of each overlap"""
    pal = P.palette("breakout", "DISTINCT")
    cfg, st = P.prepared("breakout", "DISTINCT", None, oracle_lib)
    (o,) = P.palette_engines("breakout", "DISTINCT", None, (oracle_lib,), oracle_lib)
    rgb = o.render(3)
    o.close()
    ball, paddle, frame, bg = (_rgb(pal[f]) for f in ("ball_color", "paddle_color", "frame_color", "bg_color"))
    for i in range(N):
        k = i % P.CLASSES
        bx, by = int(st["ball_x"][i, 0]), int(st["ball_y"][i, 0])
        if k == 0:
            assert _at(rgb, i, bx, by) == ball and _at(rgb, i, bx, int(st["paddle_y"][i]) + 1) == ball, i
            assert _at(rgb, i, int(st["paddle_x"][i]) - 10, int(st["paddle_y"][i]) + 1) == paddle, i
        elif k == 1:
            assert _at(rgb, i, bx, by) == ball and _at(rgb, i, bx, by + 4) == frame, i
        elif k == 2:
            assert _at(rgb, i, bx, by) == ball, i
        elif k == 3:
            assert _at(rgb, i, bx, by) == ball and _at(rgb, i, int(st["ball_x"][i, 1]), int(st["ball_y"][i, 1])) == ball, i
        hud = {tuple(c) for c in rgb[i, :13].reshape(-1, 3).tolist()}
        assert hud == {frame, bg}, (i, hud)
    written = np.arange(N) % P.CLASSES == 4                          # the class written for the HUD: every glyph, lives and level too
    digits = P.hud_digits(st)
    assert set(digits[written].reshape(-1).tolist()) == set(range(10))
    assert len(set(digits[written, 5].tolist())) >= 5 and len(set(digits[written, 6].tolist())) >= 5
    assert P.hud_full(st)[written].all() and not P.hud_full(st)[~written].any()


def test_amidar_draw_order_on_the_oracle(oracle_lib):
    """inner box, track, enemies in index order, the player, the HUD in the player's colour: at pixels chosen from the records --
    the player's centre, the middle of what two enemies share, the last column and row of the mover on a painted box's corner and
    the interior pixel beside it -- the frame holds the colour palettes.amidar_pixel derives from the record by that order, and
    each of those pixels decides between two colours in at least 4 envs"""
    pal = P.palette("amidar", "DISTINCT")
    cfg, st = P.prepared("amidar", "DISTINCT", None, oracle_lib)
    (o,) = P.palette_engines("amidar", "DISTINCT", None, (oracle_lib,), oracle_lib)
    rgb = o.render(3)
    o.close()
    player, enemy, bg, inner = (_rgb(pal[f]) for f in ("player_color", "enemy_color", "bg_color", "inner_painted_color"))
    seen = {"player over enemy": 0, "enemy over enemy": 0, "enemy over inner": 0, "inner beside the mover": 0}
    for i in range(N):
        k = i % P.CLASSES
        px, py = 16 + int(st["player"]["x"][i]) // 16 + 2, 37 + int(st["player"]["y"][i]) // 16 + 2
        assert _at(rgb, i, px, py) == player == P.amidar_pixel(st, i, px, py, pal), i
        if k == 0:
            ex, ey = 16 + int(st["enemies"]["x"][i, 0]) // 16 + 2, 37 + int(st["enemies"]["y"][i, 0]) // 16 + 2
            assert (ex, ey) == (px, py), i                          # the enemy lies under that pixel
            seen["player over enemy"] += 1
        elif k == 1:
            x = 16 + int(st["enemies"]["x"][i, 1]) // 16 + 1         # enemy 1 is two pixels right of enemy 2: both cover this one
            y = 37 + int(st["enemies"]["y"][i, 1]) // 16 + 2
            want = P.amidar_pixel(st, i, x, y, pal)
            assert _at(rgb, i, x, y) == want and want in (enemy, player), i
            seen["enemy over enemy"] += want == enemy
        elif k == 3:
            x, y = 16 + int(st["enemies"]["x"][i, 3]) // 16 + 4, 37 + int(st["enemies"]["y"][i, 3]) // 16 + 5
            for qx, qy in ((x, y), (x + 1, y), (x + 1, y + 1), (x, y + 2)):
                want = P.amidar_pixel(st, i, qx, qy, pal)
                assert _at(rgb, i, qx, qy) == want, (i, qx, qy, want)
            seen["enemy over inner"] += P.amidar_pixel(st, i, x, y, pal) == enemy
            seen["inner beside the mover"] += P.amidar_pixel(st, i, x + 1, y, pal) == inner
        hud = {tuple(c) for c in rgb[i, 204:214].reshape(-1, 3).tolist()}
        assert hud == {player, bg}, (i, hud)
    assert min(seen.values()) >= OVERLAP_FLOOR, seen


def test_space_invaders_draw_order_on_the_oracle(oracle_lib):
    """shields, enemies, the ship in its own colour (alive or dying), then the lasers in theirs"""
    pal = P.palette("space_invaders", "DISTINCT")
    cfg, st = P.prepared("space_invaders", "DISTINCT", None, oracle_lib)
    (o,) = P.palette_engines("space_invaders", "DISTINCT", None, (oracle_lib,), oracle_lib)
    rgb = o.render(3)
    o.close()
    for i in range(N):
        k = i % P.CLASSES
        lasers = {_rgb(pal["enemy_laser%d" % q][i]) for q in range(8)}
        l0 = st["enemy_lasers"][i, 0]
        if k == 0:
            assert _at(rgb, i, int(l0["x"]), int(l0["y"]) + 2) in lasers, i
            sh = (i // P.CLASSES) % 3
            on_top = lasers | {_rgb(pal["ship_laser"][i]), (134, 134, 29)}          # (what is painted after the shields)
            assert _at(rgb, i, int(st["shield_x"][i, sh]) + 1, int(st["shield_y"][i, sh]) + 1) in on_top | {_rgb(pal["shield%d" % sh][i])}, i
        elif k == 1:
            assert _at(rgb, i, int(st["ship_x"][i]) + 7, int(st["ship_y"][i]) + 1) in lasers, i
            assert _at(rgb, i, int(st["ship_x"][i]) + 3, int(st["ship_y"][i]) + 4) == _rgb(pal["ship"][i]), i
        elif k == 2:
            assert _at(rgb, i, int(st["ship_x"][i]) + 4, int(st["ship_y"][i]) + 7) == _rgb(pal["ship"][i]), i
        elif k == 3:
            sl = st["ship_laser"][i]
            assert _at(rgb, i, int(sl["x"]), int(sl["y"]) + 2) == _rgb(pal["ship_laser"][i]), i
