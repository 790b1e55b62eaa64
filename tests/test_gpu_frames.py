"""Every frame of every env, on the rasteriser's launch forms where a sampled check can miss a seam (tests/support.py FrameChecker:
the whole device output against the oracle's frames of the same envs, slice by slice, np.array_equal):

* rollout chunks (TBX_OPT_ROLLOUT_CHUNKS) -- a launch per frame and one launch for a chunk's k x n frames, whose span launches cut
  at 65 536 frames, paint frames as if they were envs (frame f = env f % n of step j0 + f / n), go out in two parts when they
  start on an idle lane and in one part behind the previous chunk's launch;
* the batched render (tbx_render_device) on both sides of each size at which the rasteriser's launch form changes;
* Breakout's fused render + step launch (step blocks in front of the rasteriser's, the other records buffer), in stream order and
  overlapped on two lanes with two frame buffers, including the call right after a state write.

Sizes come from the launch code: Breakout's RGB launch has ten waves per frame and goes out in two parts (1 024 envs, then the
rest) from 32 768 blocks of four waves, i.e. from 13 107 frames; tbx_stagger_first_waves acts from 16 384 blocks (6 554 RGB
frames); Breakout gray / RGBA take 4 / 2 / 1 waves per frame up to 8 192 / 32 768 / more frames; SpaceInvaders RGBA 5 waves up to
32 768 envs, gray 4 up to 4 096; Amidar gray 4 up to 4 096; GridWorld RGB 5 waves from 16 384 envs."""
import numpy as np
import pytest

from support import FrameChecker, device_frames, oracle_frames
from toybox_amd import Engine, _abi


def _pair(game, n, hip_lib, oracle_lib, seed=1234):
    g, o = Engine(game, n, lib=hip_lib), Engine(game, n, lib=oracle_lib)
    for e in (g, o):
        e.seed(seed)
        e.new_game()
    return g, o


def _preroll(g, o, steps, t=0, seed=1337):
    for _ in range(steps):
        g.step_synthetic(seed, t, auto_reset=True)
        o.step_synthetic(seed, t, auto_reset=True)
        t += 1
    return t


def _same_end(g, o, n):
    g.sync()
    for i in sorted({0, 1, 1023 % n, 1024 % n, n // 2, n - 1} | set(range(0, n, max(1, n // 40)))):
        assert bytes(g.get_state(i)) == bytes(o.get_state(i)), i
    for x, y in zip(g.scalars(), o.scalars()):
        assert np.array_equal(x, y)


# game, channels, n, k, TBX_OPT_ROLLOUT_CHUNKS, K-step record ring
ROLLOUT_CASES = [
    ("breakout", 3, 3000, 22, 4, False),      # spans of 21 x 3 000 = 63 000 frames (the first one in two parts) + 3 000; 3 000 % 64 != 0
    ("breakout", 3, 13107, 3, 3, False),      # a launch per frame, each in two parts
    ("breakout", 3, 13107, 3, 4, False),      # one span of 39 321 frames
    ("breakout", 3, 13106, 3, 3, False),      # a launch per frame, one part with staggered first waves
    ("breakout", 4, 4096, 17, 4, False),      # a span of exactly 65 536 frames, then one of 4 096
    ("breakout", 3, 700, 3, 1, True),         # partial last block; the engine's choice under a ring
    ("space_invaders", 3, 5000, 4, 4, False),
    ("space_invaders", 1, 900, 3, 1, False),  # gray: four waves per frame
]


@pytest.mark.gpu
@pytest.mark.parametrize("game,channels,n,k,form,ring", ROLLOUT_CASES)
def test_rollout_chunks_every_frame(game, channels, n, k, form, ring, hip_lib, oracle_lib):
    """Two chunks back to back on the caller's stream (the second chunk's span launch starts behind the first one's), the first
    chunk's whole frame buffer copied device-side right behind it, then a chunk after a join (a state write) that starts on an idle
    engine: every frame of every step of every env against the oracle's k single calls (render, step, and under a ring a gather)."""
    from toybox_amd import hip
    g, o = _pair(game, n, hip_lib, oracle_lib, seed=33)
    H, W = g.height, g.width
    fb = H * W * channels
    cb = k * n * fb
    t = _preroll(g, o, 30)
    g.set_option(_abi.OPT_ROLLOUT_CHUNKS, form)
    if ring:
        for e in (g, o):
            e.set_option(_abi.OPT_GATHER_EVERY, k)
            e.gather_init(1, 0, e.gather_unique_id())
    assert g.get_option(_abi.OPT_ROLLOUT_CHUNKS_ACTIVE) == 1
    chk = FrameChecker((H, W, channels), pinned=True)
    s = hip.Stream()

    def chunk(t0):
        g.rollout_synthetic(1337, t0, k, channels=channels, auto_reset=True, stream=s.ptr)
        f, nb = g.device_buffer(_abi.BUF_ROLLOUT_FRAMES)
        assert nb == cb
        return f

    def check(ptr, t0, what):
        for j in range(k):
            chk.compare(device_frames(ptr + j * n * fb, fb), oracle_frames(o, channels), n, n=n, frame0=j * n,
                        what="%s %s n=%d form %d, chunk from t=%d" % (what, game, n, form, t0))
            o.step_synthetic(1337, t0 + j, auto_reset=True)
            if ring:
                o.gather()

    hold = hip.malloc(cb)
    try:
        f1 = chunk(t)
        hip.memcpy_dtod_async(hold, f1, cb, s)
        f2 = chunk(t + k)
        s.synchronize()
        g.sync()
        assert f1 != f2
        check(hold, t, "first chunk")
        check(f2, t + k, "second chunk (behind the first)")
        t += 2 * k
        st = o.get_state(n // 3)
        for e in (g, o):
            e.set_state(n - 2, st)
        f3 = chunk(t)
        s.synchronize()
        g.sync()
        check(f3, t, "chunk after a join")
    finally:
        hip.free(hold)
    _same_end(g, o, n)
    s.close()
    g.close(); o.close()


# game, channels, n: both sides of each launch-form threshold of the batched render
RENDER_CASES = [
    ("breakout", 3, 6553), ("breakout", 3, 6554),            # staggered first waves from 16 384 blocks
    ("breakout", 3, 13106), ("breakout", 3, 13107),          # two parts from 32 768 blocks
    ("breakout", 1, 8192), ("breakout", 1, 8193), ("breakout", 1, 32768), ("breakout", 1, 32769),
    ("breakout", 4, 8192), ("breakout", 4, 8193), ("breakout", 4, 32768), ("breakout", 4, 32769),
    ("space_invaders", 4, 32768), ("space_invaders", 4, 32769),
    ("space_invaders", 1, 4096), ("space_invaders", 1, 4097),
    ("amidar", 1, 4096), ("amidar", 1, 4097),
    ("gridworld", 3, 16383), ("gridworld", 3, 16384),
    ("breakout", 3, 65536),                                  # the benchmark's batch
]


@pytest.mark.gpu
@pytest.mark.parametrize("game,channels,n", RENDER_CASES)
def test_batched_render_every_env_at_launch_thresholds(game, channels, n, hip_lib, oracle_lib):
    """tbx_render_device after a 40-step pre-roll: every env's frame equals the oracle's."""
    g, o = _pair(game, n, hip_lib, oracle_lib, seed=61)
    _preroll(g, o, 40)
    g.render_device(0, channels)
    g.sync()
    p, nbytes = g.device_buffer(_abi.BUF_FRAME)
    fb = g.height * g.width * channels
    assert nbytes >= n * fb
    FrameChecker((g.height, g.width, channels), pinned=True).compare(device_frames(p, fb), oracle_frames(o, channels), n,
                                                                    what="%s n=%d channels %d" % (game, n, channels))
    g.close(); o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20000, 4099])
@pytest.mark.parametrize("overlap", [_abi.FUSED_OVERLAP_ON, _abi.FUSED_OVERLAP_OFF])
def test_fused_render_step_every_env(overlap, n, hip_lib, oracle_lib):
    """Breakout's fused render + step launch (brk_render_step_kernel_w5): six consecutive calls on the caller's stream, each call's
    whole frame buffer copied device-side right behind it; a state write before the third call leaves the records stale.
    Overlapped (option 1), consecutive calls alternate between two frame buffers: both are checked."""
    from toybox_amd import hip
    game, channels, T, write_at = "breakout", 3, 6, 2
    g, o = _pair(game, n, hip_lib, oracle_lib, seed=5)
    g.set_option(_abi.OPT_FUSED_OVERLAP, overlap)
    assert g.get_option(_abi.OPT_FUSED_OVERLAP_ACTIVE) == (1 if overlap == _abi.FUSED_OVERLAP_ON else 0)
    H, W = g.height, g.width
    fb = H * W * channels
    t0 = _preroll(g, o, 30)
    st = o.get_state(n // 5)
    s = hip.Stream()
    hold = hip.malloc(T * n * fb)
    addr = []
    try:
        for t in range(T):
            if t == write_at:
                g.set_state(7, st)
            g.render_step_synthetic(1337, t0 + t, channels=channels, auto_reset=True, stream=s.ptr)
            f, _ = g.device_buffer(_abi.BUF_FRAME)
            addr.append(f)
            hip.memcpy_dtod_async(hold + t * n * fb, f, n * fb, s)
        s.synchronize()
        g.sync()
        if overlap == _abi.FUSED_OVERLAP_ON:
            assert len(set(addr)) == 2 and all(addr[t] != addr[t - 1] for t in range(write_at + 1, T)), addr
        chk = FrameChecker((H, W, channels), pinned=True)
        for t in range(T):
            if t == write_at:
                o.set_state(7, st)
            chk.compare(device_frames(hold + t * n * fb, fb), oracle_frames(o, channels), n, n=n, frame0=t * n,
                        what="fused call %d (overlap option %d, n=%d)" % (t, overlap, n))
            o.step_synthetic(1337, t0 + t, auto_reset=True)
    finally:
        hip.free(hold)
    _same_end(g, o, n)
    s.close()
    g.close(); o.close()
