"""Helpers shared by the test-suite (host-side numpy restatements of tiny pure functions)."""
import functools
from fractions import Fraction

import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)

LEGAL = {
    "breakout": [0, 1, 3, 4],
    "amidar": [0, 1, 2, 3, 4, 5],
    "space_invaders": [0, 1, 3, 4, 11, 12],
    "gridworld": [0, 2, 3, 4, 5],
}


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def synthetic_actions(game, n, t, seed=1337, env_offset=0):
    """a = legal[ splitmix64(seed ^ (env << 32) ^ t) mod n_legal ]  (same rule as tbx_step_synthetic)"""
    legal = np.asarray(LEGAL[game], dtype=np.int32)
    env = np.arange(env_offset, env_offset + n, dtype=np.uint64)
    h = splitmix64(np.uint64(seed) ^ (env << np.uint64(32)) ^ np.uint64(t))
    return legal[(h % np.uint64(len(legal))).astype(np.int64)]


def noop_count(noop_seed, global_env, episode_index, noop_max):
    """the engine's default no-op rule (include/toybox_amd.h, tbx_agent_init): 1 + splitmix64(seed ^ env << 32 ^ k) % noop_max"""
    return 1 + int(splitmix64(int(noop_seed) ^ (int(global_env) << 32) ^ int(episode_index)) % np.uint64(noop_max))


# ---------------------------------------------------------------- the observation resize (WarpFrame) by its definition
# include/toybox_amd.h, tbx_agent_config_t: an area average with exact rational weights, rounded half up.

def area_resize_exact(img, oh, ow):
    """INTER_AREA by its definition, in exact rational arithmetic, round half up."""
    H, W = img.shape
    out = np.zeros((oh, ow), np.uint8)
    for oy in range(oh):
        y0, y1 = Fraction(oy * H, oh), Fraction((oy + 1) * H, oh)
        for ox in range(ow):
            x0, x1 = Fraction(ox * W, ow), Fraction((ox + 1) * W, ow)
            acc = Fraction(0)
            sy = int(y0)
            while sy < y1:
                wy = min(y1, sy + 1) - max(y0, sy)
                sx = int(x0)
                while sx < x1:
                    acc += wy * (min(x1, sx + 1) - max(x0, sx)) * int(img[sy, sx])
                    sx += 1
                sy += 1
            mean = acc / ((y1 - y0) * (x1 - x0))
            out[oy, ox] = int(mean + Fraction(1, 2))      # floor(mean + 1/2)
    return out


@functools.lru_cache(maxsize=None)
def overlap_matrix(src, out):
    """M[o, s] = length of the overlap of output cell o with source pixel s, in units of 1/out source pixels (read-only)."""
    m = np.zeros((out, src), np.int64)
    for o in range(out):
        lo, hi = o * src, (o + 1) * src
        for s_ in range(lo // out, src):
            if s_ * out >= hi:
                break
            m[o, s_] = min(hi, (s_ + 1) * out) - max(lo, s_ * out)
    m.flags.writeable = False
    return m


def area_sums(img, oh, ow):
    """int64[..., oh, ow]: the weighted sums of the definition, sum = mean x H x W, for one image or a batch [..., H, W].
    The products run in binary64 (BLAS): every operand and partial sum is an integer below 255 H W < 2^25, so exact."""
    H, W = img.shape[-2:]
    my, mx = overlap_matrix(H, oh).astype(np.float64), overlap_matrix(W, ow).T.astype(np.float64)
    return np.rint(my @ np.asarray(img, np.float64) @ mx).astype(np.int64)


def area_resize_int(img, oh, ow):
    """The same definition from the integer sums (fast enough for whole rollouts; one image or a batch [..., H, W])."""
    H, W = img.shape[-2:]
    return ((area_sums(img, oh, ow) + (H * W) // 2) // (H * W)).astype(np.uint8)


# ---------------------------------------------------------------- the output geometries tbx_agent_init accepts
# include/toybox_amd.h, tbx_agent_config_t: 1 <= out <= frame, out_w <= 128, out_h * out_w <= 7056, and at most 8 source pixels
# per output pixel and axis, ceil(frame / out) + 1 <= 8 (else TBX_E_UNSUPPORTED).  Restated here, not read from either library.

FRAME_DIMS = {"breakout": (160, 240), "space_invaders": (210, 320), "amidar": (250, 160), "gridworld": (128, 160)}
AGENT_MAX_OUT_W, AGENT_MAX_OUT_PX, AGENT_MAX_TAPS = 128, 84 * 84, 8


def agent_range_violations(H, W, oh, ow):
    """the range limits (TBX_E_INVALID) this output geometry breaks, by name"""
    limits = {"out_h >= 1": oh >= 1, "out_w >= 1": ow >= 1, "out_h <= H": oh <= H, "out_w <= W": ow <= W,
              "out_w <= 128": ow <= AGENT_MAX_OUT_W, "out_h * out_w <= 7056": oh * ow <= AGENT_MAX_OUT_PX}
    return [k for k, ok in limits.items() if not ok]


def agent_taps_ok(H, W, oh, ow):
    """at most 8 source pixels per output pixel on each axis (else TBX_E_UNSUPPORTED); oh, ow >= 1"""
    return -(-H // oh) + 1 <= AGENT_MAX_TAPS and -(-W // ow) + 1 <= AGENT_MAX_TAPS


def agent_geometry_code(H, W, oh, ow):
    """what tbx_agent_init returns for this output geometry (other fields in range): 0, TBX_E_INVALID (-1), TBX_E_UNSUPPORTED (-4)"""
    if agent_range_violations(H, W, oh, ow):
        return -1
    return 0 if agent_taps_ok(H, W, oh, ow) else -4


def agent_geometry_ok(H, W, oh, ow):
    return agent_geometry_code(H, W, oh, ow) == 0


def agent_out_h_range(H, W, ow):
    """(smallest, largest) accepted out_h for this out_w, or None"""
    hs = [h for h in range(1, H + 1) if agent_geometry_ok(H, W, h, ow)]
    return (hs[0], hs[-1]) if hs else None


def agent_out_w_range(H, W, oh):
    """(smallest, largest) accepted out_w for this out_h, or None"""
    ws = [w for w in range(1, min(W, AGENT_MAX_OUT_W) + 1) if agent_geometry_ok(H, W, oh, w)]
    return (ws[0], ws[-1]) if ws else None


# ---------------------------------------------------------------- Amidar state edits of the wrapper corner cases
# Shared by tests/golden/make_wrapper_golden.py (applied through the reference env's write_state_json) and by
# tests/test_preproc.py (applied to the fused engine): inputs of the fixtures, not expected outputs.

def amidar_edit_last_lives(js, lives, jump_timer, perimeter_from_start):
    """every enemy parked on the player, a jump that runs out `jump_timer` frames from now: the life goes when the jump ends;
    with perimeter_from_start the enemies respawn ON the player's start tile and the next frame costs another life"""
    js["lives"], js["jump_timer"] = lives, jump_timer
    for en in js["enemies"]:
        en["position"] = dict(js["player"]["position"])
        en["step"] = None
        if perimeter_from_start:
            en["ai"] = {"EnemyPerimeterAI": {"start": {"tx": 31, "ty": 15}}}
    return js


# ---------------------------------------------------------------- mid-game states: a short window is to be full of events
# From a fresh reset a window of 30 to 100 frames (or 48 agent steps) ends no game in Breakout, SpaceInvaders or Amidar.  So every
# env starts from the state of a donor env that has played for a while, and every second env is on its last life
# (tests/test_gpu_agent_scale.py, tests/test_gpu_loop_events.py).  GridWorld ends games from a fresh reset by itself (0: no donor).
DONOR_ENVS, DONOR_SEED, DONOR_ACTION_SEED = 1024, 99, 7
DONOR_FRAMES = {"breakout": 400, "space_invaders": 600, "amidar": 600, "gridworld": 0}


def donor_records(game, oracle_lib, donors=DONOR_ENVS):
    """the state records of `donors` oracle envs after DONOR_FRAMES[game] raw auto-resetting frames (None: no donor)"""
    from toybox_amd import Engine
    if not DONOR_FRAMES[game]:
        return None
    with Engine(game, donors, lib=oracle_lib) as d:
        d.seed(DONOR_SEED)
        d.new_game()
        for t in range(DONOR_FRAMES[game]):
            d.step(synthetic_actions(game, donors, t, seed=DONOR_ACTION_SEED), auto_reset=True)
        return d.get_states_np()


def write_mid_game_states(engines, n, records):
    """env i of every engine gets donor record i % len(records), then every even env is put on its last life (a state write
    between steps, as in test_gpu_agent_pipeline_survives_state_writes); the simulator RNGs stay the envs' own, so no two envs
    play the same game"""
    from toybox_amd import _abi
    if records is None:
        return
    part = 8192                                                 # (the records are 14 KB each in Breakout: not 65 536 at once)
    for first in range(0, n, part):
        rec = records[np.arange(first, min(n, first + part)) % len(records)]
        for e in engines:
            e.set_states_np(first, rec)
    for e in engines:
        e.edit(_abi.EDIT_SET_LIVES, [1], mask=np.arange(n) % 2 == 0)


def read_buffer(engine, which, shape, dtype=np.uint8, stream=None):
    """host copy of an engine-owned buffer (TBX_BUF_*): device memory of the HIP library, plain memory of the CPU checker.
    stream (a toybox_amd.hip.Stream, the one the producing call named): the copy is queued on it right behind tbx_device_buffer and
    only that stream is waited for -- the reader of include/toybox_amd.h's contract, which leaves an overlapped form of the engine
    in force; without one the whole engine is synchronised first (tbx_sync, which also joins every internal stream)."""
    import ctypes as C
    ptr, nbytes = engine.device_buffer(which)
    out = np.empty(shape, dtype)
    assert out.nbytes == nbytes, (out.nbytes, nbytes)
    if hasattr(engine._lib, "orc_splitmix64"):
        C.memmove(out.ctypes.data, ptr, nbytes)
    elif stream is not None:
        from toybox_amd import hip
        hip.check(hip.runtime().hipMemcpyAsync(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), C.c_int(2), stream.handle),
                  "hipMemcpyAsync D2H")
        stream.synchronize()
    else:
        from toybox_amd import hip
        engine.sync()
        hip.memcpy_dtoh(out, ptr, nbytes)
    return out


def queue_read_buffer(engine, which, out, stream=None):
    """read_buffer without the wait: the copy of an engine-owned buffer (TBX_BUF_*) into `out` (a C-contiguous array of exactly
    the buffer's size; page-locked, or the copy is not asynchronous) is queued on `stream`, the one the producing call named,
    and the call returns -- the reader include/toybox_amd.h allows between a call and the next one on the handle.  `out` holds
    the result once the stream has been synchronised.  The CPU checker has nothing in flight: there the copy happens here."""
    import ctypes as C
    ptr, nbytes = engine.device_buffer(which)
    assert out.flags["C_CONTIGUOUS"] and out.nbytes == nbytes, (which, out.nbytes, nbytes)
    if hasattr(engine._lib, "orc_splitmix64"):
        C.memmove(out.ctypes.data, ptr, nbytes)
        return
    from toybox_amd import hip
    hip.check(hip.runtime().hipMemcpyAsync(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), C.c_int(2),
                                           stream.handle if stream is not None else None), "hipMemcpyAsync D2H")


# ---------------------------------------------------------------- what the engines choose by themselves (include/toybox_amd.h)
# TBX_OPT_PIPELINE = 1 resolves to this mode for (game, envs) without a gather; TBX_OPT_ROLLOUT_CHUNKS = 0 makes a chunk of
# tbx_rollout_synthetic(channels = 3) run as overlapped launches (1) or as single calls (0), (without a gather, under a K-step ring).
# tests/test_gpu_paths.py checks both tables against TBX_OPT_*_ACTIVE; tests/test_buffer_contract.py takes its large sizes from them.
ENGINES_CHOICE_PIPELINE = {("breakout", 1024): 0, ("breakout", 4096): 3, ("breakout", 16384): 0, ("space_invaders", 1024): 3,
                           ("space_invaders", 16384): 0, ("amidar", 4096): 0, ("gridworld", 4096): 0}
ENGINES_CHOICE_ROLLOUT_CHUNKS = {("breakout", 1024): (1, 0), ("breakout", 2048): (1, 1), ("breakout", 8192): (1, 1), ("breakout", 32768): (1, 1),
                                 ("breakout", 40000): (0, 0), ("space_invaders", 4096): (1, 1), ("space_invaders", 8192): (1, 1),
                                 ("space_invaders", 12000): (0, 0), ("amidar", 4096): (0, 0), ("gridworld", 4096): (0, 0)}


def stack_from_ring(ring, head):
    """uint8[stack][N][h][w] + the newest slot -> uint8[N][h][w][stack], oldest first (include/toybox_amd.h, new_plane = 2)"""
    k = ring.shape[0]
    return np.stack([ring[(head + 1 + c) % k] for c in range(k)], axis=-1)


# ---------------------------------------------------------------- whole-output frame checks
# A device frame buffer is compared with the oracle's frames of the same envs in slices of bounded size: one reused host array
# receives each device slice, another the oracle's (orc_render_envs paints just that env range), so a 10 GB chunk buffer never
# needs 10 GB of host memory.  uint8 frames and an exact oracle: equal means every byte.

FRAME_SLICE_BYTES = 384 << 20          # per host array; the two together stay under 1 GB


def bind_render_envs(lib):
    """orc_render_envs(engine, first, count, out, channels) of the oracle library (not part of the product ABI)"""
    import ctypes as C
    f = lib.orc_render_envs
    if f.argtypes is None:
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    return f


def oracle_render_envs(engine, first, count, out, channels):
    """envs first .. first + count - 1 of an oracle Engine into out[:count]"""
    assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.shape[0] >= count
    engine._check(bind_render_envs(engine._lib)(engine._h, int(first), int(count), out.ctypes.data, int(channels)))


def oracle_frames(engine, channels, first_env=0):
    """expected-frames source for FrameChecker.compare: frame f = env first_env + f of the oracle engine as it stands"""
    return lambda lo, hi, out: oracle_render_envs(engine, first_env + lo, hi - lo, out, channels)


def device_frames(ptr, frame_bytes):
    """frames-under-test source for FrameChecker.compare: frame f lies at device address ptr + f * frame_bytes"""
    def fetch(lo, hi, out):
        from toybox_amd import hip
        hip.memcpy_dtoh(out, ptr + lo * frame_bytes, (hi - lo) * frame_bytes)
    return fetch


def host_frames(ptr, frame_bytes):
    """source for FrameChecker.compare over plain memory (a buffer of the CPU checker): frame f lies at ptr + f * frame_bytes"""
    def fetch(lo, hi, out):
        import ctypes as C
        C.memmove(out.ctypes.data, ptr + lo * frame_bytes, (hi - lo) * frame_bytes)
    return fetch


def engine_is_oracle(engine):
    return hasattr(engine._lib, "orc_splitmix64")


def agent_stack_frames(engine):
    """source for FrameChecker.compare over shape (out_h, out_w, stack): frame f = the observation stack of env f as the engine
    holds it right now, whichever form it keeps -- TBX_BUF_AGENT_OBS as it lies there, or (new_plane = 2) TBX_BUF_AGENT_RING read
    through tbx_agent_ring_head the way include/toybox_amd.h states it (stack_from_ring, slice by slice: channel c of env i is
    ring[(head + 1 + c) % stack][i]).  The caller has synchronised whatever wrote the buffers."""
    import ctypes as C
    from toybox_amd import _abi
    n, oh, ow, stack = engine._agent_shape
    px = oh * ow
    if engine_is_oracle(engine):
        def copy(dst, src, nbytes):
            C.memmove(dst.ctypes.data, src, nbytes)
    else:
        from toybox_amd import hip
        copy = hip.memcpy_dtoh
    if not engine._agent_ring:
        ptr, nbytes = engine.device_buffer(_abi.BUF_AGENT_OBS)
        assert nbytes == n * px * stack
        return lambda lo, hi, out: copy(out, ptr + lo * px * stack, (hi - lo) * px * stack)
    ptr, nbytes = engine.device_buffer(_abi.BUF_AGENT_RING)
    assert nbytes == n * px * stack
    head = engine.agent_ring_head()
    keep = {}

    def fetch(lo, hi, out):
        m = hi - lo
        if "plane" not in keep or keep["plane"].shape[0] < m:
            keep["plane"] = engine.host_array((m, px))
        plane = keep["plane"][:m]
        channels = out[:m].reshape(m, px, stack)
        for c in range(stack):
            copy(plane, ptr + (((head + 1 + c) % stack) * n + lo) * px, m * px)
            channels[:, :, c] = plane
    return fetch


class FrameChecker:
    """compare(got, want, count): frames 0 .. count-1 of two sources, each a callable (lo, hi, out) that fills out[:hi - lo] with
    frames lo .. hi-1, slice by slice.  A mismatch fails with the first differing byte as (frame j, env i, y, x, channel, got,
    want) -- j = frame // n, i = frame % n with frames numbered from frame0 -- and the number of frames and envs that differ."""

    def __init__(self, shape, slice_bytes=FRAME_SLICE_BYTES, pinned=False):
        self.shape = tuple(int(d) for d in shape)
        fb = int(np.prod(self.shape))
        self.per = max(1, slice_bytes // fb)
        self._pinned = pinned
        self._got = self._want = None

    def _buffers(self, m):
        if self._got is None or self._got.shape[0] < m:
            m = self.per if m > self.per // 2 else m              # (a small batch keeps small buffers)
            if self._pinned:
                from toybox_amd import hip
                self._pin = hip.PinnedArray((m,) + self.shape)
                self._got = self._pin.array
            else:
                self._got = np.empty((m,) + self.shape, np.uint8)
            self._want = np.empty((m,) + self.shape, np.uint8)
        return self._got, self._want

    def compare(self, got, want, count, n=None, frame0=0, what=""):
        n = n or count
        g, w = self._buffers(min(count, self.per))
        first, bad_frames, bad_envs = None, 0, set()
        for lo in range(0, count, self.per):
            hi = min(count, lo + self.per)
            m = hi - lo
            got(lo, hi, g[:m])
            want(lo, hi, w[:m])
            if np.array_equal(g[:m], w[:m]):
                continue
            rows = np.flatnonzero((g[:m] != w[:m]).reshape(m, -1).any(axis=1))
            bad_frames += len(rows)
            bad_envs.update(((frame0 + lo + rows) % n).tolist())
            if first is None:
                r = int(rows[0])
                y, x, ch = (int(v) for v in np.argwhere(g[r] != w[r])[0])
                f = frame0 + lo + r
                first = (f // n, f % n, y, x, ch, int(g[r][y, x, ch]), int(w[r][y, x, ch]))
        if first is not None:
            raise AssertionError("%s: frames differ: first at frame j=%d env i=%d y=%d x=%d channel %d (got %d, want %d); "
                                 "%d frames of %d, %d envs" % ((what,) + first + (bad_frames, count, len(bad_envs))))
