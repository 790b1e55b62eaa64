"""The overlapped raw-frame loop forms through game ends, rewards, lost lives and level clears.

tests/test_gpu_paths.py and tests/test_gpu_frames.py hold rollout chunks (tbx_rollout_synthetic), Breakout's fused render + step launch
(tbx_render_step_synthetic, in stream order and overlapped on two lanes), the pipelined mode (TBX_OPT_PIPELINE 2 / 3) and the K-step
record ring to the oracle -- from a new game, over fewer than 100 frames, in which no game ends and no reward falls: every record
they compare is (0, 0, lives).  Here the same forms start from mid-game states (tests/support.py donor_records /
write_mid_game_states with 256 donor envs: env i gets donor record i % 256, every even env one life, engines seeded 33, actions
1337), so that inside a window of 48 or 60 frames games end at every position of a chunk, in chunks and calls of either parity and
in every ring slot, rewards fall and lives go without the game ending.  Eight Breakout envs (LEVEL_ENVS) get the hand-made "last
brick in the ball's way" state of test_level_transitions_parity (only alive bits and the ball differ from a donor state, so the wall
stays canonical and TBX_OPT_RECORDS_ACTIVE stays 1); Amidar's envs 0..7 get amidar_edit_last_lives.

Every case asserts, after the state writes and again at the end of the loop, that the form it names is in force (TBX_OPT_*_ACTIVE),
runs the whole window back to back on a caller's stream with every result copied device-side right behind tbx_device_buffer, and
compares with np.array_equal against the oracle's single calls: every frame's packed word of every env, the five output arrays
(every call; the last step of every chunk), the gathered block under a ring, every frame of the window for every env whose game
ends, that loses a life or scores inside it plus a fixed sample (FrameChecker), and at the end every env's state bytes and
simulator RNG words -- then a score is written into every env and one host step taken, whose reward shows the one per-env value no
record holds: the score the next reward is measured from (two Breakout cases stop the window right behind a chunk whose last frame
ended a game, where a stale one would be left).

The coverage conditions are asserted on the ORACLE's outputs (Reference), per case, in the device cases and in the CPU twins alike:
a failure there means the inputs have gone dull, not that the device is wrong.  Measured on the oracle alone with this recipe
(envs x frames: envs whose game ends / share; dones by position in a chunk of 4 | of 3; non-zero rewards; lives lost without the
game ending; LEVEL_ENVS that clear their level):

    breakout       333 x 48: 139 / 0.417;  40 / 31 / 31 / 37 | 40 / 52 / 47;  274;  48;  8
    breakout       700 x 60: 294 / 0.420;  83 / 71 / 72 / 68 | 81 / 109 / 104;  578;  102;  8
    space_invaders 333 x 48: 17 / 0.051;  2 / 0 / 11 / 4 | 3 / 8 / 6;  476;  21;  0
    space_invaders 700 x 60: 62 / 0.089;  18 / 2 / 36 / 6 | 14 / 33 / 15;  1058;  58;  0
    amidar         333 x 48: 9 / 0.027;  2 / 2 / 2 / 3 | 3 / 3 / 3;  373;  13;  0

At 333 x 48 no SpaceInvaders game ends at position 1 of a chunk of 4 (at 700 x 48 neither): its chunks of 4 run 700 x 60, its
other cases 333 x 48.  Nearly every env scores inside the window (322 of 333 in Breakout, 698 of 700 in SpaceInvaders), so the
frame check covers nearly the whole batch in the device cases.

The tests without the gpu mark are the twins: the same loops with the CPU checker in the device's place (its chunk call against
its own single calls), the same coverage conditions, and one that flips a single done bit in the results the comparison reads."""
import ctypes as C
import re

import numpy as np
import pytest

from fork_replay import sim_rngs, states_bytes
from support import (FrameChecker, amidar_edit_last_lives, donor_records, engine_is_oracle, oracle_render_envs, read_buffer,
                     synthetic_actions, write_mid_game_states)
from toybox_amd import Engine, _abi
from toybox_amd.games import codec

SEED, ACTION_SEED, DONORS = 33, 1337, 256
SMALL, LARGE = (333, 48), (700, 60)           # envs x frames: no multiple of 64 or 128; 48 and 60 are multiples of both chunk lengths
K_PLAIN, K_RING = 4, 3                        # frames per chunk without a ring; = K of the record ring
LEVEL_ENVS = (5, 37, 69, 101, 133, 165, 197, 229)      # odd: they keep their donor's lives
AMIDAR_LAST_LIVES_ENVS = range(8)
# share of envs with a game over inside the window (at least 3 envs for Amidar): about half of what the recipe gives
SHARE_FLOOR = {"breakout": 0.25, "space_invaders": 0.02}
AFTERMATH_SCORE = 54321                       # written into every env behind the window; no game reaches it by play
OUTS = ((_abi.BUF_REWARD, np.int32), (_abi.BUF_LIVES, np.int32), (_abi.BUF_SCORE, np.int32), (_abi.BUF_DONE, np.uint8))
ACTIVE = {"records": _abi.OPT_RECORDS_ACTIVE, "chunks": _abi.OPT_ROLLOUT_CHUNKS_ACTIVE, "fused": _abi.OPT_RENDER_STEP_FUSED,
          "overlap": _abi.OPT_FUSED_OVERLAP_ACTIVE, "pipeline": _abi.OPT_PIPELINE_ACTIVE}


# ================================================================ inputs

_START = {}


def start_records(game, n, oracle_lib):
    """the state records the window starts from, computed once per (game, envs) and left unchanged: donor record i % 256 in env i,
    in Breakout the last-brick state in LEVEL_ENVS"""
    if (game, n) not in _START:
        rec = donor_records(game, oracle_lib, DONORS)[np.arange(n) % DONORS].copy()
        if game == "breakout":
            B = rec["bricks"]
            for i, env in enumerate(LEVEL_ENVS):
                keep, nb = 7 * i + 3, int(rec["n_bricks"][env])
                B["alive"][env, :nb] = 0
                B["alive"][env, keep] = 1
                rec["n_balls"][env] = 1
                for name in ("ball_x", "ball_y", "ball_vx", "ball_vy"):
                    rec[name][env, 1:] = 0.0
                rec["ball_x"][env, 0] = B["x"][env, keep] + 6.0       # right under the brick, flying up
                rec["ball_y"][env, 0] = B["y"][env, keep] + B["h"][env, keep] + 2.5
                rec["ball_vx"][env, 0], rec["ball_vy"][env, 0] = 0.25, -2.0
                rec["is_dead"][env] = rec["reset"][env] = 0
        rec.flags.writeable = False
        _START[(game, n)] = rec
    return _START[(game, n)]


def prepare(engines, game, n, oracle_lib):
    """every engine: seeded 33, a new game, the start records, every even env on its last life; Amidar's envs 0..7 with two lives,
    every enemy parked on the player and a jump that runs out 1..8 frames from now (the life goes, and the next frame's too)"""
    for e in engines:
        e.seed(SEED)
        e.new_game()
    write_mid_game_states(engines, n, start_records(game, n, oracle_lib))
    if game == "amidar":
        cd = codec("amidar")
        for i in AMIDAR_LAST_LIVES_ENVS:
            st = cd.state_from_json(amidar_edit_last_lives(cd.state_to_json(engines[0].get_state(i)), lives=2, jump_timer=i + 1,
                                                           perimeter_from_start=True))
            for e in engines:
                e.set_state(i, st)


def oracle_step(o, t):
    return o.step(synthetic_actions(o.game, o.n_envs, t, seed=ACTION_SEED), auto_reset=True)


# ================================================================ the oracle's single calls, once per (game, envs, frames)

class Reference:
    """what the oracle's single calls give over the window: per frame and env the packed word and reward / lives / score / done;
    which envs end a game, score, lose a life without the game ending, clear a level"""

    def __init__(self, game, n, frames, oracle_lib):
        self.game, self.n, self.frames = game, n, frames
        self.packed = np.empty((frames, n), np.uint64)
        self.outs = {which: np.empty((frames, n), dt) for which, dt in OUTS}
        with Engine(game, n, lib=oracle_lib) as o:
            prepare([o], game, n, oracle_lib)
            _, lives0, level, _ = o.scalars()
            self.level_up = np.zeros(n, bool)
            for t in range(frames):
                oracle_step(o, t)
                self.packed[t] = read_buffer(o, _abi.BUF_PACKED, (n,), np.uint64)
                for which, dt in OUTS:
                    self.outs[which][t] = read_buffer(o, which, (n,), dt)
                now = o.scalars()[2]
                self.level_up |= now > level
                level = now
        self.reward, self.lives = self.outs[_abi.BUF_REWARD], self.outs[_abi.BUF_LIVES]
        self.done = self.outs[_abi.BUF_DONE] != 0
        before = np.vstack([lives0[None, :], self.lives[:-1]])   # (after an auto-reset the output still shows the lost game's 0 lives)
        self.life_lost = (self.lives < before) & ~self.done
        self.ended = self.done.any(axis=0)
        self.event_envs = np.flatnonzero(self.ended | (self.reward != 0).any(axis=0) | self.life_lost.any(axis=0))
        for a in (self.packed, self.done, self.life_lost) + tuple(self.outs.values()):
            a.flags.writeable = False

    def counts(self):
        by = lambda k: " / ".join(str(int(self.done[j::k].sum())) for j in range(k))
        return "%-14s %d x %d: %d / %.3f;  %s | %s;  %d;  %d;  %d" % (
            self.game, self.n, self.frames, self.ended.sum(), self.ended.mean(), by(K_PLAIN), by(K_RING),
            (self.reward != 0).sum(), self.life_lost.sum(), self.level_up[list(LEVEL_ENVS)].sum() if self.game == "breakout" else 0)

    # ---- coverage conditions: on these outputs alone
    def assert_events(self):
        g = self.game
        if g == "amidar":
            assert self.ended.sum() >= 3, (g, int(self.ended.sum()))
        else:
            assert self.ended.mean() >= SHARE_FLOOR[g], (g, float(self.ended.mean()))
        assert (self.reward != 0).any(), g
        assert self.life_lost.any(), g
        if g == "breakout":
            assert self.level_up[list(LEVEL_ENVS)].any(), "no last-brick env cleared its level"

    def assert_every_residue(self, mod, what, rewards=False):
        """a game ends (and, rewards: a reward falls) in a frame of every residue t % mod"""
        for j in range(mod):
            assert self.done[j::mod].any(), "%s %s: no game ends at position %d of %d" % (self.game, what, j, mod)
            assert not rewards or (self.reward[j::mod] != 0).any(), "%s %s: no reward at position %d of %d" % (self.game, what, j, mod)

    def assert_chunk_coverage(self, k, ring):
        self.assert_events()
        self.assert_every_residue(k, "chunks of %d" % k, rewards=ring)      # (under a ring, position j is ring slot j)
        chunk = np.arange(self.frames) // k
        for q in range(2):                                                  # the two chunk buffers
            assert self.done[chunk % 2 == q].any(), "%s: no game ends in a chunk of parity %d" % (self.game, q)

    def assert_call_coverage(self, ring=0):
        self.assert_events()
        self.assert_every_residue(2, "output sets and frame buffers")
        self.assert_every_residue(3, "record buffers")
        if ring:
            self.assert_every_residue(ring, "ring slots", rewards=True)


_REFS = {}


def reference(game, size, oracle_lib):
    key = (game,) + tuple(size)
    if key not in _REFS:
        _REFS[key] = Reference(game, size[0], size[1], oracle_lib)
    return _REFS[key]


def checked_envs(ref, cap=None):
    """the envs whose every frame is checked: the fixed sample and every env with an event inside the window (cap: the first so
    many of those -- the twins, which hold the frames in host memory)"""
    n = ref.n
    events = ref.event_envs if cap is None else ref.event_envs[:cap]
    return np.asarray(sorted({0, 1, 127, 128, 255, 256, n // 2, n - 1} | set(events.tolist())), np.int64)


# ================================================================ results held where the device left them

class Hold:
    """memory that receives copies queued on the caller's stream right behind a call -- device memory for the HIP library (nothing
    is synchronised until the loop has ended), plain memory for the CPU checker, which has nothing in flight"""

    def __init__(self, engine, nbytes, stream):
        self.oracle, self.stream, self.nbytes = engine_is_oracle(engine), stream, nbytes
        if self.oracle:
            self.mem = np.empty(nbytes, np.uint8)
            self.ptr = self.mem.ctypes.data
        else:
            from toybox_amd import hip
            self.ptr = hip.malloc(nbytes)

    def put(self, offset, src, nbytes):
        assert 0 <= offset and offset + nbytes <= self.nbytes, (offset, nbytes, self.nbytes)
        if self.oracle:
            C.memmove(self.ptr + offset, src, nbytes)
        else:
            from toybox_amd import hip
            hip.memcpy_dtod_async(self.ptr + offset, src, nbytes, self.stream)

    def get(self, offset, out):
        """into `out` (C-contiguous), once the stream has been synchronised"""
        assert out.flags["C_CONTIGUOUS"] and offset + out.nbytes <= self.nbytes
        if self.oracle:
            C.memmove(out.ctypes.data, self.ptr + offset, out.nbytes)
        else:
            from toybox_amd import hip
            hip.memcpy_dtoh(out, self.ptr + offset, out.nbytes)
        return out

    def close(self):
        if not self.oracle and self.ptr:
            from toybox_amd import hip
            hip.free(self.ptr)
        self.ptr = 0


class Loop:
    """one engine under test (the HIP library, or the checker in its place) over a Reference's window: holds for every frame's
    packed word, for the output arrays of the calls that name them, for the frames of the checked envs; the gathered blocks"""

    def __init__(self, d, ref, envs, stream, frames=None):
        self.d, self.ref, self.envs, self.stream = d, ref, envs, stream
        self.n, self.frames, self.m = ref.n, frames or ref.frames, len(envs)      # (frames: only so many of the Reference's window)
        self.fb = d.height * d.width * 3
        self.sp = stream.ptr if stream is not None else 0
        self.per_out = sum(np.dtype(dt).itemsize for _, dt in OUTS) * self.n
        self.holds = [Hold(d, 8 * self.n * self.frames, stream), Hold(d, self.per_out * self.frames, stream),
                      Hold(d, self.fb * self.m * self.frames, stream)]
        self.hold_p, self.hold_o, self.hold_f = self.holds
        # runs of consecutive checked envs: one copy each (position in the checked list, first env, count)
        cuts = np.flatnonzero(np.diff(envs) != 1) + 1
        self.runs = [(int(p[0]), int(envs[p[0]]), len(p)) for p in np.split(np.arange(self.m), cuts)]
        self.out_frames, self.blocks, self.addr = [], [], []

    def in_force(self, when, **want):
        """the form under test is the form that runs (the checker reports 0 everywhere: nothing to overlap on a CPU thread)"""
        if engine_is_oracle(self.d):
            return
        for name, value in want.items():
            got = self.d.get_option(ACTIVE[name])
            assert got == value, "%s %s: %s active is %d, not %d -- the engine has left the form under test" % (self.ref.game, when, name, got, value)

    def keep_packed(self, t, ptr, count=1):
        self.hold_p.put(8 * self.n * t, ptr, 8 * self.n * count)

    def keep_outputs(self, t):
        """the four output arrays at the addresses tbx_device_buffer names now, as frame t's"""
        off = self.per_out * len(self.out_frames)
        self.out_frames.append(t)
        for which, dt in OUTS:
            p, nb = self.d.device_buffer(which)
            assert nb == np.dtype(dt).itemsize * self.n
            self.hold_o.put(off, p, nb)
            off += nb

    def keep_frames(self, t, ptr):
        """frame t of the checked envs, from a buffer that holds all n envs' frames"""
        for pos, env, count in self.runs:
            self.hold_f.put(self.fb * (t * self.m + pos), ptr + self.fb * env, self.fb * count)

    def keep_block(self, t_first, K):
        assert self.d.gather_fill() == 0
        self.blocks.append((t_first, self.d.gather_host().reshape(K, -1)[:, :self.n].copy()))

    def ring(self, K):
        self.d.set_option(_abi.OPT_GATHER_EVERY, K)
        self.d.gather_init(1, 0, self.d.gather_unique_id())

    def finish(self):
        if self.stream is not None:
            self.stream.synchronize()
        self.d.sync()                                          # (reports a ticket time-out of an overlapped launch, if any)

    def close(self):
        for h in self.holds:
            h.close()

    # ---- the loop forms
    def chunks(self, k, form, ring):
        """tbx_rollout_synthetic, chunk behind chunk; every chunk's k x n packed words, its last step's outputs, its frames"""
        d, n = self.d, self.n
        d.set_option(_abi.OPT_ROLLOUT_CHUNKS, form)
        if ring:
            self.ring(k)
        self.in_force("after the state writes", records=1, chunks=1)
        for c in range(self.frames // k):
            t0 = c * k
            d.rollout_synthetic(ACTION_SEED, t0, k, channels=3, auto_reset=True, stream=self.sp)
            f, nb = d.device_buffer(_abi.BUF_ROLLOUT_FRAMES)
            assert nb == k * n * self.fb
            pk, pb = d.device_buffer(_abi.BUF_ROLLOUT_PACKED)
            assert pb == 8 * k * n                             # (one rank, records_per_rank = n: a ring's rows are n wide)
            self.addr.append(f)
            self.keep_packed(t0, pk, k)
            self.keep_outputs(t0 + k - 1)
            for j in range(k):
                self.keep_frames(t0 + j, f + self.fb * n * j)
            if ring:
                self.keep_block(t0, k)
        self.finish()
        self.in_force("at the end of the loop", records=1, chunks=1)
        if not engine_is_oracle(d):                            # the two chunk buffers alternate
            assert all(a != b for a, b in zip(self.addr, self.addr[1:])) and len(set(self.addr)) == 2, self.addr

    def fused(self, overlap, ring, pipeline=None):
        """tbx_render_step_synthetic, call behind call (under a ring each followed by tbx_gather): every call's outputs and frames.
        pipeline: TBX_OPT_PIPELINE is set to it and has to stay without effect (Amidar: two launches in stream order)"""
        d = self.d
        if pipeline is None:
            d.set_option(_abi.OPT_FUSED_OVERLAP, overlap)
            want = dict(records=1, fused=1, overlap=1 if overlap == _abi.FUSED_OVERLAP_ON else 0)
        else:
            d.set_option(_abi.OPT_PIPELINE, pipeline)
            want = dict(records=0, fused=0, overlap=0, pipeline=0)
        if ring:
            self.ring(ring)
        self.in_force("after the state writes", **want)
        for t in range(self.frames):
            d.render_step_synthetic(ACTION_SEED, t, channels=3, auto_reset=True, stream=self.sp)
            if ring:
                d.gather(stream=self.sp)
            f, _ = d.device_buffer(_abi.BUF_FRAME)
            self.addr.append(f)
            self.keep_packed(t, d.device_buffer(_abi.BUF_PACKED)[0])
            self.keep_outputs(t)
            self.keep_frames(t, f)
            if ring and (t + 1) % ring == 0:
                self.keep_block(t + 1 - ring, ring)
        self.finish()
        self.in_force("at the end of the loop", **want)
        if want["overlap"] and not engine_is_oracle(d):        # two frame buffers
            assert all(a != b for a, b in zip(self.addr, self.addr[1:])) and len(set(self.addr)) == 2, self.addr

    def pipelined(self, mode):
        """tbx_step_synthetic / tbx_render_device pairs on the caller's stream: every step's outputs, read at the address
        tbx_device_buffer names after the call, and every frame -- frame t shows the state AFTER step t"""
        d = self.d
        d.set_option(_abi.OPT_PIPELINE, mode)
        self.in_force("after the state writes", records=1, pipeline=mode)
        for t in range(self.frames):
            d.step_synthetic(ACTION_SEED, t, auto_reset=True, stream=self.sp)
            self.keep_packed(t, d.device_buffer(_abi.BUF_PACKED)[0])
            self.keep_outputs(t)
            d.render_device(0, 3, stream=self.sp)
            self.keep_frames(t, d.device_buffer(_abi.BUF_FRAME)[0])
        self.finish()
        self.in_force("at the end of the loop", records=1, pipeline=mode)

    # ---- everything the loop left against the oracle
    def compare(self, oracle_lib, what, frame_shows_state_after_step=False, tamper=None, k=None):
        ref, n, m = self.ref, self.n, self.m
        packed = self.hold_p.get(0, np.empty((self.frames, n), np.uint64))
        if tamper:
            tamper(packed)
        want = ref.packed[:self.frames]
        if not np.array_equal(packed, want):
            bad = np.argwhere(packed != want)
            t, i = (int(v) for v in bad[0])
            where = "frame %d" % t if k is None else "frame %d (chunk %d, position %d)" % (t, t // k, t % k)
            raise AssertionError("%s: packed word differs at %s env %d (got %#x, want %#x); %d words of %d envs differ"
                                 % (what, where, i, int(packed[t, i]), int(want[t, i]), len(bad), len(set(bad[:, 1].tolist()))))
        buf = np.empty(self.per_out, np.uint8)
        for row, t in enumerate(self.out_frames):
            self.hold_o.get(self.per_out * row, buf)
            off = 0
            for which, dt in OUTS:
                nb = np.dtype(dt).itemsize * n
                got, want = buf[off:off + nb].view(dt), ref.outs[which][t]
                off += nb
                if not np.array_equal(got, want):
                    bad = np.flatnonzero(got != want)
                    raise AssertionError("%s: output buffer %d of frame %d differs in %d envs, first env %d (got %d, want %d)"
                                         % (what, which, t, len(bad), bad[0], got[bad[0]], want[bad[0]]))
        for t0, block in self.blocks:
            want = ref.packed[t0:t0 + len(block)]
            if not np.array_equal(block, want):
                j, i = (int(v) for v in np.argwhere(block != want)[0])
                raise AssertionError("%s: gathered block of frames %d..%d differs in slot %d env %d (got %#x, want %#x)"
                                     % (what, t0, t0 + len(block) - 1, j, i, int(block[j, i]), int(want[j, i])))
        # frames and end state: a second oracle walks the window (its outputs are the Reference's: same engine, same calls)
        chk = FrameChecker((self.d.height, self.d.width, 3), pinned=not engine_is_oracle(self.d))
        with Engine(ref.game, n, lib=oracle_lib) as o:
            prepare([o], ref.game, n, oracle_lib)

            def want_frames(lo, hi, out):
                for pos, env, count in self.runs:
                    a, b = max(lo, pos), min(hi, pos + count)
                    if a < b:
                        oracle_render_envs(o, env + a - pos, b - a, out[a - lo:b - lo], 3)

            for t in range(self.frames):
                if frame_shows_state_after_step:
                    oracle_step(o, t)
                try:
                    chk.compare(lambda lo, hi, out: self.hold_f.get(self.fb * (t * m + lo), out[:hi - lo]), want_frames, m,
                                what="%s frame %d of the window" % (what, t))
                except AssertionError as err:
                    pos = int(re.search(r"env i=(\d+)", str(err)).group(1))
                    raise AssertionError("%s [i counts the %d checked envs: i=%d is env %d]" % (err, m, pos, self.envs[pos])) from None
                if not frame_shows_state_after_step:
                    oracle_step(o, t)
            got, want = states_bytes(self.d), states_bytes(o)
            if not np.array_equal(got, want):
                bad = np.flatnonzero((got != want).any(axis=1))
                raise AssertionError("%s: state records differ at the end in %d envs, first %s" % (what, len(bad), bad[:8]))
            got, want = sim_rngs(self.d), sim_rngs(o)
            if not np.array_equal(got, want):
                bad = np.flatnonzero((got != want).any(axis=1))
                raise AssertionError("%s: simulator RNG words differ at the end in %d envs, first %s" % (what, len(bad), bad[:8]))
            # ... and what no record shows, the score each env's next reward is measured from (0 again after an in-kernel reset):
            # a score written into every env and one host step -- its reward is the written score's distance from that
            for e in (self.d, o):
                e.edit(_abi.EDIT_SET_SCORE, [AFTERMATH_SCORE])
            a = synthetic_actions(ref.game, n, self.frames, seed=ACTION_SEED)
            for name, x, y in zip(("reward", "done", "lives", "score"), self.d.step(a, auto_reset=True), o.step(a, auto_reset=True)):
                if not np.array_equal(x, y):
                    bad = np.flatnonzero(x != y)
                    raise AssertionError("%s: %s of the step after a score write differs in %d envs, first env %d (got %d, want %d)"
                                         % (what, name, len(bad), bad[0], x[bad[0]], y[bad[0]]))


def run_case(lib, oracle_lib, game, size, form, args, frame_cap=None, tamper=None, frames=None):
    """one engine of `lib` through a Reference's window (frames: its first so many frames) in the loop form `form` ("chunks",
    "fused", "pipelined"), everything compared"""
    ref = reference(game, size, oracle_lib)
    # coverage first: dull inputs fail here, on the oracle's outputs, whatever the device does
    if form == "chunks":
        ref.assert_chunk_coverage(args["k"], args["ring"])
    else:
        ref.assert_call_coverage(args.get("ring", 0))
    d = Engine(game, ref.n, lib=lib)
    stream = None
    if not engine_is_oracle(d):
        from toybox_amd import hip
        stream = hip.Stream()
    prepare([d], game, ref.n, oracle_lib)
    loop = Loop(d, ref, checked_envs(ref, frame_cap), stream, frames)
    what = "%s %d x %d %s %r" % (game, ref.n, loop.frames, form, sorted(args.items()))
    try:
        getattr(loop, form)(**args)
        loop.compare(oracle_lib, what, frame_shows_state_after_step=form == "pipelined", tamper=tamper, k=args.get("k"))
    finally:
        d._lib.tbx_sync(d._h)                                   # (the stream may only go once the engine has forgotten it)
        loop.close()
        if stream is not None:
            stream.close()
        d.close()


# ================================================================ the cases
PER_FRAME, SPAN = _abi.ROLLOUT_CHUNKS_PER_FRAME, _abi.ROLLOUT_CHUNKS_SPAN
ON, OFF = _abi.FUSED_OVERLAP_ON, _abi.FUSED_OVERLAP_OFF

# 700 x 60 where the coverage conditions need it (SpaceInvaders' chunks of 4: at 333 x 48 no game ends at position 1) and once per
# Breakout form; everything else at 333 x 48, whose frames cost a third
CHUNK_CASES = [("breakout", SMALL, PER_FRAME, False), ("breakout", SMALL, SPAN, True), ("breakout", SMALL, PER_FRAME, True),
               ("breakout", LARGE, SPAN, False), ("space_invaders", LARGE, PER_FRAME, False), ("space_invaders", LARGE, SPAN, False),
               ("space_invaders", SMALL, PER_FRAME, True), ("space_invaders", SMALL, SPAN, True)]
FUSED_CASES = [(SMALL, ON, 0), (SMALL, OFF, 0), (LARGE, ON, K_RING)]
PIPELINE_CASES = [("breakout", SMALL, 2), ("breakout", SMALL, 3), ("space_invaders", SMALL, 2), ("space_invaders", SMALL, 3)]
AMIDAR_SIZE = SMALL
WINDOWS = sorted({(g, size) for g, size, _, _ in CHUNK_CASES} | {("breakout", size) for size, _, _ in FUSED_CASES}
                 | {(g, size) for g, size, _ in PIPELINE_CASES} | {("amidar", AMIDAR_SIZE)})
TWIN_FRAME_CAP = 24                            # (a twin holds the checked frames in host memory)


def chunk_args(form, ring):
    return dict(k=K_RING if ring else K_PLAIN, form=form, ring=ring)


@pytest.mark.gpu
@pytest.mark.parametrize("game,size,form,ring", CHUNK_CASES)
def test_gpu_rollout_chunks_through_game_ends(game, size, form, ring, hip_lib, oracle_lib):
    """Rollout chunks (TBX_OPT_ROLLOUT_CHUNKS 3: a rasteriser launch per frame, 4: one per chunk; k = 4 without a ring, k = 3 under
    a K = 3 record ring) back to back on a caller's stream from mid-game states: Breakout's brk_rollout_step_kernel resets games
    inside its frame loop at every position of a chunk -- on the last one the new game is the next chunk's first record, in the
    other chunk buffer -- and SpaceInvaders' k step launches carry dones, rewards and dying ships."""
    run_case(hip_lib, oracle_lib, game, size, "chunks", chunk_args(form, ring))


def frames_to_a_reset_on_a_chunks_last_frame(ref, k):
    """the longest whole number of chunks of k frames after whose LAST frame some env has just lost a game with points on the
    board -- a condition on the inputs, read from the oracle's outputs"""
    hit = (ref.done & (ref.outs[_abi.BUF_SCORE] > 0)).any(axis=1)
    ends = [t + 1 for t in range(k - 1, ref.frames, k) if hit[t]]
    assert ends, "%s: no game with a score ends on the last frame of a chunk of %d" % (ref.game, k)
    return ends[-1]


REWARD_BASE_CASES = [(PER_FRAME, False), (SPAN, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,ring", REWARD_BASE_CASES)
def test_gpu_reset_on_a_chunks_last_frame_leaves_the_new_games_reward_base(form, ring, hip_lib, oracle_lib):
    """brk_rollout_step_kernel keeps the score the next reward is measured from in a register and stores it with the state at the
    chunk's end; after a reset inside the loop it must be the NEW game's score.  Play cannot show a stale one (the next frame's
    reward would be negative and is clamped to 0, after which the value is fresh again), a score written right behind a chunk
    whose last frame ended a game can: the window stops there, and the step after the score write (Loop.compare) pays the written
    score out in full only if the stored value was the new game's 0."""
    k = K_RING if ring else K_PLAIN
    frames = frames_to_a_reset_on_a_chunks_last_frame(reference("breakout", SMALL, oracle_lib), k)
    run_case(hip_lib, oracle_lib, "breakout", SMALL, "chunks", chunk_args(form, ring), frame_cap=0, frames=frames)


@pytest.mark.parametrize("form,ring", REWARD_BASE_CASES)
def test_reset_on_a_chunks_last_frame_on_the_checker(form, ring, oracle_lib):
    k = K_RING if ring else K_PLAIN
    frames = frames_to_a_reset_on_a_chunks_last_frame(reference("breakout", SMALL, oracle_lib), k)
    run_case(oracle_lib, oracle_lib, "breakout", SMALL, "chunks", chunk_args(form, ring), frame_cap=0, frames=frames)


@pytest.mark.gpu
@pytest.mark.parametrize("size,overlap,ring", FUSED_CASES)
def test_gpu_fused_render_step_through_game_ends(size, overlap, ring, hip_lib, oracle_lib):
    """Breakout's fused render + step launch, overlapped on two lanes (the COH = true step blocks: agent-scope loads and stores of
    the simulator RNG and the record, across three record buffers and two output sets) and in stream order; overlapped again under
    the K = 3 record ring: the frame of call N + 1 shows the new game that call N's step blocks started."""
    run_case(hip_lib, oracle_lib, "breakout", size, "fused", dict(overlap=overlap, ring=ring))


@pytest.mark.gpu
@pytest.mark.parametrize("game,size,mode", PIPELINE_CASES)
def test_gpu_pipelined_mode_through_game_ends(game, size, mode, hip_lib, oracle_lib):
    """TBX_OPT_PIPELINE 2 / 3, step / render pairs on a caller's stream: both output sets and both frame buffers carry dones,
    rewards and lost lives, each read at the address tbx_device_buffer names after the call."""
    run_case(hip_lib, oracle_lib, game, size, "pipelined", dict(mode=mode))


@pytest.mark.gpu
def test_gpu_amidar_render_step_ignores_the_pipeline_option(hip_lib, oracle_lib):
    """Amidar: tbx_render_step_synthetic is two launches in stream order and TBX_OPT_PIPELINE = 3 changes nothing
    (TBX_OPT_PIPELINE_ACTIVE stays 0) -- and the events, last lives lost in consecutive frames among them, still match."""
    run_case(hip_lib, oracle_lib, "amidar", AMIDAR_SIZE, "fused", dict(overlap=0, ring=0, pipeline=3))


# ---------------------------------------------------------------- the twins: the checker in the device's place

@pytest.mark.parametrize("game,size,form,ring", CHUNK_CASES)
def test_rollout_chunks_loop_and_coverage_on_the_checker(game, size, form, ring, oracle_lib):
    """the checker's chunk call against its own single calls, and every coverage condition of the device case"""
    run_case(oracle_lib, oracle_lib, game, size, "chunks", chunk_args(form, ring), frame_cap=TWIN_FRAME_CAP)


@pytest.mark.parametrize("size,overlap,ring", FUSED_CASES)
def test_fused_render_step_loop_and_coverage_on_the_checker(size, overlap, ring, oracle_lib):
    run_case(oracle_lib, oracle_lib, "breakout", size, "fused", dict(overlap=overlap, ring=ring), frame_cap=TWIN_FRAME_CAP)


@pytest.mark.parametrize("game,size,mode", PIPELINE_CASES)
def test_pipelined_loop_and_coverage_on_the_checker(game, size, mode, oracle_lib):
    run_case(oracle_lib, oracle_lib, game, size, "pipelined", dict(mode=mode), frame_cap=TWIN_FRAME_CAP)


def test_amidar_render_step_loop_and_coverage_on_the_checker(oracle_lib):
    run_case(oracle_lib, oracle_lib, "amidar", AMIDAR_SIZE, "fused", dict(overlap=0, ring=0, pipeline=3), frame_cap=TWIN_FRAME_CAP)


def test_the_loop_notices_one_wrong_done_bit_in_the_last_env_of_the_last_chunk(oracle_lib):
    """the harness has teeth: in the copy of the results that the comparison reads, the done bit of ONE packed word -- the last
    env's, in the last frame of the last chunk -- is flipped, as a kernel that mishandled one game end would leave it"""
    n, frames = SMALL

    def flip(packed):
        packed[frames - 1, n - 1] ^= np.uint64(1 << 32)

    want = r"packed word differs at frame %d \(chunk %d, position %d\) env %d .*; 1 words of 1 envs differ" % (
        frames - 1, frames // K_PLAIN - 1, K_PLAIN - 1, n - 1)
    with pytest.raises(AssertionError, match=want):
        run_case(oracle_lib, oracle_lib, "breakout", SMALL, "chunks", chunk_args(PER_FRAME, False), frame_cap=0, tamper=flip)


def test_measured_counts_in_the_docstring_are_the_recipe_s(oracle_lib):
    """the counts the module docstring quotes are what the committed recipe gives (the oracle is exact: they do not move)"""
    got = [reference(g, size, oracle_lib).counts() for g, size in WINDOWS]
    doc = " ".join(__doc__.split())
    for line in got:
        assert " ".join(line.split()) in doc, "\n".join(got)
