"""What every TBX_BUF_* id names after every call that produces it (include/toybox_amd.h: the TBX_BUF_* block, tbx_rollout_synthetic,
tbx_device_buffer, the engine options).

A table of fixed call scripts.  After EACH call the test reads the five step-output ids, TBX_BUF_FRAME and the two rollout ids --
tbx_device_buffer, then a copy on the stream the call named (support.read_buffer) -- and compares size and every byte with a small
MODEL of the header that the test keeps itself:

* REWARD / DONE / LIVES / SCORE / PACKED hold the outputs of the last step-like call (of a chunk: of its last step).  They come from
  a TWIN oracle engine that is only ever driven through the host-pointer tbx_step with support.synthetic_actions.
* FRAME: after a call that rasterises into an engine-owned buffer (tbx_render_device(NULL), tbx_render_step_synthetic(NULL),
  tbx_step_begin with a frame, the host-pointer tbx_render) it is the frame of the state at that call in that call's channel count;
  after tbx_rollout_synthetic the chunk's last frame; after every other call unchanged.  Its size is that of the frame it names,
  N * H * W * channels, never the capacity of an allocation; before the first such call the id is NULL / 0 bytes.
* ROLLOUT_FRAMES / ROLLOUT_PACKED hold the last chunk's k frames and k rows of records; other calls leave them alone; before the
  first chunk they are TBX_E_INVALID.

Expected frames are the twin's one-env painter (tbx_render_env), env by env.  On the hip parameter the same script also runs on a
second engine of the oracle library and BOTH are held against the model, so a failure says which library left the header.  The
engine form each case means to exercise is asserted through the read-only TBX_OPT_*_ACTIVE options, so that no case silently tests
the stream-order fallback twice.  Deterministic, one reader, on the caller's stream: this is about what the ids name, not about races.
"""
import numpy as np
import pytest

from support import ENGINES_CHOICE_PIPELINE, ENGINES_CHOICE_ROLLOUT_CHUNKS, read_buffer, synthetic_actions
from toybox_amd import Engine, ToyboxAmdError, _abi

SEED = 1337                                                  # action seed of every synthetic call
WARM = 300                                                   # host steps before a script starts: scores, lives and pictures differ between envs by then


def warm_up(e, game, n):
    """the same WARM host steps on every engine of a case; returns the last one's outputs"""
    for w in range(WARM):
        out = e.step(synthetic_actions(game, n, w, seed=3), auto_reset=True)
    return out


@pytest.fixture(params=["oracle", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request, oracle_lib):
    if request.param == "oracle":
        return oracle_lib
    from toybox_amd import _lib
    return _lib.load()


STEP_IDS = (("REWARD", _abi.BUF_REWARD, np.int32), ("DONE", _abi.BUF_DONE, np.uint8), ("LIVES", _abi.BUF_LIVES, np.int32),
            ("SCORE", _abi.BUF_SCORE, np.int32), ("PACKED", _abi.BUF_PACKED, np.uint64))

EDITS = {"breakout": (_abi.EDIT_BRK_COLUMN_ALIVE, (3, 0)), "space_invaders": (_abi.EDIT_SET_LIVES, (2,)), "amidar": (_abi.EDIT_SET_LIVES, (2,))}


# ---------------------------------------------------------------- the model: what the header says each id holds

def packed_records(reward, done, lives):
    """{reward:i32, done:u8, lives:u8, pad:u16} (include/toybox_amd.h, TBX_BUF_PACKED)"""
    return (reward.view(np.uint32).astype(np.uint64) | (done.astype(np.uint64) << np.uint64(32))
            | (np.clip(lives, 0, 255).astype(np.uint64) << np.uint64(40)))


class Model:
    """the header's rules in plain Python over a twin oracle engine (host tbx_step + tbx_render_env only)"""

    def __init__(self, game, n, oracle_lib, stride):
        self.game, self.n, self.stride = game, n, stride
        self.twin = Engine(game, n, lib=oracle_lib)
        self.twin.seed(11)
        self.twin.new_game()
        self.t = 0
        self.outs = None                                     # {name: array} of the last step-like call
        self._took(warm_up(self.twin, game, n))
        self.frame = None                                    # uint8[n, H, W, C] or None (NULL / 0 bytes)
        self.roll = None                                     # (frames uint8[k, n, H, W, C], records uint64[k, stride]) or None (TBX_E_INVALID)

    def frames(self, ch):
        return np.stack([self.twin.render_env(i, ch) for i in range(self.n)])

    def actions(self):
        return synthetic_actions(self.game, self.n, self.t, seed=SEED)

    def _took(self, out):
        r, d, lv, sc = out
        d = d.astype(np.uint8)
        self.outs = {"REWARD": r, "DONE": d, "LIVES": lv, "SCORE": sc, "PACKED": packed_records(r, d, lv)}

    def step(self):
        self._took(self.twin.step(self.actions(), auto_reset=True))
        self.t += 1

    def chunk(self, ch, k):
        fr, rows = [], np.zeros((k, self.stride), np.uint64)
        for j in range(k):
            fr.append(self.frames(ch))                       # frame j shows the state BEFORE step t0 + j
            self.step()
            rows[j, :self.n] = self.outs["PACKED"]
        self.roll = (np.stack(fr), rows)
        self.frame = fr[-1]                                  # TBX_BUF_FRAME: the chunk's last frame


# ---------------------------------------------------------------- an engine under test and how a script's calls reach it

class Under:
    def __init__(self, name, lib, case):
        self.name, self.is_hip = name, not hasattr(lib, "orc_splitmix64")
        game, n = case["game"], case["n"]
        self.e = e = Engine(game, n, lib=lib)
        e.seed(11)
        e.new_game()
        warm_up(e, game, n)
        self.fb = e.height * e.width
        if self.is_hip:
            from toybox_amd import hip
            self.hip = hip
            self.stream = hip.Stream()
            self.sp = self.stream.ptr
            self.user_frame = hip.malloc(n * self.fb * 4)   # a caller's frame buffer, a caller's action array
            self.user_actions = hip.malloc(4 * n)
        else:
            self.stream, self.sp = None, 0
            self._frame_arr, self._act_arr = np.zeros(n * self.fb * 4, np.uint8), np.zeros(n, np.int32)
            self.user_frame, self.user_actions = self._frame_arr.ctypes.data, self._act_arr.ctypes.data
        for opt, val in case.get("opts", ()):                # (the oracle stores launch-time options without effect)
            e.set_option(opt, val)
        g = case.get("gather")
        if g:
            e.set_option(_abi.OPT_GATHER_EVERY, g["every"])
            e.gather_init(1, 0, e.gather_unique_id(), records_per_rank=case["n"] + g["pad"])
        if self.is_hip:                                      # which form runs: only the device engine has any
            for opt, val in case.get("active", {}).items():
                assert e.get_option(opt) == val, "%s: option %d reads %d, the case needs %d" % (case["id"], opt, e.get_option(opt), val)

    def put_actions(self, a):
        if self.is_hip:
            self.hip.memcpy_htod(self.user_actions, a, a.nbytes)
        else:
            self._act_arr[:] = a

    def user_frames(self, shape):
        m = int(np.prod(shape))
        if not self.is_hip:
            return self._frame_arr[:m].reshape(shape).copy()
        out = np.empty(shape, np.uint8)
        self.stream.synchronize()
        self.hip.memcpy_dtoh(out, self.user_frame, m)
        return out

    def close(self):
        self.e.close()
        if self.is_hip:
            self.hip.free(self.user_frame)
            self.hip.free(self.user_actions)
            self.stream.close()


def first_diff(got, want):
    """the first differing element as its index tuple, with both values"""
    i = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
    idx = tuple(int(v) for v in np.unravel_index(i, got.shape))
    return "first wrong element at %r (got %d, want %d), %d of %d differ" % (idx, int(got[idx]), int(want[idx]), int((got != want).sum()), got.size)


def run_call(u, m, op, case):
    """carry out call `op` on engine u; m is the model BEFORE the call (its twin still shows the state the call starts from).
    Returns the problems found with what the call itself handed back (host outputs, a caller's buffer)."""
    e, n, kind, bad = u.e, case["n"], op[0], []
    H, W = e.height, e.width

    def same(what, got, want):
        if not np.array_equal(got, want):
            bad.append("%s: %s" % (what, first_diff(np.asarray(got), np.asarray(want))))

    if kind == "step":
        out = e.step(m.actions(), auto_reset=True)
        return ("host", out)
    if kind == "step_device":
        u.put_actions(m.actions())
        e.step_device(u.user_actions, auto_reset=True, stream=u.sp)
    elif kind == "step_synth":
        e.step_synthetic(SEED, m.t, auto_reset=True, stream=u.sp)
    elif kind == "rd_own":
        e.render_device(0, op[1], stream=u.sp)
    elif kind == "rd_ptr":
        e.render_device(u.user_frame, op[1], stream=u.sp)
        same("the caller's frame buffer", u.user_frames((n, H, W, op[1])), m.frames(op[1]))
    elif kind == "render":
        same("the host frames", e.render(op[1]), m.frames(op[1]))
    elif kind == "render_env":
        same("the host frame", e.render_env(op[1], op[2]), m.twin.render_env(op[1], op[2]))
    elif kind == "rs_own":
        if u.is_hip and len(op) > 2 and op[2] is not None:
            assert e.get_option(_abi.OPT_FUSED_OVERLAP_ACTIVE) == int(op[2]), "%s: overlapped fused launches are %s" % (case["id"], "off" if op[2] else "on")
        e.render_step_synthetic(SEED, m.t, 0, op[1], auto_reset=True, stream=u.sp)
    elif kind == "rs_ptr":
        want = m.frames(op[1])
        e.render_step_synthetic(SEED, m.t, u.user_frame, op[1], auto_reset=True, stream=u.sp)
        same("the caller's frame buffer", u.user_frames((n, H, W, op[1])), want)
    elif kind == "rollout":
        ch, k, path = op[1], op[2], op[3]
        if u.is_hip and path is not None:
            if case["game"] == "breakout" and ch == 1:       # gray frames never chunk there (TBX_OPT_ROLLOUT_CHUNKS_ACTIVE answers for RGB)
                assert path == "fallback"
            else:
                assert e.get_option(_abi.OPT_ROLLOUT_CHUNKS_ACTIVE) == int(path == "chunk"), "%s: this chunk was to take the %s path" % (case["id"], path)
        e.rollout_synthetic(SEED, m.t, k, channels=ch, auto_reset=True, stream=u.sp)
    elif kind == "begin_end":
        ch = op[1]
        r, lv, sc, d = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint8)
        fr = np.empty((n, H, W, ch), np.uint8)
        e.step_begin(m.actions(), auto_reset=True, reward=r, done=d, lives=lv, score=sc, frame=fr, channels=ch)
        e.step_end()
        return ("host+frame", (r, d, lv, sc), fr)
    elif kind == "new_game":
        e.new_game((np.arange(n) % 3 == 1).astype(np.uint8))
    elif kind == "set_state":
        e.set_state(n - 1, case["_state"])
    elif kind == "edit":
        code, args = EDITS[case["game"]]
        e.edit(code, args, mask=(np.arange(n) % 2 == 0))
    elif kind == "gather":
        e.gather(stream=u.sp)
    elif kind == "opt":
        e.set_option(op[1], op[2])
    else:
        raise AssertionError("unknown call kind %r" % (kind,))
    return ("checked", bad)


def model_call(m, op, case):
    """the model's side of call `op`: the twin moves on, the ids' expected contents follow the header's rules"""
    kind, n = op[0], case["n"]
    if kind in ("step", "step_device", "step_synth"):
        m.step()
    elif kind in ("rd_own", "render"):
        m.frame = m.frames(op[1])
    elif kind == "rs_own":
        m.frame = m.frames(op[1])                            # the state BEFORE the step
        m.step()
    elif kind == "rs_ptr":
        m.step()
    elif kind == "rollout":
        m.chunk(op[1], op[2])
    elif kind == "begin_end":
        m.step()
        m.frame = m.frames(op[1])                            # the state the step leaves
    elif kind == "new_game":
        m.twin.new_game((np.arange(n) % 3 == 1).astype(np.uint8))
    elif kind == "set_state":
        m.twin.set_state(n - 1, case["_state"])
    elif kind == "edit":
        code, args = EDITS[case["game"]]
        m.twin.edit(code, args, mask=(np.arange(n) % 2 == 0))
    # rd_ptr, render_env, gather, opt: no id changes, the twin stays where it is


def check_ids(u, m, where):
    """every id of engine u against the model, size first, then every byte; returns the problems"""
    e, bad = u.e, []

    def held(name, which, want):
        ptr, nbytes = e.device_buffer(which)
        if nbytes != want.nbytes:
            bad.append("%s TBX_BUF_%s on %s: %d bytes reported, the header says %d" % (where, name, u.name, nbytes, want.nbytes))
            return
        got = read_buffer(e, which, want.shape, want.dtype, stream=u.stream)
        if not np.array_equal(got, want):
            bad.append("%s TBX_BUF_%s on %s: %s" % (where, name, u.name, first_diff(got, want)))

    for name, which, dt in STEP_IDS:
        held(name, which, m.outs[name])
    if m.frame is None:
        ptr, nbytes = e.device_buffer(_abi.BUF_FRAME)
        if ptr or nbytes:
            bad.append("%s TBX_BUF_FRAME on %s: %#x / %d bytes before anything was rasterised into an engine-owned buffer" % (where, u.name, ptr, nbytes))
    else:
        held("FRAME [env, y, x, channel]", _abi.BUF_FRAME, m.frame)
    for name, which, idx in (("ROLLOUT_FRAMES [j, env, y, x, channel]", _abi.BUF_ROLLOUT_FRAMES, 0), ("ROLLOUT_PACKED [j, record]", _abi.BUF_ROLLOUT_PACKED, 1)):
        if m.roll is None:
            try:
                e.device_buffer(which)
                bad.append("%s TBX_BUF_%s on %s: addressable before the first chunk" % (where, name, u.name))
            except ToyboxAmdError as err:
                if err.code != _abi.E_INVALID:
                    bad.append("%s TBX_BUF_%s on %s: error %d before the first chunk, not TBX_E_INVALID" % (where, name, u.name, err.code))
        else:
            held(name, which, m.roll[idx])
    return bad


# ---------------------------------------------------------------- the table
# calls: step (host pointer) | step_device | step_synth | rd_own C / rd_ptr C (tbx_render_device into the engine's / a caller's buffer) |
# render C (host pointer) | render_env E C | rs_own C [overlapped?] / rs_ptr C (tbx_render_step_synthetic) | rollout C k path |
# begin_end C (tbx_step_begin with a frame + tbx_step_end) | new_game (a mask) | set_state | edit | gather | opt OPTION VALUE

OFF2 = [(_abi.OPT_FUSED_OVERLAP, _abi.FUSED_OVERLAP_OFF), (_abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_OFF)]
CHUNKS, FUSED, PIPE, RECS, ONE = (_abi.OPT_ROLLOUT_CHUNKS_ACTIVE, _abi.OPT_FUSED_OVERLAP_ACTIVE, _abi.OPT_PIPELINE_ACTIVE, _abi.OPT_RECORDS_ACTIVE,
                                  _abi.OPT_RENDER_STEP_FUSED)
# sizes at which the engines themselves pick an overlapped form: the smallest the two tables of tests/test_gpu_paths.py name
N_BRK_AUTO = min(n for (g, n), (plain, _) in ENGINES_CHOICE_ROLLOUT_CHUNKS.items() if g == "breakout" and plain)
N_SI_AUTO = min(n for (g, n), mode in ENGINES_CHOICE_PIPELINE.items() if g == "space_invaders" and mode == 3)

CASES = [
    # stream order: every producer, 3 -> 1 -> 4 -> 3 through tbx_render_device(NULL), fallback chunks at 3 and 1 channels
    dict(id="breakout-stream-order", game="breakout", n=9, opts=OFF2, active={PIPE: 0, FUSED: 0, CHUNKS: 0, RECS: 1, ONE: 1}, script=[
        ("step",), ("rd_own", 3), ("step_device",), ("rd_ptr", 4), ("step_synth",), ("rd_own", 1), ("render_env", 2, 3), ("rd_own", 4), ("new_game",),
        ("rd_own", 3), ("rs_own", 3, False), ("rs_ptr", 1), ("rollout", 3, 2, "fallback"), ("set_state",), ("render", 1), ("begin_end", 4), ("edit",),
        ("rollout", 1, 1, "fallback"), ("rs_own", 4, False), ("render", 3)]),
    # pipelined mode, two engine-owned frame buffers and two output sets alternating
    dict(id="breakout-pipelined", game="breakout", n=77, opts=OFF2 + [(_abi.OPT_PIPELINE, _abi.PIPELINE_OVERLAP_RENDERS)], active={PIPE: 3, FUSED: 0, CHUNKS: 0},
         script=[("step_synth",), ("rd_own", 3), ("step_synth",), ("rd_own", 1), ("step_synth",), ("rd_own", 4), ("step_synth",), ("rd_own", 3), ("rd_ptr", 3),
                 ("step",), ("rd_own", 3), ("new_game",), ("step_synth",), ("render", 4), ("step_synth",), ("rollout", 1, 2, "fallback"), ("rd_own", 3),
                 ("begin_end", 1)]),
    # overlapped fused launches; a gray fused call is the two launches in stream order into the engine's own buffer
    dict(id="breakout-fused-overlap", game="breakout", n=255, opts=[(_abi.OPT_FUSED_OVERLAP, _abi.FUSED_OVERLAP_ON), (_abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_OFF)],
         active={PIPE: 0, FUSED: 1, CHUNKS: 0}, script=[
        ("rs_own", 3, True), ("rs_own", 3, True), ("rs_own", 4, True), ("rs_ptr", 3), ("rs_own", 3, True), ("rs_own", 1), ("rs_own", 3, True), ("step",),
        ("rs_own", 3, True), ("render", 1), ("rs_own", 4, True), ("edit",), ("rs_own", 3, True), ("rollout", 3, 2, "fallback"), ("rs_own", 3, True),
        ("set_state",), ("rs_own", 3, True)]),
    # rollout chunks in every form of the option, 3 -> 1 -> 4 -> 3 through chunks, steps of other kinds behind a chunk
    dict(id="breakout-chunks", game="breakout", n=257, opts=[(_abi.OPT_FUSED_OVERLAP, _abi.FUSED_OVERLAP_OFF), (_abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_PER_FRAME)],
         active={CHUNKS: 1, FUSED: 0}, script=[
        ("rollout", 3, 2, "chunk"), ("rollout", 3, 2, "chunk"), ("step",), ("rollout", 1, 1, "fallback"), ("opt", _abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_SPAN),
        ("rollout", 4, 4, "chunk"), ("rs_ptr", 3), ("rollout", 3, 1, "chunk"), ("new_game",), ("opt", _abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_OFF),
        ("rollout", 3, 2, "fallback"), ("opt", _abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_AUTO), ("rollout", 3, 2, "chunk"), ("render", 1),
        ("rollout", 4, 1, "chunk"), ("rd_own", 3), ("step_synth",), ("rollout", 3, 2, "chunk"), ("step_device",)]),
    # one collective per step: chunks are single calls
    dict(id="breakout-gather-per-step", game="breakout", n=33, gather=dict(every=1, pad=3), opts=[(_abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_ON)],
         active={CHUNKS: 0, FUSED: 0}, script=[
        ("step_synth",), ("gather",), ("rs_own", 3, False), ("gather",), ("rollout", 3, 2, "fallback"), ("rd_own", 1), ("rollout", 4, 1, "fallback"), ("step",),
        ("gather",), ("rd_own", 3), ("rollout", 1, 2, "fallback"), ("render", 3)]),
    # a K-step record ring with k == K: the chunk's rows ARE the ring (stride = records_per_rank)
    dict(id="breakout-ring", game="breakout", n=65, gather=dict(every=2, pad=3), opts=[(_abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_ON)], active={CHUNKS: 1, FUSED: 0},
         script=[("rollout", 3, 2, "chunk"), ("rd_own", 1), ("step_synth",), ("gather",), ("rs_own", 3, False), ("gather",), ("rollout", 4, 2, "chunk"),
                 ("rollout", 3, 2, "chunk"), ("step",), ("gather",), ("step_device",), ("gather",), ("opt", _abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_OFF),
                 ("rollout", 3, 2, "fallback"), ("render", 3)]),
    # the engine's own choices at a size where it chunks (and may overlap fused launches)
    dict(id="breakout-auto", game="breakout", n=N_BRK_AUTO, active={CHUNKS: 1}, script=[
        ("rollout", 3, 2, "chunk"), ("rs_own", 3), ("rs_own", 3), ("step",), ("rollout", 3, 2, "chunk"), ("rd_own", 1), ("rollout", 3, 1, "chunk"), ("new_game",),
        ("rs_own", 3), ("rollout", 3, 2, "chunk"), ("render", 3), ("step_synth",)]),
    # SpaceInvaders on render records: chunks in RGB, gray and RGBA, the option off and on
    dict(id="space_invaders-records", game="space_invaders", n=131, opts=[(_abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_ON)], active={CHUNKS: 1, RECS: 1, PIPE: 0}, script=[
        ("rollout", 3, 2, "chunk"), ("step",), ("rollout", 1, 2, "chunk"), ("rd_own", 4), ("rollout", 4, 1, "chunk"), ("rs_own", 3), ("edit",),
        ("rollout", 3, 2, "chunk"), ("opt", _abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_OFF), ("rollout", 3, 2, "fallback"), ("render", 1),
        ("opt", _abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_SPAN), ("rollout", 3, 2, "chunk"), ("begin_end", 3), ("step_device",), ("rd_ptr", 1)]),
    # SpaceInvaders on the state-reading rasteriser (an off-grid enemy): every chunk is single calls, RGB and gray
    dict(id="space_invaders-state", game="space_invaders", n=21, state="off-grid", opts=[(_abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_ON)], active={CHUNKS: 1, RECS: 1},
         script=[("step",), ("rollout", 3, 2, "chunk"), ("set_state",), ("rollout", 3, 2, "fallback"), ("rd_own", 1), ("rollout", 1, 1, "fallback"), ("rs_own", 3),
                 ("render", 4), ("rollout", 4, 2, "fallback"), ("step_synth",), ("rd_own", 3), ("new_game",), ("rollout", 3, 4, "fallback")]),
    dict(id="space_invaders-gather-per-step", game="space_invaders", n=15, gather=dict(every=1, pad=0), opts=[(_abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_ON)],
         active={CHUNKS: 0}, script=[
        ("rollout", 3, 2, "fallback"), ("step_synth",), ("gather",), ("rd_own", 1), ("rollout", 1, 2, "fallback"), ("rs_own", 4), ("gather",), ("render_env", 14, 3),
        ("begin_end", 3), ("gather",), ("rollout", 3, 1, "fallback"), ("render", 3)]),
    # the engine's own choice of the pipelined mode (and of chunks, whichever way) at a size where it picks overlapped launches
    dict(id="space_invaders-auto", game="space_invaders", n=N_SI_AUTO, opts=[(_abi.OPT_PIPELINE, _abi.PIPELINE_AUTO)], active={PIPE: 3, RECS: 1}, script=[
        ("step_synth",), ("rd_own", 3), ("step_synth",), ("rd_own", 3), ("step_synth",), ("rd_own", 1), ("step",), ("rollout", 3, 2, None), ("step_synth",),
        ("rd_own", 3), ("render_env", 700, 3), ("new_game",), ("step_synth",), ("rd_own", 3)]),
    # Amidar and GridWorld never chunk
    dict(id="amidar", game="amidar", n=37, opts=[(_abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_ON), (_abi.OPT_PIPELINE, _abi.PIPELINE_OVERLAP_RENDERS)],
         active={CHUNKS: 0, PIPE: 0, FUSED: 0, RECS: 0}, script=[
        ("step",), ("rd_own", 3), ("rollout", 3, 2, "fallback"), ("rd_own", 1), ("rollout", 1, 2, "fallback"), ("step_device",), ("rd_own", 4), ("rollout", 4, 1, "fallback"),
        ("rs_own", 3, False), ("rs_ptr", 3), ("edit",), ("rollout", 3, 4, "fallback"), ("render", 1), ("begin_end", 3), ("set_state",), ("new_game",), ("step_synth",),
        ("render_env", 36, 4)]),
    dict(id="amidar-ring", game="amidar", n=19, gather=dict(every=4, pad=3), active={CHUNKS: 0}, script=[
        ("rollout", 3, 4, "fallback"), ("step_synth",), ("gather",), ("step",), ("gather",), ("rs_own", 1), ("gather",), ("step_device",), ("gather",),
        ("rollout", 1, 4, "fallback"), ("rd_own", 3), ("rollout", 4, 4, "fallback")]),
    dict(id="gridworld", game="gridworld", n=299, active={CHUNKS: 0, PIPE: 0, FUSED: 0, RECS: 0}, script=[
        ("step",), ("rollout", 3, 2, "fallback"), ("rd_own", 4), ("rollout", 1, 1, "fallback"), ("render", 3), ("rs_own", 1), ("step_synth",), ("rollout", 4, 4, "fallback"),
        ("rd_ptr", 3), ("new_game",), ("set_state",), ("rd_own", 3), ("begin_end", 1), ("rollout", 3, 1, "fallback"), ("step_device",)]),
]


def test_the_table_covers_what_it_promises():
    """every producer, every game with a fallback chunk at 3 channels, one at 1 channel, k in {1, 2, 4}, every form of the options"""
    kinds = {op[0] for c in CASES for op in c["script"]}
    assert kinds >= {"step", "step_device", "step_synth", "rd_own", "rd_ptr", "render", "render_env", "rs_own", "rs_ptr", "rollout", "begin_end",
                     "new_game", "set_state", "edit"}
    rolls = [(c["game"], op[1], op[2], op[3]) for c in CASES for op in c["script"] if op[0] == "rollout"]
    for game in ("breakout", "space_invaders", "amidar", "gridworld"):
        assert (game, 3) in {(g, ch) for g, ch, _, path in rolls if path == "fallback"}, game
    assert any(ch == 1 and path == "fallback" for _, ch, _, path in rolls)
    assert {k for _, _, k, _ in rolls} == {1, 2, 4}
    values = {op[2] for c in CASES for op in c["script"] if op[0] == "opt" and op[1] == _abi.OPT_ROLLOUT_CHUNKS}
    values |= {v for c in CASES for o, v in c.get("opts", ()) if o == _abi.OPT_ROLLOUT_CHUNKS}
    assert values >= {_abi.ROLLOUT_CHUNKS_PER_FRAME, _abi.ROLLOUT_CHUNKS_SPAN, _abi.ROLLOUT_CHUNKS_OFF, _abi.ROLLOUT_CHUNKS_AUTO}
    assert {(c.get("gather") or {}).get("every", 0) for c in CASES} >= {0, 1, 2}
    assert all(12 <= len(c["script"]) <= 20 for c in CASES)
    for c in CASES:                                          # 3 -> 1 -> 4 -> 3 on one engine: through tbx_render_device(NULL), chunks, the host render
        for kind in ("rd_own", "rollout", "render"):
            if (c["id"], kind) in (("breakout-stream-order", "rd_own"), ("breakout-chunks", "rollout")):
                seq = [op[1] for op in c["script"] if op[0] == kind]
                assert any(seq[i:i + 4] == [3, 1, 4, 3] for i in range(len(seq))), (c["id"], kind, seq)
    host = [op[1] for c in CASES if c["id"] == "breakout-stream-order" for op in c["script"] if op[0] in ("render", "begin_end", "rd_own")]
    assert host[-4:] == [3, 1, 4, 3]                         # ... rd_own 3, render 1, begin_end 4, render 3


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_buffer_ids_after_every_call(case, lib, oracle_lib):
    case = dict(case)
    n, game = case["n"], case["game"]
    g = case.get("gather")
    m = Model(game, n, oracle_lib, stride=n + g["pad"] if g and g["every"] > 1 else n)
    under = [Under("hip" if not hasattr(lib, "orc_splitmix64") else "oracle", lib, case)]
    if under[0].is_hip:
        under.append(Under("oracle", oracle_lib, case))
    form = "%s, %d envs" % (case["id"], n)
    try:
        bad = [b for u in under for b in check_ids(u, m, "%s, before the first call:" % form)]
        assert not bad, "\n".join(bad)
        for i, op in enumerate(case["script"]):
            where = "%s, call %d %r:" % (form, i, op)
            if op[0] == "set_state":                         # env 0's state into the last env -- off the grid where the case says so
                st = m.twin.get_state(0)
                if case.get("state") == "off-grid":
                    st.enemies[2].x += 3
                case["_state"] = st
            results = [run_call(u, m, op, case) for u in under]
            model_call(m, op, case)
            bad = []
            for u, res in zip(under, results):
                if res[0] == "checked":
                    bad += ["%s %s on %s: %s" % (where, op[0], u.name, b) for b in res[1]]
                else:                                        # host outputs of tbx_step / tbx_step_begin: the step's, as the ids
                    r, d, lv, sc = res[1]
                    for name, got in (("REWARD", r), ("DONE", np.asarray(d).astype(np.uint8)), ("LIVES", lv), ("SCORE", sc)):
                        if not np.array_equal(got, m.outs[name]):
                            bad.append("%s host output %s on %s: %s" % (where, name, u.name, first_diff(got, m.outs[name])))
                    if res[0] == "host+frame" and not np.array_equal(res[2], m.frame):
                        bad.append("%s host frames on %s: %s" % (where, u.name, first_diff(res[2], m.frame)))
                bad += check_ids(u, m, where)
            assert not bad, "\n".join(bad)
        for u in under:
            u.e.sync()
    finally:
        for u in under:
            u.close()
        m.twin.close()
