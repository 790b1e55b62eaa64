"""Writes between agent steps, the first frame after a write, and the edges of the edit and query kernels -- held to the CPU oracle
bit for bit: every env, every output, every byte; nothing sampled, no tolerance.

1. Writes between agent steps on the fused observation paths.  1 027 envs (no multiple of a block, of four waves or of 64) from
   mid-game states: 12 agent steps, a write, 8 steps, the next write ... -- every tbx_edit op through a mask over about half the
   envs with per-env arguments, in the host form (one case) and as tbx_edit_device on the caller's stream with nothing synchronised
   before the next tbx_agent_step_device / tbx_agent_step_synthetic (another case); then tbx_set_states on a range in the middle of
   the batch, tbx_new_game with a mask and tbx_seed_array.  Observation (rolled stack or ring), reward, done and the episode monitor of every
   env after every step; state records and simulator RNGs at the end.  And one directed case per game, at the same 1 027 envs, in
   which the game ends in frame 0 or 1 of the agent step after the write in a subset of the envs (the others stay mid-game), while
   MaxAndSkipEnv's buffer still holds snapshots from before it.
2. The first frame after a write on a plain engine: behind every tbx_edit op of the game, with step-written render records in force
   and no step in between, each reader once as the FIRST reader -- tbx_render_device in 3 channels and in 1, the fused
   tbx_render_step_synthetic, a tbx_rollout_synthetic chunk of 2, TBX_QUERY_LOOKAHEAD_ALL over 8 frames -- then 20 batch steps.
3. Edges of the edit and query kernels: batches of 1, 65, 257 and 1 027 envs, every op of every game in four forms (shared
   arguments without and with a mask, per-env rows with a mask, device pointers) with mask bytes 1, 2 and 255, every query row by
   row, the device form into a buffer with 64 sentinel doubles behind it, and per-env arguments outside their range where both
   the kernel and the oracle guard them (include/toybox_amd.h: "entries that do not exist read -1", "the env is left alone").

The tests without the gpu mark are the twins: the same scripts over the checker alone.  There the write is ALSO applied by numpy on
the state records (numpy_edit, written from include/toybox_amd.h, not from either library) and the batched edit must leave exactly
those records; and the conditions that say a script still reaches the code are asserted on the oracle's outputs against a control
engine that gets no write: a picture-changing write changes the observation of at least half the selected envs (against the
control at the same step; the control never catches up, so from the second write on this says less than at the first), a drop in
lives under EpisodicLifeEnv is reported as done, a score edit shows in the reward, a stale-snapshot case ends games in frame 0 or 1.
"""
import ctypes as C

import numpy as np
import pytest

from fork_replay import sim_rngs
from lookahead_replay import assert_fields_equal, expected
from support import (FrameChecker, amidar_edit_last_lives, device_frames, donor_records, engine_is_oracle, oracle_frames, read_buffer,
                     splitmix64, synthetic_actions, write_mid_game_states)
from test_gpu_agent_scale import assert_same_end_state, falling_ball_states
from test_gpu_custom_states import _close, _same_rngs, _same_states, agent_observation, run_agent
from toybox_amd import Engine, _abi
from toybox_amd.games import codec

E = _abi
N = 1027
SEED, ACTION_SEED = 4242, 7
FIRST_STEPS, STEPS_PER_WRITE = 12, 8
BARE = dict(clip_reward=False, episodic_life=False, fire_reset=False, noop_max=0)
FULL = dict(clip_reward=True, episodic_life=True, fire_reset=True, noop_max=7, noop_seed=17)
GAMES = ["breakout", "space_invaders", "amidar"]


# ---------------------------------------------------------------- the edits by numpy, from the header's text

def to_int(x):
    """an integer argument (include/toybox_amd.h via TbxEditArgs): clamped to +-2e9, NaN reads -2e9, truncated"""
    x = np.asarray(x, np.float64)
    x = np.where(x > -2.0e9, x, -2.0e9)
    return np.trunc(np.where(x > 2.0e9, 2.0e9, x)).astype(np.int64)


def to_u32(x):
    x = np.asarray(x, np.float64)
    return np.where(x >= 4294967295.0, 4294967295.0, np.where(x > 0.0, np.floor(x), 0.0)).astype(np.uint64)


def arg_rows(args, n):
    a = np.asarray(args, np.float64)
    return np.broadcast_to(a, (n, a.shape[0])).copy() if a.ndim == 1 else a


def amidar_random_tile(st, i, seed, draw, env_offset, tag_mask, min_dist):
    """TBX_QUERY_AMI_RANDOM_TILE for env i of the records st -> (tx, ty, tag, count): the (r mod count)-th, row by row, of the tiles
    whose tag is in tag_mask and -- min_dist > 0 -- for which NOT every enemy is nearer than that"""
    tiles = st["tiles"][i]
    ok = ((int(tag_mask) >> tiles.astype(np.int64)) & 1) != 0
    if min_dist > 0:
        ne = int(st["n_enemies"][i])
        yy, xx = np.mgrid[0:E.AMI_BOARD_H, 0:E.AMI_BOARD_W]
        etx, ety = st["enemies"]["x"][i, :ne] // E.AMI_TILE_WX, st["enemies"]["y"][i, :ne] // E.AMI_TILE_WY
        near = (np.abs(etx[:, None, None] - xx[None]) + np.abs(ety[:, None, None] - yy[None])) < min_dist
        ok &= ~near.all(axis=0)                                    # (no enemies: all([]) is True, nothing is accepted)
    cand = np.argwhere(ok)
    if not len(cand):
        return -1, -1, -1, 0
    r = int(splitmix64(int(seed) ^ (((int(env_offset) + i) & 0xFFFFFFFF) << 32) ^ int(draw)))
    ty, tx = cand[r % len(cand)]
    return int(tx), int(ty), int(tiles[ty, tx]), len(cand)


def numpy_edit(game, st, op, args, mask):
    """what tbx_edit(op, args, mask) must leave in the state records st (get_states_np), by the text of include/toybox_amd.h"""
    st = st.copy()
    n = len(st)
    a = arg_rows(args, n)
    k = a.shape[1]
    col = lambda i: a[:, i] if i < k else np.zeros(n)              # (an argument that was left out reads 0)
    I = lambda i: to_int(col(i))
    sel = np.ones(n, bool) if mask is None else np.asarray(mask) != 0
    scalar = {E.EDIT_SET_LIVES: "lives", E.EDIT_SET_SCORE: "score", E.EDIT_SET_LEVEL: "level", E.EDIT_AMI_JUMPS: "jumps",
              E.EDIT_SI_UFO_APPEARANCE: "ufo_appearance_counter"}
    if op in scalar:
        st[scalar[op]][sel] = I(0)[sel]
    elif op in (E.EDIT_BRK_COLUMN_ALIVE, E.EDIT_BRK_ROW_ALIVE, E.EDIT_BRK_ALL_ALIVE, E.EDIT_BRK_BRICK_ALIVE):
        B = st["bricks"]
        j = np.arange(E.BRK_MAX_BRICKS)[None, :]
        key = I(0)[:, None]
        hit = {E.EDIT_BRK_COLUMN_ALIVE: B["col"] == key, E.EDIT_BRK_ROW_ALIVE: B["row"] == key, E.EDIT_BRK_ALL_ALIVE: j >= 0,
               E.EDIT_BRK_BRICK_ALIVE: j == key}[op] & (j < st["n_bricks"][:, None]) & sel[:, None]
        on = I(0 if op == E.EDIT_BRK_ALL_ALIVE else 1) != 0
        B["alive"][hit] = np.broadcast_to(on[:, None], hit.shape)[hit]
    elif op == E.EDIT_BRK_PADDLE:
        st["paddle_x"][sel] = col(0)[sel]
        if k >= 2:
            st["paddle_y"][sel] = col(1)[sel]
    elif op == E.EDIT_BRK_BALL:
        b = I(0)
        r = np.flatnonzero(sel & (b >= 0) & (b < E.BRK_MAX_BALLS) & (b < st["n_balls"]))
        for f, name in enumerate(("ball_x", "ball_y", "ball_vx", "ball_vy")):
            st[name][r, b[r]] = col(1 + f)[r]
    elif op == E.EDIT_AMI_TIMERS:
        for i, name in enumerate(("jump_timer", "chase_timer")):
            r = sel & (I(i) >= 0)
            st[name][r] = I(i)[r]
    elif op == E.EDIT_AMI_TILE:
        tx, ty = I(0), I(1)
        r = np.flatnonzero(sel & (tx >= 0) & (ty >= 0) & (tx < E.AMI_BOARD_W) & (ty < E.AMI_BOARD_H))
        st["tiles"][r, ty[r], tx[r]] = (I(2) & 3)[r]
    elif op == E.EDIT_AMI_ENEMY_AI:
        slot = I(0)
        r = np.flatnonzero(sel & (slot >= 0) & (slot < st["n_enemies"]))
        A = st["enemies"]["ai"]
        assert len(A.dtype.names) == 14
        for f, name in enumerate(A.dtype.names):
            A[name][r, slot[r]] = I(1 + f)[r]
    elif op == E.EDIT_AMI_PLAYER_TILE:
        st["player"]["x"][sel] = (I(0) * E.AMI_TILE_WX)[sel]
        st["player"]["y"][sel] = (I(1) * E.AMI_TILE_WY)[sel]
    elif op == E.EDIT_AMI_PLAYER_RANDOM_START:
        seed, draw, off, dist = to_u32(col(0)), to_u32(col(1)), to_u32(col(2)), I(3)
        for i in np.flatnonzero(sel):
            tx, ty, _, count = amidar_random_tile(st, i, seed[i], draw[i], off[i], 15, dist[i])
            if count:
                st["player"]["x"][i], st["player"]["y"][i] = tx * E.AMI_TILE_WX, ty * E.AMI_TILE_WY
    else:
        raise ValueError(op)
    return st


def records_equal(a, b, what):
    a, b = (np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1) for x in (a, b))
    if not np.array_equal(a, b):
        bad = np.flatnonzero((a != b).any(axis=1))
        i = int(bad[0])
        raise AssertionError("%s: state records differ in %d envs, first env %d at byte %d" % (what, len(bad), i, int(np.flatnonzero(a[i] != b[i])[0])))


# ---------------------------------------------------------------- the calls, on either library

class Memory:
    """where an engine reads masks, per-env rows and actions in the device-pointer forms: HBM of the HIP library (released at the
    end), the arrays themselves for the checker"""

    def __init__(self, engine):
        self.oracle = engine_is_oracle(engine)
        self.held = []

    def put(self, array):
        a = np.ascontiguousarray(array)
        if self.oracle:
            self.held.append(a)
            return a.ctypes.data
        from toybox_amd import hip
        p = hip.malloc(max(a.nbytes, 8))
        self.held.append(p)
        hip.memcpy_htod(p, a, a.nbytes)
        return p

    def room(self, nbytes):
        return self.put(np.zeros(nbytes, np.uint8))

    def fetch(self, ptr, out):
        if self.oracle:
            C.memmove(out.ctypes.data, ptr, out.nbytes)
        else:
            from toybox_amd import hip
            hip.memcpy_dtoh(out, ptr, out.nbytes)
        return out

    def release(self):
        if not self.oracle:
            from toybox_amd import hip
            for p in self.held:
                hip.free(p)
        self.held = []


def host_edit(e, op, args, mask, byte=1):
    """tbx_edit with host pointers; the selected envs' mask byte is `byte`"""
    a = np.ascontiguousarray(args, np.float64)
    m = None if mask is None else (np.asarray(mask) != 0).astype(np.uint8) * np.uint8(byte)
    per_env, k = (1, a.shape[1]) if a.ndim == 2 else (0, a.shape[0])
    e._check(e._lib.tbx_edit(e._h, int(op), a.ctypes.data_as(C.c_void_p) if k else None, k, per_env,
                             m.ctypes.data_as(C.c_void_p) if m is not None else None))


def device_edit(e, mem, op, args, mask, stream=0, byte=1):
    """tbx_edit_device on `stream`: the mask and per-env rows where the engine reads device pointers"""
    a = np.ascontiguousarray(args, np.float64)
    m = 0 if mask is None else mem.put((np.asarray(mask) != 0).astype(np.uint8) * np.uint8(byte))
    if a.ndim == 2:
        e.edit_device(op, mask_ptr=m, stream=stream, per_env_ptr=mem.put(a), n_args=a.shape[1])
    else:
        e.edit_device(op, list(a), mask_ptr=m, stream=stream)


AGENT_OUTS = ((E.BUF_AGENT_REWARD, np.float32), (E.BUF_AGENT_DONE, np.uint8), (E.BUF_AGENT_EP_DONE, np.uint8),
              (E.BUF_AGENT_EP_RETURN, np.float32), (E.BUF_AGENT_EP_LENGTH, np.int32))
ROW_NAMES = ("observation", "reward", "done", "episode end", "episode return", "episode length")


def stream_outputs(e, stream):
    """the last agent step's outputs of every env where the engine keeps them, read behind the step on its stream -- the layout of
    run_agent's rows"""
    n, oh, ow, stack = e._agent_shape
    reward, done, ended, ret, length = (read_buffer(e, which, (n,), dt, stream=stream) for which, dt in AGENT_OUTS)
    obs = agent_observation(e, None if e._agent_ring else read_buffer(e, E.BUF_AGENT_OBS, (n, oh, ow, stack), stream=stream), stream=stream)
    ended = ended != 0
    return obs, reward, done != 0, ended, np.where(ended, ret, 0), np.where(ended, length, 0)


def run_agent_on_streams(es, mems, streams, game, t0, t1):
    """run_agent through the entry points of a policy loop: tbx_agent_step_synthetic (even t) and tbx_agent_step_device (odd t: the
    same actions, uploaded) on each engine's stream, the outputs read where they lie; -> the last engine's rows"""
    n = es[0].n_envs
    rows = []
    for t in range(t0, t1):
        outs = []
        for e, mem, s in zip(es, mems, streams):
            sp = s.ptr if s is not None else 0
            if t % 2 == 0:
                e.agent_step_synthetic(ACTION_SEED, t, stream=sp)
            else:
                e.agent_step_device(mem.put(synthetic_actions(game, n, t, seed=ACTION_SEED).astype(np.int32)), stream=sp)
            outs.append(stream_outputs(e, s))
        for x, y, name in zip(outs[0], outs[-1], ROW_NAMES):
            if not np.array_equal(x, y):
                diff = np.moveaxis(x != y, 1, 0) if x.shape[0] != n else x != y
                bad = np.flatnonzero(diff.reshape(n, -1).any(axis=1))
                raise AssertionError("agent step %d (stream form): %s differs in %d envs, first %s" % (t, name, len(bad), bad[:8]))
        rows.append(outs[-1])
    codes = [e._lib.tbx_sync(e._h) for e in es]                     # (a step on an env that needed a reset is carried out all the same)
    assert codes[0] == codes[-1] and codes[-1] in (E.OK, E.E_NEEDS_RESET), codes
    return rows


def obs_by_env(obs, ring):
    """[N, h, w, k], oldest plane first, from a rolled stack (as it is) or (ring) from a ring read in head order [k, N, h, w]"""
    return np.moveaxis(obs, 0, -1) if ring else obs


# ---------------------------------------------------------------- 1. the writes

def walkable_tiles(cur, rng):
    """per env: a tile of the track, drawn from the board as it stands"""
    n = len(cur)
    ty, tx = np.nonzero(cur["tiles"][0] != 0)
    pick = rng.integers(0, len(tx), n)
    return tx[pick], ty[pick]


def edits_of(game):
    """name -> (picture-changing, builder(cur records, rng, second) -> (op, args, steps until the picture shows it)).  `second`:
    the write's second run (the device form) takes other arguments."""
    n_ = lambda cur: len(cur)
    common = {
        "lives down": (False, lambda cur, rng, second: (E.EDIT_SET_LIVES, np.maximum(cur["lives"] - 1, 1)[:, None].astype(np.float64), 1)),
        "lives up": (False, lambda cur, rng, second: (E.EDIT_SET_LIVES, (cur["lives"] + 1)[:, None].astype(np.float64), 1)),
        "score": (False, lambda cur, rng, second: (E.EDIT_SET_SCORE, (cur["score"] + (2000 if second else 1000) + np.arange(n_(cur)) % 7)[:, None].astype(np.float64), 1)),
        "level": (False, lambda cur, rng, second: (E.EDIT_SET_LEVEL, (cur["level"] + 1)[:, None].astype(np.float64), 1)),
    }
    if game == "breakout":
        def ball(cur, rng, second):
            n = n_(cur)
            return E.EDIT_BRK_BALL, np.stack([np.zeros(n), rng.uniform(40, 200, n), rng.uniform(60, 120, n), rng.choice([-1.5, 1.25], n),
                                              rng.choice([-1.75, 1.5], n)], axis=1), 1
        own = {
            "column": (True, lambda cur, rng, second: (E.EDIT_BRK_COLUMN_ALIVE, np.stack([rng.integers(0, 18, n_(cur)), np.zeros(n_(cur))], axis=1).astype(np.float64), 1)),
            "row": (True, lambda cur, rng, second: (E.EDIT_BRK_ROW_ALIVE, np.stack([rng.integers(0, 6, n_(cur)), np.zeros(n_(cur))], axis=1).astype(np.float64), 1)),
            "all": (True, lambda cur, rng, second: (E.EDIT_BRK_ALL_ALIVE, (cur["bricks"]["alive"][:, :108].sum(axis=1) < 54)[:, None].astype(np.float64), 1)),
            "brick": (True, lambda cur, rng, second: (E.EDIT_BRK_BRICK_ALIVE, np.stack([rng.integers(0, 108, n_(cur)), np.zeros(n_(cur))], axis=1).astype(np.float64), 1)),
            "paddle": (True, lambda cur, rng, second: (E.EDIT_BRK_PADDLE, np.stack([rng.uniform(30, 210, n_(cur)), cur["paddle_y"]][:2 if second else 1], axis=1), 1)),
            "ball": (True, ball),
        }
    elif game == "amidar":
        def tile(cur, rng, second):
            tx, ty = walkable_tiles(cur, rng)
            tag = np.where(cur["tiles"][np.arange(n_(cur)), ty, tx] == 2, 1, 2)
            return E.EDIT_AMI_TILE, np.stack([tx, ty, tag], axis=1).astype(np.float64), 1

        def player_tile(cur, rng, second):
            tx, ty = walkable_tiles(cur, rng)
            return E.EDIT_AMI_PLAYER_TILE, np.stack([tx, ty], axis=1).astype(np.float64), 1

        def random_start(cur, rng, second):
            n = n_(cur)
            return E.EDIT_AMI_PLAYER_RANDOM_START, np.stack([np.full(n, 9 + second), np.arange(n) % 11, np.full(n, 123456), np.full(n, 6)], axis=1).astype(np.float64), 1

        def enemy_ai(cur, rng, second):
            n = n_(cur)
            row = np.zeros((n, 15))
            row[:, 0] = rng.integers(0, 5, n)                           # the enemy
            row[:, 1] = E.AI_NAMES.index("EnemyRandomMvmt" if second else "EnemyTargetPlayer")
            row[:, 4], row[:, 5] = 12, 12                              # start tile
            row[:, 10] = row[:, 11] = rng.integers(0, 4, n)            # start_dir, dir
            row[:, 12] = 9                                             # vision_distance
            row[:, 13] = row[:, 14] = -1                               # nothing seen
            return E.EDIT_AMI_ENEMY_AI, row, STEPS_PER_WRITE

        own = {
            "tile": (True, tile), "player tile": (True, player_tile), "player random start": (True, random_start), "enemy ai": (True, enemy_ai),
            "timers": (True, lambda cur, rng, second: (E.EDIT_AMI_TIMERS, np.stack([np.where(np.arange(n_(cur)) % 3 == 0, -1, 40 + np.arange(n_(cur)) % 50),
                                                                                   np.where(np.arange(n_(cur)) % 3 == 1, -1, 60 + np.arange(n_(cur)) % 9)], axis=1).astype(np.float64), STEPS_PER_WRITE)),
            "jumps": (True, lambda cur, rng, second: (E.EDIT_AMI_JUMPS, ((cur["jumps"] + 1 + np.arange(n_(cur)) % 3) % 6)[:, None].astype(np.float64), STEPS_PER_WRITE)),
        }
    else:
        own = {"ufo appearance": (True, lambda cur, rng, second: (E.EDIT_SI_UFO_APPEARANCE, (np.arange(n_(cur)) % 3)[:, None].astype(np.float64), STEPS_PER_WRITE))}
    own.update(common)
    return own


class Case:
    """one run of the script: the engines under comparison `es` (the last one the oracle), the control engine or None"""

    def __init__(self, game, es, control, new_plane, wrappers, skip, oracle_lib, twin):
        self.game, self.es, self.control, self.twin = game, es, control, twin
        self.first_steps, self.steps_per_write = FIRST_STEPS, STEPS_PER_WRITE
        self.o = es[-1]
        self.n = self.o.n_envs
        self.episodic = wrappers["episodic_life"]
        self.clip = wrappers["clip_reward"]
        self.all = es + ([control] if control is not None else [])
        for e in self.all:
            e.seed(SEED)
            e.agent_init(skip=skip, out_h=84, out_w=84, stack=4, new_plane=new_plane if e is not control else 0, **wrappers)
            e.agent_reset()
        write_mid_game_states(self.all, self.n, donor_records(game, oracle_lib))
        self.mems = [Memory(e) for e in self.all]
        self.streams = [None] * len(self.all)
        if not engine_is_oracle(es[0]):
            from toybox_amd import hip
            self.streams[0] = hip.Stream()
        self.t = 0
        self.rng = np.random.default_rng(5)
        self.seen = {}

    def close(self):
        for e, mem, s in zip(self.all, self.mems, self.streams):
            e._lib.tbx_sync(e._h)
            mem.release()
            if s is not None:
                s.close()
        _close(self.all)

    def steps(self, count, on_streams):
        """`count` agent steps on every engine -> (the oracle's rows, the control's)"""
        t0, t1 = self.t, self.t + count
        self.t = t1
        k = len(self.es)
        if on_streams:
            rows = run_agent_on_streams(self.es, self.mems[:k], self.streams[:k], self.game, t0, t1)
            ctl = run_agent_on_streams([self.control], self.mems[k:], [None], self.game, t0, t1) if self.control is not None else None
        else:
            rows = run_agent(self.es, self.game, t0, t1, action_seed=ACTION_SEED, tolerate_needs_reset=True)[2]
            ctl = run_agent([self.control], self.game, t0, t1, action_seed=ACTION_SEED, tolerate_needs_reset=True)[2] if self.control is not None else None
        return rows, ctl

    def edit(self, name, second):
        """one tbx_edit op in every engine but the control -- host form, or (second) the device-pointer form on the stream with no
        synchronisation before the next agent step -- then STEPS_PER_WRITE agent steps and the write's conditions"""
        picture, build = edits_of(self.game)[name]
        cur = self.o.get_states_np()
        op, args, horizon = build(cur, self.rng, second)
        horizon = min(horizon, self.steps_per_write)
        mask = self.rng.random(self.n) < 0.5
        before = self.o.render(1) if picture and horizon == 1 else None
        for e, mem, s in zip(self.es, self.mems, self.streams):
            if second:
                device_edit(e, mem, op, args, mask, stream=s.ptr if s is not None else 0, byte=255)
            else:
                host_edit(e, op, args, mask)
        if self.twin:
            records_equal(self.o.get_states_np(), numpy_edit(self.game, cur, op, args, mask), "%s (%s form)" % (name, "device" if second else "host"))
        what = "%s %s (%s form)" % (self.game, name, "device" if second else "host")
        sel = np.flatnonzero(mask)
        if before is not None:                                        # the frame of the written state against the frame before the write
            changed = int((self.o.render(1)[sel] != before[sel]).reshape(len(sel), -1).any(axis=1).sum())
            self.seen[what + " frame"] = "%d of %d" % (changed, len(sel))
            assert 2 * changed >= len(sel), "%s: the frame changed in %d of %d selected envs" % (what, changed, len(sel))
        rows, ctl = self.steps(self.steps_per_write, on_streams=second)
        # conditions on the oracle's own rows (asserted in the device cases too), then those against the control (the twins)
        after = to_int(arg_rows(args, self.n)[:, 0])
        if name == "lives down" and self.episodic:
            fell = mask & (after < cur["lives"])
            self.seen[what] = "%d envs" % fell.sum()
            assert fell.sum() >= 16 and rows[0][2][fell].all(), "%s: a drop in lives was not reported as done" % what
        if name == "lives up":
            rose = mask & (after > cur["lives"])
            lost = rows[0][3] != 0                                    # (the Monitor saw a real game over)
            assert rose.sum() >= 16 and not rows[0][2][rose & ~lost].any(), "%s: done after an increase in lives" % what
        if name == "score":                                           # (the step's reward is the jump plus what play gave, never less)
            got = rows[0][1][sel]
            self.seen[what] = "rewards %s" % np.unique(got)[:4]
            assert (got == 1).all() if self.clip else (got >= 1000).all(), "%s: the reward does not show the jump" % what
        if ctl is None:
            return
        if picture:
            x, y = obs_by_env(rows[horizon - 1][0], self.o._agent_ring)[sel], obs_by_env(ctl[horizon - 1][0], self.control._agent_ring)[sel]
            changed = int((x != y).reshape(len(sel), -1).any(axis=1).sum())
            self.seen[what + " observation"] = "%d of %d" % (changed, len(sel))
            assert 2 * changed >= len(sel), "%s: the observation changed in %d of %d selected envs" % (what, changed, len(sel))
        if name == "score":
            got, base = rows[0][1][sel], ctl[0][1][sel]
            if self.clip:
                # Not "differs in every selected env": under clip_reward the jump reads sign(jump + play) = +1, and play alone gives
                # the control +1 in some envs.  What clipping leaves to assert: +1 everywhere (above), and a difference wherever
                # the control's reward is not +1.
                assert (got != base)[base != 1].all(), "%s: the clipped reward equals the control's where that is not +1" % what
            else:
                assert (got != base).all(), "%s: the reward of a selected env equals the control's" % what

    def script(self, forms):
        """forms: "host" -- every edit in the host form, then the writes that have no other; "device" -- every edit as tbx_edit_device"""
        self.steps(self.first_steps, on_streams=False)
        for name in edits_of(self.game):
            for form in forms:
                self.edit(name, second=form == "device")
        if "host" not in forms:
            return self.end()
        n, o = self.n, self.o
        # tbx_set_states on a range in the middle of the batch: the records of other envs of the same batch (canonical, mid-game)
        rec = o.get_states_np(100, 411)
        for e in self.es:
            e.set_states_np(303, rec)
        self.steps(self.steps_per_write, on_streams=False)
        mask = self.rng.random(n) < 0.5
        for e in self.es:
            e.new_game(mask)
        self.steps(self.steps_per_write, on_streams=True)
        seeds = self.rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        for e in self.es:
            e.seed_array(seeds)
        for e in self.es:
            e.new_game(~mask)                                         # (the new seeds show in the games that start from here)
        self.steps(self.steps_per_write, on_streams=False)
        self.end()

    def end(self):
        for e in self.es:
            e._lib.tbx_sync(e._h)
        _same_states(self.es, "%s at the end" % self.game)
        _same_rngs(self.es, "%s simulator RNGs at the end" % self.game)
        for x, y in zip(self.es[0].scalars(), self.o.scalars()):
            assert np.array_equal(x, y)


WRITE_CASES = [(g, p, w, 4, 0) for g in GAMES for p in (0, 2) for w in ("bare", "full")] + \
              [("breakout", 2, "full", 2, 0), ("space_invaders", 0, "full", 2, 0), ("amidar", 0, "bare", 2, 0)] + \
              [("amidar", 0, "full", 4, E.STEP_FORM_THREAD_PER_ENV)]       # (the one agent kernel that reads the movers' mirror; a batch this small does not choose it)


def run_write_case(game, new_plane, wrappers, skip, forms, libs, oracle_lib, twin, step_form=0):
    es = [Engine(game, N, lib=lib) for lib in libs]
    control = Engine(game, N, lib=oracle_lib) if twin else None
    for e in es if step_form else []:
        e.set_option(E.OPT_STEP_FORM, step_form)
    case = Case(game, es, control, new_plane, BARE if wrappers == "bare" else FULL, skip, oracle_lib, twin)
    try:
        case.script(forms)
    finally:
        case.close()
    return case.seen


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("game,new_plane,wrappers,skip,step_form", WRITE_CASES)
def test_gpu_writes_between_agent_steps(game, new_plane, wrappers, skip, step_form, form, hip_lib, oracle_lib):
    """the script of part 1 on the device and on the oracle, one form of the edits per case; the conditions that need no control
    engine are asserted here too, on the oracle's rows (the control engine runs in the twin)"""
    run_write_case(game, new_plane, wrappers, skip, (form,), (hip_lib, oracle_lib), oracle_lib, twin=False, step_form=step_form)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("game,wrappers,skip", [(g, w, 4) for g in GAMES for w in ("bare", "full")])
def test_writes_between_agent_steps_on_the_checker(game, wrappers, skip, form, oracle_lib):
    """the script of the device case of the same name -- same step counts, one form, so the same states, masks and arguments -- over
    the oracle and the control engine that gets no write: every batched edit leaves the records numpy leaves, and the conditions of
    the module's docstring hold"""
    seen = run_write_case(game, 0, wrappers, skip, (form,), (oracle_lib,), oracle_lib, twin=True)
    print(seen)


# ---------------------------------------------------------------- 1b. a game that ends in frame 0 or 1 of the step after the write

def stale_states(game, engines, oracle_lib):
    """written into every engine: states that are one to three frames from losing a life; -> the envs written"""
    o, n = engines[-1], N
    i = np.arange(n)
    if game == "breakout":                                            # the ball below the paddle: from 161.5 down it is gone in frame 0, at 161 and
        fall = falling_ball_states(oracle_lib, n)                     # 160.5 in frame 1, then a frame later per pixel
        fall["ball_y"][:, 0] = 162.0 - 0.5 * (i % 8)
        sel = i % 3 != 1                                              # (the other envs stay in their mid-game states)
        st = o.get_states_np()
        st[sel] = fall[sel]
    elif game == "space_invaders":                                    # the ship's explosion one to three frames from its end
        st = o.get_states_np()
        sel = i % 4 != 3
        st["life_display_timer"][sel] = 0
        st["ship_alive"][sel] = 0
        st["ship_death_counter"][sel] = (1 + i % 3)[sel]
    else:                                                             # every enemy on the player, the jump one to three frames from its end
        cd = codec("amidar")
        sel = (i % 21 == 5) & (i < 21 * 48)                           # 48 envs, some in every block of the launch
        for k in np.flatnonzero(sel):
            rec = cd.state_from_json(amidar_edit_last_lives(cd.state_to_json(o.get_state(int(k))), lives=3, jump_timer=1 + int(k) // 21 % 3,
                                                            perimeter_from_start=True))
            for e in engines:
                e.set_state(int(k), rec)
        return sel
    for e in engines:
        e.set_states_np(0, st)
    return sel


def ends_in_the_first_two_frames(o, game, t, oracle_lib):
    """bool[N]: a clone of the oracle's batch, played two raw frames with the actions of agent step t, has no lives left"""
    from lookahead_replay import clone_of
    c = clone_of(oracle_lib, o)
    a = synthetic_actions(game, o.n_envs, t, seed=ACTION_SEED)
    over = np.zeros(o.n_envs, bool)
    for _ in range(2):
        over |= c.step(a, auto_reset=False)[2] <= 0
    c.close()
    return over


def run_stale_case(game, new_plane, libs, oracle_lib, twin):
    """agent steps, the states of stale_states, TBX_EDIT_SET_LIVES 1 (new_plane 2: as tbx_edit_device on the stream), agent steps:
    MaxAndSkipEnv's buffer holds snapshots from before the write when the game ends; -> envs whose game ended in frame 0 or 1"""
    es = [Engine(game, N, lib=lib) for lib in libs]
    case = Case(game, es, None, new_plane, FULL, 4, oracle_lib, twin)
    try:
        case.steps(4, on_streams=False)
        sel = stale_states(game, es, oracle_lib)
        ready = ~read_buffer(case.o, E.BUF_AGENT_DONE, (N,)).astype(bool)     # (a done env starts its next step with a reset)
        for e, mem, s in zip(es, case.mems, case.streams):
            if new_plane == 2:
                device_edit(e, mem, E.EDIT_SET_LIVES, [1.0], sel, stream=s.ptr if s is not None else 0)
            else:
                host_edit(e, E.EDIT_SET_LIVES, [1.0], sel)
        early = sel & ready & ends_in_the_first_two_frames(case.o, game, case.t, oracle_lib)
        rows, _ = case.steps(6, on_streams=new_plane == 2)
        assert early.sum() >= 16, "the game ends in frame 0 or 1 in %d envs only" % early.sum()
        assert rows[0][2][early].all() and rows[0][3][early].all(), "a game that ended in frame 0 or 1 was not reported as over"
        case.end()
        assert_same_end_state(case.o, es[:-1], N, "%s stale snapshots" % game)
    finally:
        case.close()
    return early


@pytest.mark.gpu
@pytest.mark.parametrize("new_plane", [0, 2])
@pytest.mark.parametrize("game", GAMES)
def test_gpu_game_over_in_the_first_frames_after_a_write(game, new_plane, hip_lib, oracle_lib):
    run_stale_case(game, new_plane, (hip_lib, oracle_lib), oracle_lib, twin=False)


@pytest.mark.parametrize("game", GAMES)
def test_game_over_in_the_first_frames_after_a_write_on_the_checker(game, oracle_lib):
    """the directed states do what they are for: in at least 16 envs the game ends inside frame 0 or 1 of the agent step after the
    write, and that step reports done and a finished episode there"""
    early = run_stale_case(game, 0, (oracle_lib,), oracle_lib, twin=True)
    print("%s: the game ends in frame 0 or 1 in %d envs" % (game, early.sum()))
    assert early.sum() >= 16, early.sum()


# ---------------------------------------------------------------- 2. the first frame after a write, on a plain engine

READERS = ("render 3", "render 1", "fused", "chunk", "lookahead")
PLAIN_CASES = [("breakout", 0), ("breakout", E.STEP_FORM_WAVE_PER_ENV), ("amidar", E.STEP_FORM_THREAD_PER_ENV), ("amidar", E.STEP_FORM_WAVE_PER_ENV),
               ("space_invaders", 0)]


def packed_equal(g, o, stream, what, rows=None):
    n = o.n_envs
    got = read_buffer(g, E.BUF_PACKED, (n,), np.uint64, stream=stream) if rows is None else rows
    assert np.array_equal(got, read_buffer(o, E.BUF_PACKED, (n,), np.uint64)), what


def read_first(g, o, reader, t, stream, chks, oracle_lib, what):
    """one reader as the first call after a write on the device engine g, against the oracle o (g is None: the twin, which only
    moves the oracle on); -> frames stepped"""
    n, H, W = o.n_envs, o.height, o.width
    sp = stream.ptr if stream is not None else 0
    if reader.startswith("render"):
        ch = int(reader[-1])
        if g is not None:
            g.render_device(0, ch, stream=sp)
            stream.synchronize()
            p, nbytes = g.device_buffer(E.BUF_FRAME)
            assert nbytes >= n * H * W * ch
            chks[ch].compare(device_frames(p, H * W * ch), oracle_frames(o, ch), n, what=what)
        return 0
    if reader == "lookahead":
        if g is not None:
            want = expected(oracle_lib, o.game, o.get_states(), sim_rngs(o), dict(frames=8, seed=5, t=t), all_actions=True)
            assert_fields_equal(g.lookahead_all(8, seed=5, t=t), want, what)
        return 0
    k = 1 if reader == "fused" else 2
    if g is not None:
        fb = H * W * 3
        if k == 1:
            g.render_step_synthetic(ACTION_SEED, t, channels=3, auto_reset=True, stream=sp)
        else:
            g.rollout_synthetic(ACTION_SEED, t, k, channels=3, auto_reset=True, stream=sp)
        stream.synchronize()
        f, nbytes = g.device_buffer(E.BUF_FRAME if k == 1 else E.BUF_ROLLOUT_FRAMES)
        assert nbytes >= k * n * fb
        packed = read_buffer(g, E.BUF_PACKED if k == 1 else E.BUF_ROLLOUT_PACKED, (k, n), np.uint64, stream=stream)
    for j in range(k):
        if g is not None:
            chks[3].compare(device_frames(f + j * n * fb, fb), oracle_frames(o, 3), n, n=n, frame0=j * n, what="%s frame %d" % (what, j))
        o.step_synthetic(ACTION_SEED, t + j, auto_reset=True)
        if g is not None:
            packed_equal(g, o, stream, "%s step %d" % (what, j), rows=packed[j])
    return k


def run_first_frames(game, step_form, libs, oracle_lib, twin):
    es = [Engine(game, N, lib=lib) for lib in libs]
    o = es[-1]
    g = None if twin else es[0]
    stream = None
    if g is not None:
        from toybox_amd import hip
        stream = hip.Stream()
    mems = [Memory(e) for e in es]
    sp = stream.ptr if stream is not None else 0
    chks = {ch: FrameChecker((o.height, o.width, ch)) for ch in (1, 3)}
    rng = np.random.default_rng(9)
    seen = {}
    try:
        for e in es:
            if step_form:
                e.set_option(E.OPT_STEP_FORM, step_form)
            e.seed(SEED)
            e.new_game()
        write_mid_game_states(es, N, donor_records(game, oracle_lib))
        t = 0

        def step(count):
            nonlocal t
            for _ in range(count):
                if g is not None:
                    g.step_synthetic(ACTION_SEED, t, auto_reset=True, stream=sp)
                o.step_synthetic(ACTION_SEED, t, auto_reset=True)
                if g is not None:
                    packed_equal(g, o, stream, "%s batch step %d" % (game, t))
                t += 1

        step(10)
        for name, (picture, build) in edits_of(game).items():         # (lives, score and level too: SpaceInvaders paints its lives)
            for r, reader in enumerate(READERS):
                step(1)                                               # step-written render records are in force again
                cur = o.get_states_np()
                op, args, horizon = build(cur, rng, bool(r % 2))
                mask = rng.random(N) < 0.5
                before = o.render(1) if twin and picture and horizon == 1 else None
                for e, mem in zip(es, mems):
                    if r % 2:
                        device_edit(e, mem, op, args, mask, stream=sp if e is g else 0, byte=2)
                    else:
                        host_edit(e, op, args, mask)
                what = "%s form %d, %s read first after %s" % (game, step_form, reader, name)
                if twin:
                    records_equal(o.get_states_np(), numpy_edit(game, cur, op, args, mask), what)
                if before is not None:
                    sel = np.flatnonzero(mask)
                    changed = int((o.render(1)[sel] != before[sel]).reshape(len(sel), -1).any(axis=1).sum())
                    seen[what] = "%d of %d" % (changed, len(sel))
                    assert 2 * changed >= len(sel), "%s: the frame changed in %d of %d selected envs" % (what, changed, len(sel))
                t += read_first(g, o, reader, t, stream, chks, oracle_lib, what)
            step(20)
        for e in es:
            e.sync()
        _same_states(es, "%s at the end" % game)
        _same_rngs(es, "%s simulator RNGs at the end" % game)
    finally:
        for e, mem in zip(es, mems):
            e._lib.tbx_sync(e._h)
            mem.release()
        if stream is not None:
            stream.close()
        _close(es)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("game,step_form", PLAIN_CASES)
def test_gpu_first_frame_after_a_write(game, step_form, hip_lib, oracle_lib):
    """part 2 of the module's docstring; Amidar on both forms of its step kernel, Breakout also on the wave-per-env one"""
    run_first_frames(game, step_form, (hip_lib, oracle_lib), oracle_lib, twin=False)


@pytest.mark.parametrize("game", GAMES)
def test_first_frame_after_a_write_on_the_checker(game, oracle_lib):
    """the same writes on the oracle alone: each leaves the records numpy leaves, and those that show at once change the frame of at
    least half the selected envs"""
    print(run_first_frames(game, 0, (oracle_lib,), oracle_lib, twin=True))


# ---------------------------------------------------------------- 3. edges of the edit and query kernels

EDGE_SIZES = [1, 65, 257, 1027]
BAD_KEYS = lambda count: [-1.0, float(count), 255.0, 256.0, 1e12, float("nan")]     # brick, column and row keys nothing answers to
SENTINEL = np.uint64(0x7FF8C0DEC0DEC0DE)                                           # (a NaN: no query writes this bit pattern)


def edge_engines(game, n, wall, libs):
    """engines with the same mid-game batch: 60 frames of play from a new game; wall = "custom": Breakout with a generated brick table
    of up to 256 bricks in every env (tests/test_gpu_custom_states.py, kind 1)"""
    from test_gpu_custom_states import gen_breakout
    es = [Engine(game, n, lib=lib) for lib in libs]
    for e in es:
        e.seed(SEED + n)
        e.new_game()
        for t in range(60):
            e.step_synthetic(ACTION_SEED, t, auto_reset=True)
        e.sync()
    if wall == "custom":
        st = gen_breakout(es[-1].get_states_np(), np.random.default_rng(n), [1] * n)
        st["n_bricks"] = np.asarray([256, 129, 192, 255, 128, 108, 64, 1])[np.arange(n) % 8]      # (every slot of such a table is filled)
        st["bricks"]["col"][:, 3] = 255                                # (a column key of BAD_KEYS that a brick does answer to)
        for e in es:
            e.set_states_np(0, st)
    return es


def cycle(values, n, shift=0):
    return np.asarray(values, np.float64)[(np.arange(n) + shift) % len(values)]


def edge_edits(game, cur, rng):
    """[(op, shared arguments, per-env rows, per-env rows outside the range or None)] for the records `cur`"""
    n = len(cur)
    i = np.arange(n)
    rows = lambda *cols: np.stack([np.broadcast_to(np.asarray(c, np.float64), (n,)) for c in cols], axis=1)
    out = [(E.EDIT_SET_LIVES, [2], rows(1 + i % 4), None), (E.EDIT_SET_SCORE, [777], rows(3 * i), None), (E.EDIT_SET_LEVEL, [2], rows(1 + i % 3), None)]
    if game == "breakout":
        B = cur["bricks"]
        inb = np.arange(E.BRK_MAX_BRICKS)[None, :] < cur["n_bricks"][:, None]
        count = lambda f: int(np.where(inb, B[f], 0).max()) + 1
        nb = np.maximum(cur["n_bricks"], 1)
        out += [
            (E.EDIT_BRK_COLUMN_ALIVE, [4, 0], rows(rng.integers(0, 18, n), i % 2), rows(cycle(BAD_KEYS(count("col")), n), (i + 1) % 2)),
            (E.EDIT_BRK_ROW_ALIVE, [2, 0], rows(rng.integers(0, 6, n), i % 2), rows(cycle(BAD_KEYS(count("row")), n), (i + 1) % 2)),
            (E.EDIT_BRK_ALL_ALIVE, [0], rows(i % 2), None),
            (E.EDIT_BRK_BRICK_ALIVE, [107, 0], rows(rng.integers(0, nb), i % 2),
             rows(np.where(i % 6 == 1, cur["n_bricks"], cycle(BAD_KEYS(0), n)), 1 - (B["alive"][:, 255] != 0))),
            (E.EDIT_BRK_PADDLE, [100.5], rows(40.25 + i % 150, 140.0 + i % 3), None),
            (E.EDIT_BRK_BALL, [0, 60.0, 90.0, 1.0, -1.5], rows(i % 4, rng.uniform(40, 200, n), rng.uniform(60, 120, n), 1.25, -1.75),
             rows(np.where(i % 3 == 1, cur["n_balls"], cycle([-1, 0, 4], n)), 7.0, 8.0, 9.0, 10.0)),
        ]
    elif game == "amidar":
        tx, ty = walkable_tiles(cur, rng)
        ai = lambda slot: rows(slot, 2 + i % 4, 0, 0, i % 32, i % 31, i % 4, i % 4, i % 4, i % 4, i % 4, i % 4, 3 + i % 9, -1, -1)
        out += [
            (E.EDIT_AMI_TIMERS, [75, -1], rows(i % 50, 300 - i % 7), rows(-1, -1)),
            (E.EDIT_AMI_JUMPS, [5], rows(i % 6), None),
            (E.EDIT_AMI_TILE, [5, 6, 2], rows(tx, ty, 1 + i % 3), rows(cycle([-1, 32, 5, 5], n), cycle([6, 6, -1, 31], n), 3)),
            (E.EDIT_AMI_ENEMY_AI, [1, 4, 0, 0, 0, 30, 0, 0, 0, 0, 3, 0, 9, -1, -1], ai(i % 5), ai(np.where(i % 3 == 1, cur["n_enemies"], cycle([-1, 0, 16], n)))),
            (E.EDIT_AMI_PLAYER_TILE, [31, 15], rows(tx, ty), None),
            (E.EDIT_AMI_PLAYER_RANDOM_START, [3, 0, 0, 12], rows(21, i % 7, 123456, 4 + i % 9), rows(21, i % 7, 0, 200)),   # nobody is 200 tiles away
        ]
    else:
        out += [(E.EDIT_SI_UFO_APPEARANCE, [-1], rows(i % 5 - 1), None)]
    return out


def in_range(game, op, cur, bad):
    """bool[N]: the row of `bad` names something that exists in that env after all (key 255 on a wall with 256 bricks, ball 0)"""
    key = to_int(bad[:, 0])
    if op == E.EDIT_BRK_BRICK_ALIVE:
        return (key >= 0) & (key < cur["n_bricks"])
    if op == E.EDIT_BRK_BALL:
        return (key >= 0) & (key < cur["n_balls"])
    if op == E.EDIT_AMI_ENEMY_AI:
        return (key >= 0) & (key < cur["n_enemies"])
    if op in (E.EDIT_BRK_COLUMN_ALIVE, E.EDIT_BRK_ROW_ALIVE):
        f = "col" if op == E.EDIT_BRK_COLUMN_ALIVE else "row"
        return ((cur["bricks"][f] == key[:, None]) & (np.arange(E.BRK_MAX_BRICKS)[None, :] < cur["n_bricks"][:, None])).any(axis=1)
    return np.zeros(len(cur), bool)


def run_edge_edits(game, n, wall, libs, twin):
    es = edge_engines(game, n, wall, libs)
    o = es[-1]
    mems = [Memory(e) for e in es]
    rng = np.random.default_rng(n)
    try:
        for k, (op, shared, per_env, bad) in enumerate(edge_edits(game, o.get_states_np(), rng)):
            masks = [rng.random(n) < 0.5 for _ in range(4)]
            forms = [("shared", lambda e, m: host_edit(e, op, shared, None), shared, None),
                     ("shared, mask byte 2", lambda e, m: host_edit(e, op, shared, masks[0], byte=2), shared, masks[0]),
                     ("per env, mask byte 1", lambda e, m: host_edit(e, op, per_env, masks[1], byte=1), per_env, masks[1]),
                     ("device pointers, mask byte 255", lambda e, m: device_edit(e, m, op, per_env[::-1].copy(), masks[2], byte=255), per_env[::-1].copy(), masks[2])]
            if bad is not None:
                forms += [("per env out of range", lambda e, m: host_edit(e, op, bad, masks[3]), bad, masks[3]),
                          ("device pointers out of range", lambda e, m: device_edit(e, m, op, bad, None), bad, None)]
            for name, call, args, mask in forms:
                what = "%s n=%d edit %d, %s" % (game, n, op, name)
                cur = o.get_states_np()
                for e, m in zip(es, mems):
                    call(e, m)
                    e.sync()
                after = o.get_states_np()
                if twin:
                    records_equal(after, numpy_edit(game, cur, op, args, mask), what)
                    if "out of range" in name:
                        out = ~in_range(game, op, cur, args)
                        assert out.sum() * 2 >= n, what                # (most rows do name nothing)
                        records_equal(after[out], cur[out], what + ": an env whose row names nothing changed")
                else:
                    records_equal(es[0].get_states_np(), after, what)
    finally:
        for e, m in zip(es, mems):
            e.sync()
            m.release()
        _close(es)


def edge_queries(game, cur, rng):
    """[(query, shared arguments, per-env rows or None, the answer nothing-there rows must get or None)]; the per-env rows of a query
    with such an answer name nothing in any env"""
    n = len(cur)
    i = np.arange(n)
    rows = lambda *cols: np.stack([np.broadcast_to(np.asarray(c, np.float64), (n,)) for c in cols], axis=1)
    if game == "space_invaders":
        return [(E.QUERY_SI_SHIP, [], None, None)]
    if game == "breakout":
        B = cur["bricks"]
        inb = np.arange(E.BRK_MAX_BRICKS)[None, :] < cur["n_bricks"][:, None]
        absent = lambda f: [v for v in BAD_KEYS(int(np.where(inb, B[f], 0).max()) + 1) if not (np.where(inb, B[f], -7) == v).any()]
        words = rng.integers(0, 2 ** 32, (n, 8)).astype(np.float64)
        return [
            (E.QUERY_BRK_BRICKS_REMAINING, [], None, None), (E.QUERY_BRK_NUM_BRICKS, [], None, None),
            (E.QUERY_BRK_COLUMN, [4], rows(i % 18), None), (E.QUERY_BRK_COLUMN, [0], rows(cycle(absent("col"), n)), [-1.0] * 32),
            (E.QUERY_BRK_ROW, [1], rows(i % 6), None), (E.QUERY_BRK_ROW, [0], rows(cycle(absent("row"), n)), [-1.0] * 32),
            (E.QUERY_BRK_IS_CHANNEL, [3], rows(i % 18), None), (E.QUERY_BRK_IS_CHANNEL, [0], rows(cycle(absent("col"), n)), [0.0]),
            (E.QUERY_BRK_CHANNEL_COUNT, [18], None, None), (E.QUERY_BRK_FIND_CHANNEL, [18], None, None),
            (E.QUERY_BRK_PADDLE, [], None, None), (E.QUERY_BRK_BALLS, [], None, None),
            (E.QUERY_BRK_FIND_BRICK, [1, 0, 0xFFFF0000, 0, 0xF, 0, 0, 0, 0], np.concatenate([rows(i % 3 - 1), words], axis=1), None),
            (E.QUERY_BRK_FIND_BRICK, [-1, 0, 0, 0, 0x800, 0xFFFFFFFF, 0, 0, 0x80000000], np.concatenate([rows(i % 3 - 1), words * (np.arange(8) >= 3)], axis=1), None),
            (E.QUERY_BRK_FIND_BRICK, [-1], rows(i % 3 - 1, 0, 0, 0, 0, 0, 0, 0, 0), [-1.0]),
        ]
    tx, ty = walkable_tiles(cur, rng)
    off_x, off_y = cycle([-1, 32, 5, 5], n), cycle([6, 6, -1, 31], n)
    return [
        (E.QUERY_AMI_MODE, [], None, None), (E.QUERY_AMI_ANY_CAUGHT, [], None, None), (E.QUERY_AMI_PLAYER_TILE, [], None, None),
        (E.QUERY_AMI_PLAYER_ENEMY_DISTANCES, [], None, None), (E.QUERY_AMI_PLAYER_ON_PAINTED, [], None, None),
        (E.QUERY_AMI_TILE, [5, 6], rows(tx, ty), None), (E.QUERY_AMI_TILE, [0, 0], rows(off_x, off_y), [-1.0]),
        (E.QUERY_AMI_COUNT_TILES, [1], rows(i % 4), None),
        (E.QUERY_AMI_ADJACENT, [6, 6], rows(i % 32, i % 31), None), (E.QUERY_AMI_ADJACENT, [0, 0], rows(cycle([-2, 33], n), cycle([-2, 32], n)), [-1.0] * 4),
        (E.QUERY_AMI_ENEMY_DISTANCES, [9, 12], rows(off_x, off_y), None),
        (E.QUERY_AMI_PLAYER_NEAR_UNPAINTED, [4], rows(1 + i % 6), None),
        (E.QUERY_AMI_TILES_MASK, [2], rows(i % 16), None),
        (E.QUERY_AMI_RANDOM_TILE, [21, 5, 40, 14, 0], rows(21, i % 7, 99, 1 + i % 15, np.where(i % 2 == 0, 0, 6)), None),
        (E.QUERY_AMI_RANDOM_TILE, [1, 0, 0, 4, 200], rows(1, i % 7, 0, 15, 200), [-1.0, -1.0, -1.0, 0.0]),
        (E.QUERY_AMI_RANDOM_DIR, [2, 1, 0, 6, 6], rows(2, i % 5, 7, tx, ty), None),
        (E.QUERY_AMI_RANDOM_DIR, [2, 1, 0, -5, -5], rows(2, i % 5, 7, cycle([-2, 33], n), cycle([-2, 32], n)), [-1.0, 0.0]),
    ]


def device_reduce(e, mem, query, args, width):
    """tbx_reduce_device into n * width + 64 doubles, the last 64 a sentinel that must come back untouched -> float64[n, width]"""
    n = e.n_envs
    buf = np.full(n * width + 64, SENTINEL, np.uint64)
    p = mem.put(buf)
    a = np.ascontiguousarray(args, np.float64)
    if a.ndim == 2:
        e.reduce_device(query, p, per_env_ptr=mem.put(a), n_args=a.shape[1])
    else:
        e.reduce_device(query, p, list(a))
    e.sync()
    mem.fetch(p, buf)
    assert (buf[n * width:] == SENTINEL).all(), "query %d wrote behind its %d x %d doubles" % (query, n, width)
    return buf[:n * width].view(np.float64).reshape(n, width)


def same_answers(got, want, what):
    if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        raise AssertionError("%s: %d entries differ, first at env %d column %d: got %r, want %r" % ((what, len(bad)) + tuple(bad[0]) + (got[tuple(bad[0])], want[tuple(bad[0])])))


def run_edge_queries(game, n, wall, libs, twin):
    es = edge_engines(game, n, wall, libs)
    o = es[-1]
    mems = [Memory(e) for e in es]
    try:
        cur = o.get_states_np()
        for query, shared, per_env, nothing in edge_queries(game, cur, np.random.default_rng(n)):
            width = o.reduce_width(query)
            for name, args in (("shared", shared), ("per env", per_env)):
                if args is None:
                    continue
                what = "%s n=%d query %d, %s" % (game, n, query, name)
                want = o.reduce(query, args)
                assert want.shape == (n, width)
                same_answers(device_reduce(o, mems[-1], query, args, width), want, what + ": the oracle's two forms")
                if nothing is not None and name == "per env":
                    same_answers(want, np.broadcast_to(np.asarray(nothing), (n, width)).copy(), what + ": the answer for nothing")
                if not twin:
                    same_answers(es[0].reduce(query, args), want, what + ", host form")
                    same_answers(device_reduce(es[0], mems[0], query, args, width), want, what + ", device form")
        if twin and game == "breakout":                                    # a second formulation of the mask query, over the records
            words = np.random.default_rng(7).integers(0, 2 ** 32, (n, 8)).astype(np.uint64) * (np.arange(8) >= 4).astype(np.uint64)
            got = o.reduce(E.QUERY_BRK_FIND_BRICK, np.concatenate([np.ones((n, 1)), words.astype(np.float64)], axis=1))[:, 0]
            j = np.arange(E.BRK_MAX_BRICKS)
            hit = (((words[:, j // 32] >> (j % 32).astype(np.uint64)) & np.uint64(1)) != 0) & (j[None, :] < cur["n_bricks"][:, None]) & (cur["bricks"]["alive"] != 0)
            assert np.array_equal(got, np.where(hit.any(axis=1), hit.argmax(axis=1), -1))
            if wall == "custom":
                assert (got > 107).any(), "no answer past brick 107"
        _same_states(es, "queries change nothing")
    finally:
        for e, m in zip(es, mems):
            e.sync()
            m.release()
        _close(es)


EDGE_CASES = [(g, "canonical") for g in GAMES] + [("breakout", "custom")]


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
@pytest.mark.parametrize("game,wall", EDGE_CASES)
def test_gpu_every_edit_in_every_form(game, wall, n, hip_lib, oracle_lib):
    """every op of the game in six forms (module docstring, 3); all state records of both engines after each"""
    run_edge_edits(game, n, wall, (hip_lib, oracle_lib), twin=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
@pytest.mark.parametrize("game,wall", EDGE_CASES)
def test_gpu_every_query_row_by_row(game, wall, n, hip_lib, oracle_lib):
    """every query of the game, shared and per-env arguments, host form and device form with 64 sentinel doubles behind the rows"""
    run_edge_queries(game, n, wall, (hip_lib, oracle_lib), twin=False)


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("game,wall", EDGE_CASES)
def test_every_edit_in_every_form_on_the_checker(game, wall, n, oracle_lib):
    """the oracle's edits leave the records numpy leaves, and a row that names nothing leaves its env unchanged"""
    run_edge_edits(game, n, wall, (oracle_lib,), twin=True)


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("game,wall", EDGE_CASES)
def test_every_query_row_by_row_on_the_checker(game, wall, n, oracle_lib):
    """the oracle's two forms agree, rows that name nothing get the documented answer, the mask query agrees with numpy"""
    run_edge_queries(game, n, wall, (oracle_lib,), twin=True)
