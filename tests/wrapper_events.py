"""The agent wrapper stack a second time, in Python over raw engine calls, with a log of what every wrapper call met; and the builders
that put a lost life or a game over on a chosen raw frame of a chosen wrapper call (test support, like tests/rule_inputs.py; nothing here
touches a GPU).

Stack restates include/toybox_amd.h ("agent-side preprocessing") and oracle/orc_abi.c (base_step .. commit_obs) class by class over an
engine that has NO agent layer: tbx_step1 (one frame of one env, no auto-reset), tbx_new_game(mask), tbx_render_env(channels = 1) and the
area resize of tests/support.py.  All wrapper state is kept here, per env.  It is slow (a Python loop per env and frame): the batches that
use it are small.

The event log has one Event per env and wrapper call:

    call      "step" (the agent's own step), "noop_frames" (NoopResetEnv's frames after a real reset), "lost_life_noop_step"
              (EpisodicLifeEnv.reset after a lost life), "fire_step_1", "fire_step_2" (FireResetEnv.reset)
    f         the raw frame of the call at which a life went, or at which a call on a game already over stopped (None: neither)
    what      "nothing", "life_lost" (lives still > 0) or "game_over"
    stopped   the call was cut short at f (MaxAndSkipEnv leaves its loop only when the game is over)
    source    what the observation is made of once the call has returned: one of SOURCES

and every agent step (and the reset) records the source of the observation it returned, per env."""
import collections

import numpy as np

from support import LEGAL, area_resize_int, noop_count

CALLS = ("step", "noop_frames", "lost_life_noop_step", "fire_step_1", "fire_step_2")
# black: both slots of MaxAndSkipEnv's buffer still hold np.zeros; slot_a / slot_b: one of them has been written; max: both;
# live: the raw frame of a real reset (NoopResetEnv.reset's return value); kept: the buffer as FireResetEnv's step(2) left it, although a
# reset has run since
SOURCES = ("black", "slot_a", "slot_b", "max", "live", "kept")
OK, E_ACTION, E_NEEDS_RESET = 0, -5, -6

Event = collections.namedtuple("Event", "env t call f what stopped source")


class Stack:
    """fault: None, or one wrong reading of the stack (the comparison's self-checks): "step_after_done" keeps repeating the action once
    the game is over, "slot_a_late" writes slot A one frame late, "rewritten_buffer" returns the buffer as it is AFTER the reset that
    follows a life lost in FireResetEnv's step(2) -- which is also what DESIGN.md section 8 documents for the device's generic path."""

    def __init__(self, raw, skip=4, out_h=84, out_w=84, stack=4, clip_reward=False, episodic_life=False, fire_reset=False, noop_max=0,
                 noop_seed=0, env_offset=0, stack_fill=0, noops=None, fault=None, resize=area_resize_int):
        assert fault in (None, "step_after_done", "slot_a_late", "rewritten_buffer")
        self.raw, self.n, self.legal = raw, raw.n_envs, LEGAL[raw.game]
        self.skip, self.oh, self.ow, self.stack = skip, out_h, out_w, stack
        self.clip, self.episodic, self.fire, self.fill = bool(clip_reward), bool(episodic_life), bool(fire_reset), bool(stack_fill)
        self.noop_max, self.noop_seed, self.env_offset = noop_max, noop_seed, env_offset
        self.noops = None if noops is None else [int(k) for k in noops]
        self.fault, self.resize = fault, resize
        n, H, W = self.n, raw.height, raw.width
        self.buf = np.zeros((2, n, H, W), np.uint8)                      # MaxAndSkipEnv._obs_buffer: zeros at construction
        self.written = np.zeros((2, n), bool)
        score, lives = raw.scalars()[:2]
        self.prev_score, self.lives = score.copy(), lives.copy()         # ToyboxBaseEnv.score
        self.ep_ret, self.ep_len, self.ep_index = (np.zeros(n, np.int64) for _ in range(3))
        self.prev_lives = np.zeros(n, np.int64)
        self.was_real_done, self.needs_reset = np.ones(n, bool), np.zeros(n, bool)
        self.ep_done, self.ep_return, self.ep_length = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.int32)
        self.obs = np.zeros((n, out_h, out_w, stack), np.uint8)
        self.plane = np.zeros((n, out_h, out_w), np.uint8)
        self.head, self.t, self.code = 0, -1, OK
        self.log, self.cur, self.cur_source = [], [None] * n, [None] * n

    # ---------------------------------------------------------------- ToyboxBaseEnv
    def _frame(self, i):
        return self.raw.render_env(i, 1)[:, :, 0]

    def _base_step(self, i, action):
        _, _, lives, score = self.raw.step1(i, action)
        reward = max(score - int(self.prev_score[i]), 0)
        self.prev_score[i], self.lives[i] = score, lives
        return reward, lives <= 0

    def _base_reset(self, i):
        mask = np.zeros(self.n, np.uint8)
        mask[i] = 1
        self.raw.new_game(mask)
        score, lives = self.raw.scalars()[:2]
        self.prev_score[i], self.lives[i] = score[i], lives[i]

    def _note(self, i, call, f, what, stopped, source):
        self.cur_source[i] = source
        self.log.append(Event(i, self.t, call, f, what, stopped, source))

    # ---------------------------------------------------------------- NoopResetEnv
    def _noop_reset(self, i):
        self._base_reset(i)
        self.cur[i] = self._frame(i)
        k = 0
        if self.noops is not None and self.noops[i] > 0:
            k = self.noops[i]
        elif self.noop_max > 0:
            k = noop_count(self.noop_seed, self.env_offset + i, int(self.ep_index[i]) & 0xFFFFFFFF, self.noop_max)
        ended = None
        for j in range(k):
            _, done = self._base_step(i, 0)
            if done:
                self._base_reset(i)
                ended = j if ended is None else ended
        if k > 0:
            self.cur[i] = self._frame(i)
            self._note(i, "noop_frames", ended, "nothing" if ended is None else "game_over", False, "live")
        self.cur_source[i] = "live"

    # ---------------------------------------------------------------- MaxAndSkipEnv
    def _skip_step(self, i, action, call):
        total, done, f_event, what, stopped = 0, False, None, "nothing", False
        slot_a_frame = self.skip - 2 + (self.fault == "slot_a_late")
        for f in range(self.skip):
            before = self.lives[i]
            r, done = self._base_step(i, action)
            if f_event is None and self.lives[i] < before:
                f_event, what = f, "game_over" if done else "life_lost"
            elif f_event is None and done:                      # a step on a game that was over already: cut short, nothing lost
                f_event = f
            if f == slot_a_frame:
                self.buf[0, i], self.written[0, i] = self._frame(i), True
            if f == self.skip - 1:
                self.buf[1, i], self.written[1, i] = self._frame(i), True
            total += r
            if done and self.fault != "step_after_done":
                stopped = True
                break
        self.cur[i] = np.maximum(self.buf[0, i], self.buf[1, i])
        a, b = self.written[:, i]
        self._note(i, call, f_event, what, stopped, "max" if a and b else "slot_a" if a else "slot_b" if b else "black")
        return done, total

    # ---------------------------------------------------------------- bench.Monitor
    def _monitor_step(self, i, action, call):
        stale = self.needs_reset[i]
        done, total = self._skip_step(i, action, call)
        if stale:
            self.code = E_NEEDS_RESET
            return done, total
        self.ep_ret[i] += total
        self.ep_len[i] += 1
        if done:
            self.needs_reset[i] = True
            self.ep_done[i], self.ep_return[i], self.ep_length[i] = 1, float(self.ep_ret[i]), self.ep_len[i]
        return done, total

    def _monitor_reset(self, i):
        self.ep_ret[i] = self.ep_len[i] = 0
        self.needs_reset[i] = False
        self.ep_index[i] += 1
        self._noop_reset(i)

    # ---------------------------------------------------------------- EpisodicLifeEnv
    def _episodic_step(self, i, action, call):
        done, total = self._monitor_step(i, action, call)
        if not self.episodic:
            return done, total
        self.was_real_done[i] = done
        lives = int(self.lives[i])
        if lives < self.prev_lives[i] and lives > 0:
            done = True
        self.prev_lives[i] = lives
        return done, total

    def _episodic_reset(self, i):
        if not self.episodic:
            self._monitor_reset(i)
            return
        if self.was_real_done[i]:
            self._monitor_reset(i)
        else:
            self._monitor_step(i, 0, "lost_life_noop_step")           # its `done` is ignored
        self.prev_lives[i] = int(self.lives[i])

    # ---------------------------------------------------------------- FireResetEnv
    def _top_reset(self, i):
        self._episodic_reset(i)
        if not self.fire:
            return
        if self._episodic_step(i, self.legal[1], "fire_step_1")[0]:
            self._episodic_reset(i)
        if self._episodic_step(i, self.legal[2], "fire_step_2")[0]:
            keep = self.cur[i]
            self._episodic_reset(i)
            if self.fault == "rewritten_buffer":
                keep = np.maximum(self.buf[0, i], self.buf[1, i])
            self.cur[i], self.cur_source[i] = keep, "kept"

    # ---------------------------------------------------------------- WarpFrame + VecFrameStack
    def _commit(self, i, fresh):
        small = self.resize(self.cur[i], self.oh, self.ow)
        if fresh:
            self.obs[i, :, :, :-1] = small[:, :, None] if self.fill else 0
        else:
            self.obs[i, :, :, :-1] = self.obs[i, :, :, 1:].copy()
        self.obs[i, :, :, -1] = small
        self.plane[i] = small

    def _record(self, reward=None, done=None):
        return {"reward": reward, "done": done, "ep_done": self.ep_done.copy(), "ep_return": self.ep_return.copy(),
                "ep_length": self.ep_length.copy(), "code": self.code, "obs": self.obs.copy(), "plane": self.plane.copy(),
                "head": self.head, "source": list(self.cur_source)}

    # ---------------------------------------------------------------- the calls of the ABI
    def write_states(self, records):
        """tbx_set_states between agent steps: the wrappers' own state (the remembered score and lives among it) stays"""
        self.raw.set_states_np(0, records)
        self.lives = self.raw.scalars()[1].copy()

    def reset(self):
        self.head = (self.head + 1) % self.stack
        for i in range(self.n):
            self._top_reset(i)
            self._commit(i, True)
        self.ep_done[:] = 0
        return self._record()

    def step(self, actions):
        self.t += 1
        self.head = (self.head + 1) % self.stack
        self.code = OK
        bad = False
        reward, done_out = np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)
        for i in range(self.n):
            a = int(actions[i])
            if not 0 <= a < 18:
                a, bad = 0, True
            self.ep_done[i] = 0
            done, total = self._episodic_step(i, a, "step")
            reward[i] = ((total > 0) - (total < 0)) if self.clip else total
            done_out[i] = done
            if done:
                self._top_reset(i)
            self._commit(i, done)
        if bad and self.code == OK:                      # (a step on an env that needed a reset outranks an illegal id: tbx_sync)
            self.code = E_ACTION
        return self._record(reward, done_out)


# ================================================================ the cells

def cell_of(event):
    """(call, f, what): the matrix's cell of one log entry; NoopResetEnv's frames are one cell, "in", whichever frame ended the game"""
    return (event.call, "in" if event.call == "noop_frames" and event.f is not None else event.f, event.what)


def cell_counts(log, t_first=0):
    """{cell: set of envs} over the entries of agent steps >= t_first (-1: the first reset too), nothing-cells left out"""
    out = {}
    for ev in log:
        if ev.t >= t_first and ev.what != "nothing":
            out.setdefault(cell_of(ev), set()).add(ev.env)
    return out


def first_event_cell(log, n):
    """per env, the cell of its first entry in which something happened at or after agent step 0 (None: nothing ever did)"""
    out = [None] * n
    for ev in log:
        if ev.t >= 0 and ev.what != "nothing" and out[ev.env] is None:
            out[ev.env] = cell_of(ev)
    return out


# ================================================================ builders: build_<game>_event(records, n, skip) -> records
# Env i gets the event of slot c = i % (8 * skip): raw frame F = c // 2 after the write (F // skip = the wrapper call it falls in when a
# reset procedure follows the first step at once: step, lost_life_noop_step, fire_step_1, fire_step_2; F % skip = the frame of that call),
# and the kind c % 2: 0 the last life (game over), 1 the last but one (a lost life).  Neighbouring envs differ in both.  The lives written
# (1 or 2) are below what EpisodicLifeEnv remembers from the reset (5 / 3 / 3), so with that wrapper on the first step after the write
# reports done and the reset procedure runs from the written state.  The actions of the steps that follow are event_actions().

def event_slot(i, skip):
    c = np.asarray(i) % (8 * skip)
    return c // 2, c % 2


def event_actions(game, n):
    """the action every env repeats in the steps after the write: the no-op (a ship, a paddle and a player that stay where the builder
    put them), in GridWorld RIGHT along the corridor"""
    return np.full(n, 3 if game == "gridworld" else 0, np.int32)


def build_breakout_event(st, n, skip):
    """one ball left of the paddle's reach and below its upper edge, falling one pixel per frame: it has left the screen (y - radius >
    160) after exactly F + 1 frames"""
    F, kind = event_slot(np.arange(n), skip)
    st["n_balls"] = 1
    for name in ("ball_x", "ball_y", "ball_vx", "ball_vy"):
        st[name][:] = 0.0
    st["ball_x"][:, 0], st["ball_vy"][:, 0] = 30.0, 1.0
    st["ball_y"][:, 0] = 162.5 - (F + 1)
    st["ball_radius"] = 2.0
    st["is_dead"] = st["reset"] = 0
    st["lives"] = 1 + kind
    return st


def build_space_invaders_event(st, n, skip):
    """the ship explodes: the life goes when ship_death_counter, F + 1, has run out (oracle/orc_si.c, phase B)"""
    F, kind = event_slot(np.arange(n), skip)
    st["life_display_timer"] = 0
    st["ship_alive"], st["ship_death_hit_1"] = 0, 1
    st["ship_death_counter"] = F + 1
    st["lives"] = 1 + kind
    return st


def build_amidar_event(st, n, skip, perimeter_from_start=False):
    """every enemy parked on the player and all of them at speed 0, the player in the air for F + 1 more frames with no jump left (FIRE
    is FireResetEnv's first action): the life goes in the frame the jump ends"""
    from support import amidar_edit_last_lives
    from toybox_amd import _abi
    from toybox_amd.games import codec
    cd = codec("amidar")
    F, kind = event_slot(np.arange(n), skip)
    out = st.copy()
    for i in range(n):
        rec = _abi.AmidarState.from_buffer_copy(st[i].tobytes())
        js = amidar_edit_last_lives(cd.state_to_json(rec), lives=int(1 + kind[i]), jump_timer=int(F[i] + 1), perimeter_from_start=perimeter_from_start)
        js["jumps"] = 0
        for mover in [js["player"]] + js["enemies"]:               # nobody walks off: UP is FireResetEnv's second action
            mover["speed"] = 0
        out[i] = np.frombuffer(bytes(cd.state_from_json(js)), dtype=st.dtype)[0]
    return out


def build_gridworld_event(st, n, skip):
    """a corridor along row 3 of a 32 x 7 board, the player at its left end, the goal F + 1 cells to the right: RIGHT repeated reaches it
    in raw frame F.  GridWorld has one life: the kind is always game over."""
    F, _ = event_slot(np.arange(n), skip)
    st["width"], st["height"] = 32, 7
    st["score"] = st["game_over"] = 0
    st["player_x"], st["player_y"] = 1, 3
    grid = np.ones((n, 32, 32), np.uint8)                      # tile 1: a wall
    grid[:, 3, 1:31] = 0                                       # tile 0: floor
    grid[np.arange(n), 3, 2 + F] = 2                           # tile 2: the goal
    st["grid"] = grid.reshape(n, -1)
    return st


BUILDERS = {"breakout": build_breakout_event, "space_invaders": build_space_invaders_event, "amidar": build_amidar_event,
            "gridworld": build_gridworld_event}


def one_life_config(game, lib):
    """the game's default config with start_lives = 1"""
    from toybox_amd import Engine
    with Engine(game, 1, lib=lib) as e:
        cfg = e.get_config()
    cfg.start_lives = 1
    return cfg


def noop_end_frames(game, n, seed, config, lib, limit=4000):
    """int[n]: how many no-op frames env i's new game lasts under this engine seed and config, from a raw replay (a game that never
    ends: limit)"""
    from toybox_amd import Engine
    with Engine(game, n, config=config, lib=lib) as e:
        e.seed(seed)
        e.new_game()
        end = np.full(n, limit, np.int64)
        noop = np.zeros(n, np.int32)
        for t in range(limit):
            done = e.step(noop)[1]
            end = np.where(done & (end == limit), t + 1, end)
            if (end < limit).all():
                break
    return end


def build_noop_game_over(game, n, seed, lib):
    """(config, counts): one life per game, and no-op counts from 3 below the frame at which env i's new game ends to 3 above it, env i
    at offset i % 7 - 3.  SpaceInvaders and Amidar only: a Breakout game without FIRE has no ball, a GridWorld game without a move no goal."""
    config = one_life_config(game, lib)
    end = noop_end_frames(game, n, seed, config, lib)
    assert (end < 4000).all(), (game, end.max())             # (most SpaceInvaders games end at frame 475, a few after 2 000)
    return config, (end + np.arange(n) % 7 - 3).astype(np.int32)
