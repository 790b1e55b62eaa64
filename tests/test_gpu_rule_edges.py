"""One hand-built case per game-rule branch that the shared step-parity inputs (tests/rule_inputs.py) leave untaken or take through
one device form only, in all four games; tests/test_rule_reach.py is the ratchet that says what is left.

A case writes a state into every env through set_states on both libraries, varying one parameter across the envs (which brick, which
column, which value), and plays FRAMES = 4 frames of the synthetic action rule.  Every device form that carries its own copy of the
rule plays it and must equal the oracle bit for bit:

    batch1 / batch2   tbx_step under TBX_OPT_STEP_FORM 1 (thread per env) and 2 (wave per env) in Breakout and Amidar; SpaceInvaders and
                      GridWorld have one form, batch.  A Breakout engine whose wall has been written steps through its brick-table
                      kernel under either option, so a case that writes bricks (canonical = False) runs batch2 alone.  Reward, done,
                      lives, score of every frame, the raw state bytes of every env after every frame, the frame in every format before the first step and
                      the RGB frame after the last
    synthetic         tbx_step_synthetic with the same action rule: the packed word and the raw state bytes after every frame
    rollout           one tbx_rollout_synthetic chunk of 4: its frames, its packed words, the state bytes behind it
    agent             one fused agent step (skip 4, 84 x 84 x 4, no reset-time wrapper, so that written states are not refused), the
                      frame-0 action held: observation, reward, done, the state bytes behind it
    lookahead         TBX_QUERY_LOOKAHEAD_PLAN over the same four actions, no reset: the five rows (against the plan replayed on a second
                      oracle engine with the same config, states and RNGs, tests/search_replay.py); the engine's states untouched

A case may also change the config (Case.config): every engine of the case then gets that config before its new game.

at 65 and 257 envs (a partial wavefront; a partial block and more than one).  The oracle's side of every case is computed once per
(case, envs) and shared (expected()).

The tests without the gpu mark are the twins: each asserts on the oracle's own before and after states that the case's branch was in
fact taken (the predicate restated in Python), so a case that has gone dull fails where no GPU is, whatever the device does; and that
the oracle's own forms agree with each other."""
import functools

import numpy as np
import pytest

from fork_replay import sim_rngs, states_bytes
from search_replay import plan_columns, play_plan
from support import engine_is_oracle, read_buffer, synthetic_actions
from toybox_amd import Engine, _abi
from toybox_amd.engine import plan_code

FRAMES, ENGINE_SEED, ACTION_SEED = 4, 5, 4242
SIZES = [65, 257]
FORMS = {"breakout": ["batch1", "batch2", "synthetic", "rollout", "agent", "lookahead"],
         "space_invaders": ["batch", "synthetic", "rollout", "agent", "lookahead"],
         "amidar": ["batch1", "batch2", "synthetic", "rollout", "agent", "lookahead"],
         "gridworld": ["batch", "synthetic", "rollout", "agent", "lookahead"]}
AGENT = dict(skip=4, out_h=84, out_w=84, stack=4, clip_reward=False, episodic_life=False, fire_reset=False, noop_max=0)

# Breakout's geometry (SPEC.md): the field, the canonical wall of 18 x 6 bricks of 12 x 4, index col * 6 + row, depth 5 - row
BRK_LEFT, BRK_RIGHT, BRK_TOP, BRK_BOTTOM, BRK_ROWS, BRK_WALL = 12.0, 228.0, 25.0, 160.0, 6, 108
EXTREMES = np.array([1e6 - 1, 1e6, 1e6 + 1, -1e6 + 1, -1e6, -1e6 - 1, 1e300, -1e300, np.inf, -np.inf])


# ================================================================ the cases: build(records, n) -> records; taken(start, after, outs)

def _launch_one_ball(st, x, y, vx, vy):
    """every env: one launched ball"""
    st["n_balls"] = 1
    for name, v in (("ball_x", x), ("ball_y", y), ("ball_vx", vx), ("ball_vy", vy)):
        st[name][:] = 0.0
        st[name][:, 0] = v
    st["is_dead"] = st["reset"] = 0


def _clear_below(st, env, j):
    """kill the bricks of brick j's column that hang below it, so that a ball from below reaches it first"""
    col, row = j // BRK_ROWS, j % BRK_ROWS
    st["bricks"]["alive"][env, col * BRK_ROWS + row + 1:(col + 1) * BRK_ROWS] = 0


def _under(st, j):
    """(x, y) 2.5 below the middle of the lower edge of brick j[i] in env i"""
    B, ar = st["bricks"], np.arange(len(st))
    return B["x"][ar, j] + 6.0, B["y"][ar, j] + B["h"][ar, j] + 2.5


def _speed(st, b=0):
    return np.sqrt(st["ball_vx"][:, b] ** 2 + st["ball_vy"][:, b] ** 2)


def build_radius_nonpositive(st, n):
    """radius 0 (even envs) and -1 (odd) with a launched ball: the frame is one slice, and the overlap test still hits bricks.  The ball
    flies up into the lowest brick of column env % 18 at 3 units per frame."""
    i = np.arange(n)
    j = (i % 18) * BRK_ROWS + BRK_ROWS - 1
    x, y = _under(st, j)
    _launch_one_ball(st, x, y - 1.0, 0.5 * (i % 5 - 2), -3.0)
    st["ball_radius"] = np.where(i % 2 == 0, 0.0, -1.0)
    return st


def taken_radius_nonpositive(start, after, outs):
    assert (start["ball_radius"] <= 0.0).all() and (start["is_dead"] == 0).all()
    assert (start["ball_radius"] == 0.0).any() and (start["ball_radius"] < 0.0).any()
    # one slice: the first frame moves the ball by exactly its velocity, at 3 units per frame (a radius of 2 would cut it in two)
    assert np.array_equal(after[0]["ball_x"][:, 0], start["ball_x"][:, 0] + start["ball_vx"][:, 0])
    assert np.array_equal(after[0]["ball_y"][:, 0], start["ball_y"][:, 0] + start["ball_vy"][:, 0])
    assert (after[-1]["score"] > start["score"]).all(), "a ball without a box must still hit the brick it is in"


def build_indestructible_hit(st, n):
    """brick (7 env + 3) % 108 is indestructible and first in the way of a ball from below"""
    i = np.arange(n)
    j = (7 * i + 3) % BRK_WALL
    for env in range(n):
        _clear_below(st, env, int(j[env]))
    st["bricks"]["destructible"][i, j] = 0
    x, y = _under(st, j)
    _launch_one_ball(st, x, y, 0.25, -2.0)
    return st


def taken_indestructible_hit(start, after, outs):
    i = np.arange(len(start))
    j = (7 * i + 3) % BRK_WALL
    assert (start["bricks"]["destructible"][i, j] == 0).all()
    assert (after[0]["ball_vy"][:, 0] > 0.0).all(), "the ball bounced off it in the first frame"
    for a in after:
        assert np.array_equal(a["score"], start["score"]) and (a["bricks"]["alive"][i, j] == 1).all()


def build_speed_rows(st, n):
    """a brick of a speed-up row (rows 0..2, depth >= 3) hit by a ball at exactly ball_speed_fast = 4 (env % 3 == 0), at 6 (1) and by
    a ball at rest inside it (2): none is rescaled.  Column (env // 3) % 18, row (env // 9) % 3."""
    i = np.arange(n)
    j = ((i // 3) % 18) * BRK_ROWS + (i // 9) % 3
    for env in range(n):
        _clear_below(st, env, int(j[env]))
    x, y = _under(st, j)
    rest = i % 3 == 2
    B = st["bricks"]
    _launch_one_ball(st, x, np.where(rest, B["y"][i, j] + 2.0, y), 0.0, np.where(rest, 0.0, np.where(i % 3 == 0, -4.0, -6.0)))
    return st


def taken_speed_rows(start, after, outs):
    i = np.arange(len(start))
    j = ((i // 3) % 18) * BRK_ROWS + (i // 9) % 3
    B = start["bricks"]
    assert (B["depth"][i, j] >= 3).all()
    v0 = _speed(start)
    assert (v0[i % 3 == 0] == 4.0).all() and (v0[i % 3 == 1] == 6.0).all() and (v0[i % 3 == 2] == 0.0).all()
    assert np.array_equal(after[0]["score"], start["score"] + B["points"][i, j]), "the brick was hit in the first frame"
    assert (after[0]["bricks"]["alive"][i, j] == 0).all()
    assert np.array_equal(_speed(after[0]), v0), "no ball at or above ball_speed_fast, and none at rest, is rescaled"
    assert (after[0]["ball_vy"][i % 3 < 2, 0] > 0.0).all()


def build_wall_returns(st, n):
    """the last destructible brick, (7 env + 3) % 108, with a ball under it, in a wall that also holds indestructible bricks -- every
    fifth brick outside the ball's column, every second of them dead: the wall that comes back leaves those as they are"""
    i = np.arange(n)
    j = (7 * i + 3) % BRK_WALL
    B = st["bricks"]
    for env in range(n):
        k = np.arange(BRK_WALL)
        hard = (k % 5 == env % 5) & (k // BRK_ROWS != j[env] // BRK_ROWS)
        B["destructible"][env, :BRK_WALL] = ~hard
        B["alive"][env, :BRK_WALL] = np.where(hard, (k // 5) % 2 == 0, k == j[env])
    x, y = _under(st, j)
    _launch_one_ball(st, x, y, 0.25, -2.0)
    return st


def taken_wall_returns(start, after, outs):
    B0, B1 = start["bricks"], after[-1]["bricks"]
    hard = B0["destructible"][:, :BRK_WALL] == 0
    assert hard.any(axis=1).all() and (hard & (B0["alive"][:, :BRK_WALL] == 0)).any(axis=1).all()
    assert np.array_equal(after[-1]["level"], start["level"] + 1)
    assert np.array_equal(B1["alive"][:, :BRK_WALL][hard], B0["alive"][:, :BRK_WALL][hard]), "indestructible bricks keep their bit"
    # the wall is back whole, but for what the ball has eaten since: it has had at most three frames
    assert ((B1["alive"][:, :BRK_WALL] == 0) & ~hard).sum(axis=1).max() <= 3


def _pick(i, mul, add):
    return EXTREMES[(i * mul + add) % len(EXTREMES)]


def build_paint_extremes(st, n, bricks=False):
    """paddle and ball rectangles at +-1e6 +- 1, +-1e300 and +-inf (the picture clamps every coordinate and size to +-1e6 before it
    converts; an undefined conversion otherwise).  Two launched balls; every env another combination."""
    i = np.arange(n)
    st["paddle_x"], st["paddle_width"] = _pick(i, 1, 0), _pick(i, 3, 1)
    st["paddle_x"][i % 11 == 0] = st["paddle_width"][i % 11 == 0] = np.inf          # inf - inf: the left edge is not a number
    st["paddle_y"] = np.where(i % 7 == 0, _pick(i // 7, 1, 2), st["paddle_y"])
    st["paddle_speed"] = 4.0
    # ball 0 beyond +1e6 in x, ball 1 at or beyond -1e6 in y: every env's picture meets both clamps, whatever the radius
    _launch_one_ball(st, np.array([1e6 + 3, 1e300, np.inf])[i % 3], 100.0, 0.5, 1.0)
    st["n_balls"] = 2
    st["ball_x"][:, 1], st["ball_vx"][:, 1], st["ball_vy"][:, 1] = 100.0, -0.75, -1.0
    st["ball_y"][:, 1] = np.array([-1e6, -1e6 - 1, -1e300, -np.inf])[(i // 3) % 4]
    st["ball_radius"] = np.where(i % 3 == 0, _pick(i // 3, 1, 0), 2.0)
    if bricks:
        B = st["bricks"]
        B["x"][:, 0], B["w"][:, 0] = _pick(i, 1, 3), _pick(i, 3, 4)
        B["y"][:, 1], B["h"][:, 1] = _pick(i, 1, 6), _pick(i, 7, 0)
        B["x"][:, 2], B["w"][:, 2] = -1e6 - 1, 1e6 + 40 + i % 50            # clamped on both sides: ends at x = 0, nothing to see
        B["x"][:, 3], B["w"][:, 3], B["y"][:, 3], B["h"][:, 3] = -1e6, 1e6 + 20 + i % 50, -1e6 + 1, 1e6 + 40     # ... and one that shows
    return st


def _paint_arguments(st, bricks):
    """[n, k]: every value the picture converts for env i (orc_breakout_render)"""
    r = st["ball_radius"][:, None]
    with np.errstate(invalid="ignore"):
        cols = [st["paddle_x"] - st["paddle_width"] * 0.5, st["paddle_y"], st["paddle_width"]]
        cols += list((st["ball_x"][:, :2] - r).T) + list((st["ball_y"][:, :2] - r).T) + [r[:, 0] * 2.0]
        if bricks:
            cols += [st["bricks"][f][:, k] for f in "xywh" for k in range(4)]
    return np.stack(cols, axis=1)


def taken_paint_extremes(start, after, outs, bricks=False):
    with np.errstate(invalid="ignore"):
        v = _paint_arguments(start, bricks)
        assert (v > 1e6).any(axis=1).all() and (~(v > -1e6)).any(axis=1).all(), "both clamps work in every env's first picture"
        v = _paint_arguments(after[-1], bricks)           # (a ball with radius -inf has left the field by now: not every env)
        assert (v > 1e6).any(axis=1).mean() > 0.5 and (~(v > -1e6)).any(axis=1).mean() > 0.5, "... and in most envs' last one"
        v = _paint_arguments(start, bricks)
        assert np.isinf(v).any() and np.isnan(v).any() and (np.abs(v) == 1e300).any() and (v == 1e6 + 1).any() and (v == -1e6 - 1).any()


def build_paddle_zero_width(st, n):
    """paddle_width 0 and a ball that comes down exactly onto paddle_x: (x - left) / width is 0 / 0, which SPEC.md defines as 0, the
    first segment.  Another paddle_x, with and without a fraction, and another speed in every env; the paddle stands still."""
    i = np.arange(n)
    st["paddle_width"], st["paddle_speed"] = 0.0, 0.0
    st["paddle_x"] = 20.0 + i % 200 + 0.5 * (i % 2)
    _launch_one_ball(st, st["paddle_x"], st["paddle_y"] - 3.0, 0.0, 1.0 + 0.25 * (i % 4))
    return st


def taken_paddle_zero_width(start, after, outs):
    from toybox_amd.games import breakout as brk
    cfg = brk.default_config()
    assert (start["paddle_width"] == 0.0).all() and np.array_equal(start["ball_x"][:, 0], start["paddle_x"])
    assert (start["ball_vy"][:, 0] > 0.0).all()
    sp = start["ball_vy"][:, 0]
    assert np.array_equal(after[0]["ball_vx"][:, 0], sp * cfg.paddle_dir_x[0]), "re-aimed along the FIRST segment in the first frame"
    assert np.array_equal(after[0]["ball_vy"][:, 0], sp * cfg.paddle_dir_y[0])
    assert np.array_equal(after[0]["paddle_x"], start["paddle_x"])


# ---------------------------------------------------------------- SpaceInvaders (320 x 210, ground at y = 195, ship at y = 185, shields at y = 157)

SI_W, SI_GROUND_Y, SI_SHOT_DELAY, SI_MAX_LASERS = 320, 195, 50, 8
DIR_UP, DIR_DOWN, DIR_LEFT, DIR_RIGHT = 0, 1, 2, 3


def _si_ready(st):
    """every env past its get-ready phase with a live ship, no laser in flight, no march and no enemy shot within the four frames"""
    st["life_display_timer"], st["ship_alive"], st["ship_death_counter"], st["ship_death_hit_1"] = 0, 1, -1, 1
    st["n_enemy_lasers"], st["has_ship_laser"] = 0, 0
    st["enemy_lasers"] = np.zeros_like(st["enemy_lasers"])
    st["ship_laser"] = np.zeros_like(st["ship_laser"])
    st["enemy_shot_delay"], st["move_counter"] = 40, 20


def _laser(L, rows, x, y, movement, speed, w=2, h=8):
    for name, v in (("x", x), ("y", y), ("w", w), ("h", h), ("t", 0), ("movement", movement), ("speed", speed)):
        L[name][rows] = v
    L["color"]["r"][rows], L["color"]["g"][rows], L["color"]["b"][rows], L["color"]["a"][rows] = 255, 200, 40, 255


def build_si_sideways_lasers(st, n):
    """eight enemy lasers flying LEFT (even slots) and RIGHT (odd): slots 0..5 start 0..8 px from the side they leave by, at 1..3 px per
    frame, slots 6 and 7 in mid-field; the ship's laser flies LEFT (even envs) or RIGHT off its side.  All above the shields."""
    _si_ready(st)
    i = np.arange(n)
    st["n_enemy_lasers"] = SI_MAX_LASERS
    for k in range(SI_MAX_LASERS):
        left = k % 2 == 0
        edge = (i % 7 + k - 1) if left else (SI_W - 1 - i % 7 - k)
        x = edge if k < 6 else (100 + i % 60 if left else 220 - i % 60)
        _laser(st["enemy_lasers"], (i, k), x, 40 + 9 * k, DIR_LEFT if left else DIR_RIGHT, 1 + (i + k) % 3)
    st["has_ship_laser"] = 1
    _laser(st["ship_laser"], i, np.where(i % 2 == 0, i % 5, SI_W - 2 - i % 5), 20, np.where(i % 2 == 0, DIR_LEFT, DIR_RIGHT), 2 + i % 2)
    return st


def taken_si_sideways_lasers(start, after, outs):
    i = np.arange(len(start))
    L0 = start["enemy_lasers"]
    assert np.isin(L0["movement"], (DIR_LEFT, DIR_RIGHT)).all() and np.isin(start["ship_laser"]["movement"], (DIR_LEFT, DIR_RIGHT)).all()
    assert (after[-1]["n_enemy_lasers"] < SI_MAX_LASERS).all() and (after[-1]["n_enemy_lasers"] >= 2).all(), "some left by their side, two fly on"
    gone = {DIR_LEFT: 0, DIR_RIGHT: 0}
    for k in range(SI_MAX_LASERS):                              # a laser keeps its y: that is how it is found again behind the compaction
        L1 = after[0]["enemy_lasers"]
        here = (L1["y"] == 40 + 9 * k) & (np.arange(SI_MAX_LASERS)[None, :] < after[0]["n_enemy_lasers"][:, None])
        sign = -1 if k % 2 == 0 else 1
        x1 = L0["x"][:, k] + sign * L0["speed"][:, k]
        left_field = (x1 + 2 <= 0) | (x1 >= SI_W)
        assert np.array_equal(here.any(axis=1), ~left_field), k
        rows = np.flatnonzero(here.any(axis=1))
        assert np.array_equal(L1["x"][rows, here[rows].argmax(axis=1)], x1[rows]), "it moved sideways by its speed"
        gone[DIR_LEFT if k % 2 == 0 else DIR_RIGHT] += int(left_field.sum())
    assert gone[DIR_LEFT] > 0 and gone[DIR_RIGHT] > 0
    # the ship's laser leaves within the four frames (FIRE may have put a new one, flying UP, in its place)
    S = after[-1]["ship_laser"]
    assert ((after[-1]["has_ship_laser"] == 0) | (S["movement"] == DIR_UP)).all()
    assert (after[0]["has_ship_laser"] == 1).any() and np.array_equal(after[-1]["score"], start["score"])


def build_si_ship_laser_at_ground(st, n):
    """the ship's laser arrives at or below the ground line: flying UP from y = 201 + env % 9 (even envs), DOWN from 188 + env % 7 (odd)"""
    _si_ready(st)
    i = np.arange(n)
    st["has_ship_laser"] = 1
    up = i % 2 == 0
    _laser(st["ship_laser"], i, 40 + i % 240, np.where(up, 201 + i % 9, 188 + i % 7), np.where(up, DIR_UP, DIR_DOWN), np.where(up, 6, 7))
    return st


def taken_si_ship_laser_at_ground(start, after, outs):
    S = start["ship_laser"]
    y1 = np.where(S["movement"] == DIR_UP, S["y"] - S["speed"], S["y"] + S["speed"])
    assert (y1 >= SI_GROUND_Y).all() and (y1 + S["h"] > 0).all() and (S["x"] + S["w"] > 0).all() and (S["x"] < SI_W).all()
    assert (y1 == SI_GROUND_Y).any() and (y1 > SI_GROUND_Y).any() and (S["movement"] == DIR_UP).any() and (S["movement"] == DIR_DOWN).any()
    assert (after[0]["has_ship_laser"] == 0).all() and not np.frombuffer(np.ascontiguousarray(after[0]["ship_laser"]).tobytes(), np.uint8).any(), "gone and zeroed in the first frame"
    assert np.array_equal(after[0]["score"], start["score"])


def build_si_full_laser_table(st, n):
    """the enemies' shot comes due (in 1..3 frames) with all eight lasers in flight: no shot, and no draw from the RNG.  The lasers fall
    slowly along the left edge, clear of shields and ship."""
    _si_ready(st)
    i = np.arange(n)
    st["n_enemy_lasers"] = SI_MAX_LASERS
    for k in range(SI_MAX_LASERS):
        _laser(st["enemy_lasers"], (i, k), 2 + 3 * k + i % 3, 30 + 5 * k + i % 11, DIR_DOWN, 1)
    st["enemy_shot_delay"] = 1 + i % 3
    return st


def taken_si_full_laser_table(start, after, outs):
    shot_frame = start["enemy_shot_delay"] - 1
    assert (shot_frame < FRAMES).all() and len(np.unique(shot_frame)) == 3
    for t, a in enumerate(after):
        assert (a["n_enemy_lasers"] == SI_MAX_LASERS).all(), "the table stays full through the shot frame"
        assert np.array_equal(a["rand"], start["rand"]), "a refused shot draws nothing"
        assert np.array_equal(a["enemy_shot_delay"], np.where(t >= shot_frame, SI_SHOT_DELAY - (t - shot_frame), start["enemy_shot_delay"] - t - 1))
    assert (start["enemies"]["alive"] == 1).any(axis=1).all()


def build_si_empty_formation(st, n):
    """even envs: no enemy at all (n_enemies 0) -- a march over nobody (in the first frame where env % 4 == 0) and a wave cleared every
    frame; odd envs: 36 enemies, all dead and done exploding -- the shot comes due in the first frame with no column alive, then the
    formation is back"""
    _si_ready(st)
    i = np.arange(n)
    even = i % 2 == 0
    st["n_enemies"] = np.where(even, 0, st["n_enemies"])
    st["enemies"]["alive"] = 0
    st["enemies"]["death_counter"] = -1
    st["move_counter"] = np.where(i % 4 == 0, 1, 9)
    st["enemy_shot_delay"] = np.where(i % 4 == 2, 30, 1)
    st["level"] = 1 + i % 5
    return st


def taken_si_empty_formation(start, after, outs):
    i = np.arange(len(start))
    even = i % 2 == 0
    assert (start["n_enemies"][even] == 0).all() and (start["n_enemies"][~even] == 36).all() and not start["enemies"]["alive"].any()
    assert np.array_equal(after[-1]["level"][even], start["level"][even] + FRAMES), "an empty formation is cleared every frame"
    assert np.array_equal(after[-1]["level"][~even], start["level"][~even] + 1) and (after[0]["enemies"]["alive"][~even, :36] == 1).all()
    assert np.array_equal(after[0]["rand"], start["rand"]), "no column alive: the shot that came due drew nothing"
    assert (after[0]["enemy_shot_delay"][i % 4 != 2] == SI_SHOT_DELAY).all() and (after[0]["n_enemy_lasers"] == 0).all()
    assert (after[-1]["n_enemies"][even] == 0).all()


def build_si_dead_ship_idle(st, n):
    """a ship that is neither alive nor exploding, no get-ready timer running: the world stands still.  Ship position, lasers in flight
    and the counters differ across envs."""
    _si_ready(st)
    i = np.arange(n)
    st["ship_alive"] = 0
    st["ship_x"] = 40 + i % 200
    st["n_enemy_lasers"] = i % (SI_MAX_LASERS + 1)
    for k in range(SI_MAX_LASERS):
        rows = np.flatnonzero(k < st["n_enemy_lasers"])
        _laser(st["enemy_lasers"], (rows, k), 30 + 30 * k + rows % 17, 60 + 11 * k, DIR_DOWN, 3)
    st["has_ship_laser"] = i % 2
    rows = np.flatnonzero(i % 2 == 1)
    _laser(st["ship_laser"], rows, 50 + rows % 200, 120, DIR_UP, 6)
    st["move_counter"], st["enemy_shot_delay"] = 1 + i % 3, 1 + i % 2
    return st


def taken_si_dead_ship_idle(start, after, outs):
    assert (start["ship_alive"] == 0).all() and (start["ship_death_counter"] < 0).all() and (start["life_display_timer"] == 0).all()
    assert (start["n_enemy_lasers"] > 0).any() and (start["has_ship_laser"] == 1).any()
    for a in after:
        assert a.tobytes() == start.tobytes(), "nothing moves, counts down or fires"


def build_si_ufo_removed(st, n):
    """ufo_appearance_counter below zero (-1, -2, -3): a mothership taken out of the game neither counts down nor flies, wherever it is"""
    _si_ready(st)
    i = np.arange(n)
    st["ufo_appearance_counter"] = -1 - i % 3
    st["ufo_death_counter"] = -1
    st["ufo_x"] = -20 + i
    return st


def taken_si_ufo_removed(start, after, outs):
    assert (start["ufo_appearance_counter"] < 0).all() and (start["ufo_death_counter"] == -1).all()
    for a in after:
        assert np.array_equal(a["ufo_x"], start["ufo_x"]) and np.array_equal(a["ufo_appearance_counter"], start["ufo_appearance_counter"])
    assert np.array_equal(after[-1]["move_counter"], start["move_counter"] - FRAMES), "the rest of the world runs"


# ---------------------------------------------------------------- Amidar (SPEC.md "Amidar": a 32 x 31 board of tiles of 64 x 80 world units, speed 8)

AMI_WX, AMI_WY, AMI_BW, AMI_BH, AMI_N_ROUTES = _abi.AMI_TILE_WX, _abi.AMI_TILE_WY, 32, 31, 5
AMI_OX, AMI_OY, AMI_SCALE = 16, 37, 16                       # the board's origin in the picture, world units per pixel
AI_LOOKUP, AI_PERIMETER, AI_AMIDAR, AI_TARGET, AI_RANDOM = 1, 2, 3, 4, 5
NONE = -1                                                    # "no direction": the enemy stands
AMI_DELTA = {DIR_UP: (0, -1), DIR_DOWN: (0, 1), DIR_LEFT: (-1, 0), DIR_RIGHT: (1, 0), NONE: (0, 0)}
TILE_EMPTY, TILE_UNPAINTED, TILE_PAINTED, TILE_CHASE = 0, 1, 2, 3


def _ami_place(M, rows, k, tx, ty):
    """enemy k (or, k None, the player) of envs `rows` on the corner of tile (tx, ty), standing, with no past"""
    at = rows if k is None else (rows, k)
    M["x"][at], M["y"][at] = AMI_WX * np.asarray(tx), AMI_WY * np.asarray(ty)
    M["step_tx"][at] = M["step_ty"][at] = -1
    M["n_history"][at] = 0
    M["history"][at] = 0
    M["caught"][at] = 0


def _ami_moved(start, after0, k):
    """(dx, dy) of enemy k in the first frame"""
    return after0["enemies"]["x"][:, k] - start["enemies"]["x"][:, k], after0["enemies"]["y"][:, k] - start["enemies"]["y"][:, k]


def _ami_assert_dirs(start, after0, k, want, what):
    dx, dy = _ami_moved(start, after0, k)
    sp = start["enemies"]["speed"][:, k]
    wx, wy = (np.array([AMI_DELTA[int(d)][c] for d in want]) for c in (0, 1))
    bad = np.flatnonzero((dx != sp * wx) | (dy != sp * wy))
    assert not len(bad), "%s: envs %s moved by %s, expected directions %s" % (what, bad[:8], list(zip(dx[bad[:8]], dy[bad[:8]])), want[bad[:8]])


def build_amidar_lookup_tables(st, n):
    """EnemyLookupAI records beside their tables: enemy 0 with route index 99, -1, 5 or -7 (no such table: it idles), enemy 1 with
    ai.next 99, -1, 5, 1000 or -99 (taken as 0), enemies 2 (route 99) and 3 caught somewhere on rows 12 and 6 with the chase running
    out in 1..3 frames: both are put back on their route's first tile -- tile 0 for the table that does not exist"""
    i = np.arange(n)
    E = st["enemies"]
    A = E["ai"]
    A["default_route_index"][:, 0] = np.array([99, -1, AMI_N_ROUTES, -7])[i % 4]
    A["next"][:, 1] = np.array([99, -1, 5, 1000, -99])[i % 5]
    _ami_place(E, i, 2, i % 32, 12)
    _ami_place(E, i, 3, (5 * i) % 32, 6)
    A["default_route_index"][:, 2] = 99
    E["caught"][:, 2:4] = 1
    st["chase_timer"] = 1 + i % 3
    st["score"] = 10 * i
    return st


def taken_amidar_lookup_tables(start, after, outs):
    E0 = start["enemies"]
    r0, nx = E0["ai"]["default_route_index"][:, 0], E0["ai"]["next"][:, 1]
    assert ((r0 < 0) | (r0 >= AMI_N_ROUTES)).all() and (r0 == 99).any() and (r0 < 0).any()
    assert ((nx < 0) | (nx >= 5)).all() and (nx == 99).any() and (nx < 0).any()
    for a in after:
        E = a["enemies"]
        assert np.array_equal(E["x"][:, 0], E0["x"][:, 0]) and np.array_equal(E["y"][:, 0], E0["y"][:, 0]) and (E["step_tx"][:, 0] == -1).all()
    E = after[0]["enemies"]
    assert ((E["ai"]["next"][:, 1] >= 0) & (E["ai"]["next"][:, 1] < 5)).all() and (E["step_tx"][:, 1] >= 0).all(), "next was taken as 0: the enemy walks"
    F = np.arange(FRAMES)[:, None]
    caught = np.stack([a["enemies"]["caught"][:, 2:4] for a in after])                     # [frame, env, 2]
    assert np.array_equal(caught.all(axis=2), F < (start["chase_timer"] - 1)[None, :]), "both come back in the frame the chase ends"
    E = after[-1]["enemies"]
    assert (E["x"][:, 2] == 0).all() and (E["y"][:, 2] == 0).all(), "no such route: back on tile 0, and idle there"
    assert (np.abs(E["x"][:, 3]) + np.abs(E["y"][:, 3] - 2000) <= 8 * FRAMES).all(), "route 3 starts at world (0, 2000)"


def build_amidar_odd_movers(st, n):
    """enemy 0 with speed -3..-5 (it decides and stands), enemy 1 with ai.kind 7, 6, -1, 0 or 100 (no such protocol: it idles), enemy 2
    at (64 tx + 5.., 80 * 6) and enemy 3 at (64 tx, 80 * 12 + 7..) without a step (off their corner: they stand), enemy 4 one to five
    units above or below its target tile on column 0 at speed 6 or 7 (it lands on the tile, not beyond); the player off its corner
    (odd envs) or 3..6 units below its target at speed 7 (even)"""
    i = np.arange(n)
    E, P = st["enemies"], st["player"]
    E["speed"][:, 0] = -3 - i % 3
    E["ai"]["kind"][:, 1] = np.array([7, 6, -1, 0, 100])[i % 5]
    _ami_place(E, i, 2, 0, 6)
    E["x"][:, 2] = AMI_WX * (i % 32) + 5 + i % 50
    _ami_place(E, i, 3, 31 - i % 32, 12)
    E["y"][:, 3] += 7 + i % 60
    ty, down = 5 + i % 20, (i // 2) % 2 == 0
    _ami_place(E, i, 4, 0, ty)
    E["y"][:, 4] += np.where(down, -1, 1) * (1 + i % 5)
    E["step_tx"][:, 4], E["step_ty"][:, 4], E["speed"][:, 4] = 0, ty, 6 + i % 2
    even = i % 2 == 0
    _ami_place(P, i, None, 31, 15)
    P["x"] += np.where(even, 0, 5 + i % 40)
    P["y"] += np.where(even, 3 + i % 4, 0)
    P["step_tx"], P["step_ty"], P["speed"] = np.where(even, 31, -1), np.where(even, 15, -1), np.where(even, 7, 8)
    return st


def taken_amidar_odd_movers(start, after, outs):
    i = np.arange(len(start))
    E0, P0 = start["enemies"], start["player"]
    assert (E0["speed"][:, 0] < 0).all() and not np.isin(E0["ai"]["kind"][:, 1], [1, 2, 3, 4, 5]).any()
    assert (E0["x"][:, 2] % AMI_WX != 0).all() and (E0["x"][:, 3] % AMI_WX == 0).all() and (E0["y"][:, 3] % AMI_WY != 0).all()
    for a in after:
        E = a["enemies"]
        for k in range(4):
            assert np.array_equal(E["x"][:, k], E0["x"][:, k]) and np.array_equal(E["y"][:, k], E0["y"][:, k]), k
        assert (E["step_tx"][:, 1:4] == -1).all()
        assert np.array_equal(a["player"]["x"][i % 2 == 1], P0["x"][i % 2 == 1]) and np.array_equal(a["player"]["y"][i % 2 == 1], P0["y"][i % 2 == 1])
    assert (after[0]["enemies"]["step_tx"][:, 0] >= 0).all(), "a mover of negative speed decides, and then stands"
    gap = np.abs(E0["y"][:, 4] - AMI_WY * E0["step_ty"][:, 4])
    assert ((gap > 0) & (gap < E0["speed"][:, 4])).all() and (E0["y"][:, 4] < AMI_WY * E0["step_ty"][:, 4]).any() and (E0["y"][:, 4] > AMI_WY * E0["step_ty"][:, 4]).any()
    assert np.array_equal(after[0]["enemies"]["y"][:, 4], AMI_WY * E0["step_ty"][:, 4]) and (after[0]["enemies"]["x"][:, 4] == 0).all()
    even = i % 2 == 0
    assert (after[0]["player"]["y"][even] == AMI_WY * 15).all() and (P0["y"][even] - AMI_WY * 15 < 7).all()


def build_amidar_negative_world(st, n):
    """movers left of and above world 0 (the picture's board starts at pixel (16, 37), so they are in sight, and the pixel is the
    floor of world / 16, not the truncation): enemy 0 left, enemy 1 above, enemy 2 both, none on a corner; enemy 3 on the corner of
    a tile left of the board, tx -1..-3; every third env's player far out to the upper left"""
    i = np.arange(n)
    E, P = st["enemies"], st["player"]
    _ami_place(E, i, 0, 0, i % 31)
    E["x"][:, 0] = -16 * (1 + i % 9) - 5
    _ami_place(E, i, 1, i % 32, 0)
    E["y"][:, 1] = -16 * (1 + i % 7) - 3
    _ami_place(E, i, 2, 0, 0)
    E["x"][:, 2], E["y"][:, 2] = -1 - i % 33, -1 - i % 41
    _ami_place(E, i, 3, -1 - i % 3, 0)
    rows = np.flatnonzero(i % 3 == 0)
    _ami_place(P, rows, None, 0, 0)
    P["x"][rows], P["y"][rows] = -(200 + rows % 50), -(100 + rows % 70)
    return st


def taken_amidar_negative_world(start, after, outs, frame3=None):
    i = np.arange(len(start))
    E0 = start["enemies"]
    assert (E0["x"][:, 0] < 0).all() and (E0["y"][:, 1] < 0).all() and (E0["x"][:, 2] < 0).all() and (E0["y"][:, 2] < 0).all()
    assert (E0["x"][:, 2] % AMI_SCALE != 0).any() and (E0["x"][:, 2] % AMI_SCALE == 0).any()
    for a in after:
        assert np.array_equal(a["enemies"]["x"][:, :3], E0["x"][:, :3]) and np.array_equal(a["enemies"]["y"][:, :3], E0["y"][:, :3])
        assert np.array_equal(a["lives"], start["lives"])
        assert np.array_equal(a["player"]["x"][i % 3 == 0], start["player"]["x"][i % 3 == 0])
    # on its corner at tx = -1 an enemy walks onto the board; further out it finds no track
    dx, _ = _ami_moved(start, after[0], 3)
    assert np.array_equal(dx != 0, E0["x"][:, 3] == -AMI_WX) and (dx >= 0).all()
    if frame3 is not None:              # enemy 2's upper left pixel, which no other mover covers: floor(world / 16) - 1 from the origin
        px, py = AMI_OX + E0["x"][:, 2] // AMI_SCALE - 1, AMI_OY + E0["y"][:, 2] // AMI_SCALE - 1
        assert (frame3[i, py, px] == (255, 50, 100)).all()


AMI_JUNCTIONS_ROW12 = np.array([4, 9, 12, 19, 22, 27])       # columns with track above row 12 (rows 7..11) and none below it (row 13)


def build_amidar_player_arrivals(st, n):
    """the player one to three frames before junction (c, 12), coming from the left, with a history of (env % 8): 0 nothing, 1 the
    junction (0, 12) of the same row, 2 the junction (c, 6) of the same column (both stretches are painted), 3 a junction of another
    row and column, 4 (c, 18), with the gap of row 13 in between, 5 a number that is no tile (-5, 5000, 992, -1), 6 (c, 12) itself --
    and 7: walking down from (c, 12) onto (c, 13), which is no track"""
    i = np.arange(n)
    P = st["player"]
    c, v, k = AMI_JUNCTIONS_ROW12[(i // 8) % 6], i % 8, 1 + i % 3
    _ami_place(P, i, None, c, 12)
    P["x"] -= np.where(v == 7, 0, 8 * k)
    P["y"] += np.where(v == 7, AMI_WY - 8 * k, 0)
    P["step_tx"], P["step_ty"] = c, np.where(v == 7, 13, 12)
    here = 12 * AMI_BW + c
    past = [0 * c, 12 * AMI_BW + 0 * c, 6 * AMI_BW + c, 6 * AMI_BW + (c + 3) % AMI_BW, 18 * AMI_BW + c,
            np.array([-5, 5000, AMI_BW * AMI_BH, -1])[(i // 8) % 4], here, here]
    P["n_history"] = np.where(v == 0, 0, 1)
    P["history"][:, 0] = np.choose(v, past)
    st["score"] = 7 * i
    return st


def taken_amidar_player_arrivals(start, after, outs):
    n = len(start)
    i = np.arange(n)
    c, v, k = AMI_JUNCTIONS_ROW12[(i // 8) % 6], i % 8, 1 + i % 3
    T0 = start["tiles"]
    assert (T0[i, 13, c] == TILE_EMPTY).all() and (T0[:, 12, :] == TILE_UNPAINTED).all() and (T0[i[:, None], np.arange(6, 13)[None, :], c[:, None]] != TILE_EMPTY).all()
    at = lambda f: np.stack([f(a) for a in after])[k - 1, i]              # the value in the frame of the arrival
    assert np.array_equal(at(lambda a: a["player"]["x"]), AMI_WX * c) and np.array_equal(at(lambda a: a["player"]["y"]), AMI_WY * np.where(v == 7, 13, 12))
    assert (at(lambda a: a["player"]["step_tx"]) == -1).all()
    gain = at(lambda a: a["score"]) - start["score"]
    assert np.array_equal(gain, np.select([v == 1, v == 2], [c + 1, 7], 0)), "one point per newly painted tile, and only along a clear straight stretch"
    painted = (at(lambda a: a["tiles"]) == TILE_PAINTED).sum(axis=(1, 2)) - (T0 == TILE_PAINTED).sum(axis=(1, 2))
    assert np.array_equal(painted, gain)
    assert np.array_equal(at(lambda a: a["player"]["n_history"]), np.select([v == 0, v == 7], [1, 1], 2)), "every junction is remembered; (c, 13) is none"
    hist = at(lambda a: a["player"]["history"])
    assert (hist[v == 0, 0] == (12 * AMI_BW + c)[v == 0]).all() and (hist[(v > 0) & (v < 7), 1] == (12 * AMI_BW + c)[(v > 0) & (v < 7)]).all()
    assert len(np.unique(v)) == 8 and len(np.unique(start["player"]["history"][v == 5, 0])) == 4


# the directions every variant of build_amidar_protocol_branches must take in its first frame (worked out by hand from SPEC.md)
PERIMETER_WANT = [DIR_RIGHT, DIR_DOWN, DIR_LEFT, DIR_UP, DIR_LEFT, DIR_UP, None, DIR_DOWN]      # (variant 6: UP where (m, 29) is track, else RIGHT)
AMIDAR_WANT = [DIR_RIGHT, NONE, DIR_RIGHT, DIR_LEFT]
#             enemy tile, player tile, sees the player, ai.dir, tiles cut, the direction taken
TARGET_VARIANTS = [((11, 18), (15, 18), True, DIR_UP, [], DIR_RIGHT),              # the longer axis first: right
                   ((11, 18), (7, 18), True, DIR_UP, [], DIR_LEFT),                # left
                   ((11, 18), (11, 14), True, DIR_DOWN, [], DIR_UP),               # up
                   ((11, 18), (12, 12), True, DIR_DOWN, [], DIR_UP),               # up although one tile to the right
                   ((14, 18), (14, 12), True, DIR_LEFT, [], DIR_LEFT),             # up is closed and there is no second axis: ai.dir
                   ((14, 18), (15, 12), True, DIR_LEFT, [], DIR_RIGHT),            # up is closed: the second axis
                   ((14, 18), (15, 12), True, DIR_LEFT, [(15, 18)], DIR_LEFT),     # both closed: ai.dir
                   ((14, 18), (20, 15), False, DIR_UP, [], DIR_LEFT),              # out of sight, ai.dir closed: the first open one but back
                   ((7, 6), (20, 15), False, DIR_RIGHT, [(6, 6), (8, 6)], NONE),   # no way at all
                   ((7, 6), (20, 15), False, DIR_RIGHT, [(8, 6)], DIR_LEFT),       # a dead end: back
                   ((11, 12), (11, 16), True, DIR_UP, [], DIR_DOWN)]               # down
RANDOM_WANT = [[NONE], [DIR_LEFT], [DIR_RIGHT], [DIR_UP, DIR_RIGHT]]


def build_amidar_protocol_branches(st, n):
    """every protocol at each of its decision branches, on the default board with single tiles taken out.  Enemy 0, EnemyPerimeterAI
    (env % 8): on each corner, and on each side with the tile ahead missing.  Enemy 1, EnemyAmidarMvmt on a tile of row 12 with no
    track above or below (env % 4): arrived sideways and goes on, alone on its tile, arrived from above, at a dead end.  Enemy 2,
    EnemyTargetPlayer (env % 11): TARGET_VARIANTS.  Enemy 3, EnemyRandomMvmt on row 24 (env % 4): alone on its tile, at a dead end,
    in a corridor, at a junction.  The player stands (speed 0) where the hunter's variant wants it."""
    i = np.arange(n)
    T, E, P = st["tiles"], st["enemies"], st["player"]
    A = E["ai"]
    for name in A.dtype.names:
        A[name][:, :4] = 0
    E["speed"][:, :4] = np.where(i % 5 == 4, 5, 8)[:, None]
    # 0: the perimeter walker
    v, m = i % 8, 5 + (i // 8) % 20
    _ami_place(E, i, 0, np.choose(v, [0, 31, 31, 0, m, 31, m, 0]), np.choose(v, [0, 0, 30, 30, 0, m, 30, m]))
    A["kind"][:, 0] = AI_PERIMETER
    for var, (cx, cy) in ((4, (m + 1, 0 * m)), (5, (31 + 0 * m, m + 1)), (6, (m - 1, 30 + 0 * m)), (7, (0 * m, m - 1))):
        r = np.flatnonzero(v == var)
        T[r, cy[r], cx[r]] = TILE_EMPTY
    # 1: Amidar movement
    v, t = i % 4, 5 + (i // 4) % 4
    _ami_place(E, i, 1, t, 12)
    A["kind"][:, 1], A["horiz"][:, 1], A["vert"][:, 1] = AI_AMIDAR, DIR_RIGHT, np.where((i // 16) % 2 == 0, DIR_DOWN, DIR_UP)
    E["n_history"][:, 1] = 1
    E["history"][:, 1, 0] = np.where(v == 2, 11 * AMI_BW + t, 12 * AMI_BW + t - 1)
    r = np.flatnonzero((v == 1) | (v == 3))
    T[r, 12, t[r] + 1] = TILE_EMPTY
    r = np.flatnonzero(v == 1)
    T[r, 12, t[r] - 1] = TILE_EMPTY
    # 2: the hunter, and the player
    v = i % 11
    P["speed"] = 0
    A["kind"][:, 2] = AI_TARGET
    for var, (etile, ptile, sees, adir, cuts, _) in enumerate(TARGET_VARIANTS):
        r = np.flatnonzero(v == var)
        _ami_place(E, r, 2, *etile)
        _ami_place(P, r, None, *ptile)
        A["dir"][r, 2], A["vision_distance"][r, 2] = adir, (12 + (r // 11) % 3 if sees else (r // 11) % 3)
        for cx, cy in cuts:
            T[r, cy, cx] = TILE_EMPTY
    A["seen_tx"][:, 2] = A["seen_ty"][:, 2] = np.where(i % 2 == 0, -1, 5)
    # 3: the random walker
    v = i % 4
    _ami_place(E, i, 3, np.where(v == 3, 14, 9), 24)
    A["kind"][:, 3], A["dir"][:, 3] = AI_RANDOM, DIR_RIGHT
    r = np.flatnonzero(v <= 1)
    T[r, 24, 10] = TILE_EMPTY
    r = np.flatnonzero(v == 0)
    T[r, 24, 8] = TILE_EMPTY
    A["start_tx"][:, :4], A["start_ty"][:, :4] = E["x"][:, :4] // AMI_WX, E["y"][:, :4] // AMI_WY
    return st


def taken_amidar_protocol_branches(start, after, outs):
    n = len(start)
    i = np.arange(n)
    a0, E0, T0 = after[0], start["enemies"], start["tiles"]
    assert (E0["step_tx"][:, :4] == -1).all() and (E0["x"][:, :4] % AMI_WX == 0).all() and (E0["y"][:, :4] % AMI_WY == 0).all()
    m = 5 + (i // 8) % 20
    want = np.array([PERIMETER_WANT[k] if k != 6 else (DIR_UP if T0[e, 29, m[e]] else DIR_RIGHT) for e, k in enumerate(i % 8)])
    _ami_assert_dirs(start, a0, 0, want, "EnemyPerimeterAI")
    assert {DIR_UP, DIR_RIGHT} <= set(want[i % 8 == 6].tolist())
    _ami_assert_dirs(start, a0, 1, np.array(AMIDAR_WANT)[i % 4], "EnemyAmidarMvmt")
    flipped = np.isin(i % 4, (1, 3))
    A0, A1 = E0["ai"], a0["enemies"]["ai"]
    assert np.array_equal(A1["vert"][:, 1], np.where(flipped, A0["vert"][:, 1] ^ 1, A0["vert"][:, 1])), "neither way open: both preferences turn round"
    assert np.array_equal(A1["horiz"][:, 1], np.where(flipped, DIR_LEFT, DIR_RIGHT))
    _ami_assert_dirs(start, a0, 2, np.array([tv[5] for tv in TARGET_VARIANTS])[i % 11], "EnemyTargetPlayer")
    sees = np.array([tv[2] for tv in TARGET_VARIANTS])[i % 11]
    assert np.array_equal(A1["seen_tx"][:, 2], np.where(sees, start["player"]["x"] // AMI_WX, -1)) and np.array_equal(A1["seen_ty"][:, 2], np.where(sees, start["player"]["y"] // AMI_WY, -1))
    dx, dy = _ami_moved(start, a0, 3)
    sp = E0["speed"][:, 3]
    for var, dirs in enumerate(RANDOM_WANT):
        r = i % 4 == var
        ok = np.zeros(r.sum(), bool)
        for d in dirs:
            ok |= (dx[r] == sp[r] * AMI_DELTA[d][0]) & (dy[r] == sp[r] * AMI_DELTA[d][1])
        assert ok.all(), ("EnemyRandomMvmt", var)
    drew = (a0["rand"] != start["rand"]).any(axis=1)
    assert not drew[i % 4 <= 1].any() and drew[i % 4 == 3].all(), "only a walker with a choice draws"
    assert np.array_equal(a0["player"]["x"], start["player"]["x"]) and np.array_equal(a0["lives"], start["lives"])


def config_amidar_ragged_board(cfg):
    """the default board with its right-hand column missing beside the top boxes and its bottom row missing under the lower left
    one (boxes that run off the board are none), rows 6..12 turned into a mesh of 45 one-tile boxes (more boxes than the table of 64
    holds), ten more chase markers on row 12 (more than the eight the state keeps) and the player started on the bottom row, with
    no junction below it for its history"""
    B = cfg.board
    for y in range(1, 6):
        B[y][31] = TILE_EMPTY
    for x in range(1, 6):
        B[30][x] = TILE_EMPTY
    for y in range(6, 13):
        for x in range(AMI_BW):
            B[y][x] = TILE_UNPAINTED if (y % 2 == 0 or x % 2 == 0 or x == 31) else TILE_EMPTY
    for x in range(1, 11):
        B[12][x] = TILE_CHASE
    cfg.player_start_tx, cfg.player_start_ty = 31, 30


def build_amidar_ragged_board(st, n):
    """new games on that board; env % 3: 0 an enemy (another one from env to env) on the player, who is on its last life -- the game
    ends and a new one starts; 1 the same with three lives -- everybody is put back; 2 the whole board painted but tile (31, 27), and
    the player 1..3 frames below junction (31, 24) with (31, 30) as the last one: the board is complete and laid out again"""
    i = np.arange(n)
    v, k = i % 3, (i // 3) % 5
    T, E, P = st["tiles"], st["enemies"], st["player"]
    r = np.flatnonzero(v < 2)
    E["x"][r, k[r]], E["y"][r, k[r]] = P["x"][r], P["y"][r]
    E["step_tx"][r, k[r]] = E["step_ty"][r, k[r]] = -1
    st["lives"] = np.where(v == 0, 1, 3)
    st["jumps"] = np.where(v < 2, 0, 4)                           # (no jump left: FIRE cannot carry the player over the enemy)
    r = np.flatnonzero(v == 2)
    T[r] = np.where(T[r] != TILE_EMPTY, TILE_PAINTED, TILE_EMPTY)
    T[r, 27, 31] = TILE_UNPAINTED
    st["boxes"]["painted"][r] = 1
    _ami_place(P, r, None, 31, 24)
    P["y"][r] += 8 * (1 + (r // 3) % 3)
    P["step_tx"][r], P["step_ty"][r], P["n_history"][r] = 31, 24, 1
    P["history"][r, 0] = 30 * AMI_BW + 31
    st["level"], st["score"] = 1 + i % 4, 100 * i
    return st


def taken_amidar_ragged_board(start, after, outs):
    i = np.arange(len(start))
    v = i % 3
    assert (start["n_boxes"] == 64).all() and (start["n_chase_junctions"] == 8).all(), "both tables are full, and no fuller"
    new_player = lambda a, r: (a["player"]["x"][r] == AMI_WX * 31).all() and (a["player"]["y"][r] == AMI_WY * 30).all() and (a["player"]["n_history"][r] == 0).all()
    reward, done, lives, score = outs[0]
    assert done[v == 0].all() and not done[v != 0].any()
    a = after[0]
    assert (a["lives"][v == 0] == 3).all() and (a["score"][v == 0] == 0).all() and (a["level"][v == 0] == 1).all() and new_player(a, v == 0), "a new game"
    assert (a["lives"][v == 1] == 2).all() and np.array_equal(a["score"][v == 1], start["score"][v == 1]) and new_player(a, v == 1), "put back"
    for t in range(3):                                             # the frame of the arrival at (31, 24)
        assert new_player(after[t], (v == 2) & ((i // 3) % 3 == t)) and ((v == 2) & ((i // 3) % 3 == t)).any()
    a = after[-1]
    r = v == 2
    assert np.array_equal(a["level"][r], start["level"][r] + 1)
    assert not a["boxes"]["painted"][r].any() and (a["n_boxes"][r] == 64).all() and ((a["tiles"][r] == TILE_PAINTED).sum(axis=(1, 2)) == 6).all(), "the config's board again"
    assert (a["tiles"][r, 12, 1:11] == TILE_CHASE).all() and (a["tiles"][r, 1:6, 31] == TILE_EMPTY).all()


# ---------------------------------------------------------------- GridWorld (SPEC.md "GridWorld": at most one cell per frame)

GW_DIM = 32
GW_IDS = np.array([0, 0, 0, 0, 1, 3, 3, 2, 7, 200], np.uint8)       # floor, wall, reward, goal, and two numbers that name no tile (n_tiles is 4)
GW_MOVES = {2: (0, -1), 5: (0, 1), 4: (-1, 0), 3: (1, 0)}            # ALE UP, DOWN, LEFT, RIGHT


def build_gridworld_written_cells(st, n):
    """boards written cell by cell, the border included: floor, walls, rewards, goals and cells whose number names no tile (7 and 200
    with four tiles); every fourth board cut to 5 x 4, so that the player may stand outside it; the player anywhere from one cell
    left of / above the board to one cell right of / below it; every fifth game already over, with a reward on every side of the
    player; rewards of -2 in some tile tables, and
    collected reward cells that turn into walls"""
    rng = np.random.default_rng(31)
    i = np.arange(n)
    G = st["grid"].reshape(n, GW_DIM, GW_DIM).copy()
    G[:, :7, :9] = GW_IDS[rng.integers(0, len(GW_IDS), (n, 7, 9))]
    st["grid"] = G.reshape(st["grid"].shape)
    small = i % 4 == 3
    st["width"], st["height"] = np.where(small, 5, 9), np.where(small, 4, 7)
    st["player_x"] = np.where(rng.random(n) < 0.5, rng.integers(-1, 10, n), rng.choice([-1, 0, 8, 9], n))
    st["player_y"] = np.where(rng.random(n) < 0.5, rng.integers(-1, 8, n), rng.choice([-1, 0, 6, 7], n))
    st["game_over"] = i % 5 == 0
    r = np.flatnonzero(i % 5 == 0)                                # a finished game stands among rewards: one move would show in the score
    x, y = 1 + (r // 5) % 3, 1 + (r // 15) % 2
    st["player_x"][r], st["player_y"][r] = x, y
    for dx, dy in GW_MOVES.values():
        G[r, y + dy, x + dx] = 3
    st["grid"] = G.reshape(st["grid"].shape)
    st["score"] = 3 * i - 20
    st["reward_becomes"] = np.where(i % 7 == 0, 1, 0)
    st["tiles"]["reward"][:, 3] = np.where(i % 6 == 1, -2, 1)
    return st


def taken_gridworld_written_cells(start, after, outs):
    """the rule restated: every env followed until its game ends (the next frame starts a new game on the config's board)"""
    n = len(start)
    seen = set()
    for e in range(n):
        s = start[e]
        G = s["grid"].reshape(GW_DIM, GW_DIM).copy()
        x, y, score, over = int(s["player_x"]), int(s["player_y"]), int(s["score"]), bool(s["game_over"])
        for t in range(FRAMES):
            a = int(actions("gridworld", n, t)[e])
            if over:
                seen.add("over")
                assert outs[t][1][e] and outs[t][3][e] == score, "a finished game stays finished, and nothing is collected in it"
                assert all(G[y + dy, x + dx] == 3 for dx, dy in GW_MOVES.values())
                break
            if a not in GW_MOVES:
                seen.add("stands")
            else:
                nx, ny = x + GW_MOVES[a][0], y + GW_MOVES[a][1]
                if nx < 0 or ny < 0 or nx >= s["width"] or ny >= s["height"]:
                    seen.add("off " + ("left" if nx < 0 else "top" if ny < 0 else "right" if nx >= s["width"] else "bottom"))
                elif G[ny, nx] >= s["n_tiles"]:
                    seen.add("no tile %d" % G[ny, nx])
                elif not s["tiles"]["walkable"][G[ny, nx]]:
                    seen.add("wall")
                else:
                    tile = s["tiles"][G[ny, nx]]
                    x, y, score = nx, ny, score + int(tile["reward"])
                    seen.add("goal" if tile["goal"] else "reward %d" % tile["reward"] if tile["reward"] else "floor")
                    if tile["reward"]:
                        G[ny, nx] = s["reward_becomes"]
                    over = bool(tile["goal"])
            assert outs[t][3][e] == score and bool(outs[t][1][e]) == over, (e, t)
            if over:
                seen.add("ends")
                break
            b = after[t][e]
            assert (int(b["player_x"]), int(b["player_y"]), int(b["score"]), int(b["game_over"])) == (x, y, score, 0), (e, t)
            assert np.array_equal(b["grid"].reshape(GW_DIM, GW_DIM), G), (e, t)
    want = {"over", "stands", "off left", "off top", "off right", "off bottom", "no tile 7", "no tile 200", "wall", "floor", "reward 1", "reward -2", "goal", "ends"}
    assert want <= seen, sorted(want - seen)


class Case:
    def __init__(self, name, game, build, taken, canonical=True, config=None):
        self.name, self.game, self.build, self.taken = name, game, build, taken
        self.canonical = canonical            # Breakout: the wall stays canonical, so TBX_OPT_STEP_FORM 1 really is a thread per env
        self.config = config                  # config(cfg): edits the game's default config record in place

    @property
    def forms(self):
        return [f for f in FORMS[self.game] if self.canonical or f != "batch1"]

    def __repr__(self):
        return self.name


CASES = [
    Case("breakout_radius_nonpositive", "breakout", build_radius_nonpositive, taken_radius_nonpositive, True),
    Case("breakout_indestructible_hit", "breakout", build_indestructible_hit, taken_indestructible_hit, False),
    Case("breakout_speed_rows", "breakout", build_speed_rows, taken_speed_rows, True),
    Case("breakout_wall_returns", "breakout", build_wall_returns, taken_wall_returns, False),
    Case("breakout_paint_extremes", "breakout", build_paint_extremes, taken_paint_extremes, True),
    Case("breakout_paint_extremes_bricks", "breakout", functools.partial(build_paint_extremes, bricks=True),
         functools.partial(taken_paint_extremes, bricks=True), False),
    Case("breakout_paddle_zero_width", "breakout", build_paddle_zero_width, taken_paddle_zero_width, True),
    Case("si_sideways_lasers", "space_invaders", build_si_sideways_lasers, taken_si_sideways_lasers, True),
    Case("si_ship_laser_at_ground", "space_invaders", build_si_ship_laser_at_ground, taken_si_ship_laser_at_ground, True),
    Case("si_full_laser_table", "space_invaders", build_si_full_laser_table, taken_si_full_laser_table, True),
    Case("si_empty_formation", "space_invaders", build_si_empty_formation, taken_si_empty_formation, True),
    Case("si_dead_ship_idle", "space_invaders", build_si_dead_ship_idle, taken_si_dead_ship_idle, True),
    Case("si_ufo_removed", "space_invaders", build_si_ufo_removed, taken_si_ufo_removed, True),
    Case("amidar_lookup_tables", "amidar", build_amidar_lookup_tables, taken_amidar_lookup_tables),
    Case("amidar_odd_movers", "amidar", build_amidar_odd_movers, taken_amidar_odd_movers),
    Case("amidar_negative_world", "amidar", build_amidar_negative_world, taken_amidar_negative_world),
    Case("amidar_player_arrivals", "amidar", build_amidar_player_arrivals, taken_amidar_player_arrivals),
    Case("amidar_protocol_branches", "amidar", build_amidar_protocol_branches, taken_amidar_protocol_branches),
    Case("amidar_ragged_board", "amidar", build_amidar_ragged_board, taken_amidar_ragged_board, config=config_amidar_ragged_board),
    Case("gridworld_written_cells", "gridworld", build_gridworld_written_cells, taken_gridworld_written_cells),
]
BY_NAME = {c.name: c for c in CASES}


# ================================================================ playing a case

def actions(game, n, t):
    return synthetic_actions(game, n, t, seed=ACTION_SEED)


def fresh(case, n, lib, step_form=0):
    e = Engine(case.game, n, lib=lib)
    if step_form:
        e.set_option(_abi.OPT_STEP_FORM, step_form)
    if case.config:
        cfg = e.get_config()
        case.config(cfg)
        e.set_config(cfg)
    e.seed(ENGINE_SEED)
    e.new_game()
    return e


def start_records(case, n, lib):
    with fresh(case, n, lib) as o:
        return case.build(o.get_states_np(), n)


def play(case, n, lib, form, start):
    """the case through one form on a fresh engine of `lib`: a dict of everything that form is compared on"""
    game = case.game
    with fresh(case, n, lib, {"batch1": 1, "batch2": 2}.get(form, 0)) as e:
        e.set_states_np(0, start)
        out = {"written": states_bytes(e)}
        H, W = e.height, e.width
        if form in ("batch", "batch1", "batch2"):
            for ch in (1, 3, 4):
                out["frame%d" % ch] = e.render(ch)
            for t in range(FRAMES):
                for name, v in zip(("reward", "done", "lives", "score"), e.step(actions(game, n, t), auto_reset=True)):
                    out["%s%d" % (name, t)] = v.copy()
                out["states%d" % t] = states_bytes(e)
            out["frame_last"] = e.render(3)
        elif form == "synthetic":
            for t in range(FRAMES):
                e.step_synthetic(ACTION_SEED, t, auto_reset=True)
                out["packed%d" % t] = read_buffer(e, _abi.BUF_PACKED, (n,), np.uint64)
                out["states%d" % t] = states_bytes(e)
        elif form == "rollout":
            e.rollout_synthetic(ACTION_SEED, 0, FRAMES, channels=3, auto_reset=True)
            out["frames"] = read_buffer(e, _abi.BUF_ROLLOUT_FRAMES, (FRAMES, n, H, W, 3))
            out["packed"] = read_buffer(e, _abi.BUF_ROLLOUT_PACKED, (FRAMES, n), np.uint64)
            out["states"] = states_bytes(e)
        elif form == "agent":
            e.agent_init(**AGENT)
            obs, reward, done = e.agent_step(actions(game, n, 0))
            out.update(obs=obs, reward=reward, done=done, states=states_bytes(e))
        elif form == "lookahead":
            plan = np.stack([actions(game, n, t) for t in range(FRAMES)], axis=1)
            if engine_is_oracle(e):                      # the checker has no planner of its own: the plan replayed on a second engine
                with fresh(case, n, lib) as c:
                    c.set_states(0, e.get_states())
                    for i, r in enumerate(sim_rngs(e)):
                        c.set_sim_rng((int(r[0]), int(r[1])), env=i)
                    rows = play_plan(c, game, plan_columns(n, frames=FRAMES, depth=FRAMES, code=plan_code(game, plan)))
            else:
                rows = e.lookahead_plan(FRAMES, plan)
            out.update(rows)
            out["states"] = states_bytes(e)
        else:
            raise ValueError(form)
        return out


_STARTS, _EXPECTED = {}, {}           # (case name, envs) -> start records; (case name, envs, form) -> play() over the oracle


def start_of(case, n, oracle_lib):
    """the case's start records, built once from the oracle's new game and left unchanged"""
    key = (case.name, n)
    if key not in _STARTS:
        _STARTS[key] = start_records(case, n, oracle_lib)
        _STARTS[key].flags.writeable = False
    return _STARTS[key]


def expected(case, n, form, oracle_lib):
    """the oracle's side of (case, envs, form), computed once and left unchanged"""
    key = (case.name, n, form)
    if key not in _EXPECTED:
        _EXPECTED[key] = play(case, n, oracle_lib, form, start_of(case, n, oracle_lib))
        for v in _EXPECTED[key].values():
            v.flags.writeable = False
    return _EXPECTED[key]


def as_records(game, raw):
    """uint8[n, record size] (states_bytes) -> the records as a numpy structured array"""
    return np.frombuffer(raw.tobytes(), dtype=np.dtype(_abi.STATE_TYPES[_abi.GAME_IDS[game]]))


# ================================================================ the device cases

@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case,form", [(c, f) for c in CASES for f in c.forms], ids=lambda v: v if isinstance(v, str) else repr(v))
def test_rule_edge(case, form, n, hip_lib, oracle_lib):
    want = expected(case, n, form, oracle_lib)
    got = play(case, n, hip_lib, form, start_of(case, n, oracle_lib))
    assert sorted(got) == sorted(want)
    for key in want:
        if not np.array_equal(got[key], want[key]):
            a, b = got[key], want[key]
            bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
            raise AssertionError("%s %d envs, %s: %s differs in %d rows of %d, first %s" % (case, n, form, key, len(bad), a.shape[0], bad[:8]))


# ================================================================ the twins

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_takes_its_branch(case, n, oracle_lib):
    """the predicate of the case's branch on the oracle's own states; the envs are no copies of each other; and the oracle's other forms
    land where its batch steps land"""
    start = start_of(case, n, oracle_lib)
    batch = case.forms[0]
    ref = expected(case, n, batch, oracle_lib)
    after = [as_records(case.game, ref["states%d" % t]) for t in range(FRAMES)]
    outs = [[ref["%s%d" % (name, t)] for name in ("reward", "done", "lives", "score")] for t in range(FRAMES)]
    if case.name == "amidar_negative_world":
        case.taken(start, after, outs, frame3=ref["frame3"])
    else:
        case.taken(start, after, outs)
    assert len(np.unique(ref["written"], axis=0)) >= min(n, 10), "the envs of a case differ from each other"
    for form in [f for f in case.forms[1:] if f in ("batch2", "synthetic")]:
        other = expected(case, n, form, oracle_lib)
        assert all(np.array_equal(other["states%d" % t], ref["states%d" % t]) for t in range(FRAMES)), form
    assert np.array_equal(expected(case, n, "rollout", oracle_lib)["states"], ref["states%d" % (FRAMES - 1)])
    assert np.array_equal(expected(case, n, "lookahead", oracle_lib)["states"], ref["written"]), "a lookahead leaves the engine alone"


def reach(oracle_lib):
    """tests/rule_reach.py script: every case through every form over the oracle alone"""
    for case in CASES:
        for n in SIZES[:1]:
            for form in case.forms:
                play(case, n, oracle_lib, form, start_records(case, n, oracle_lib))
