"""Palettes other than the default one, and states in which the draw order shows (tests/test_gpu_palettes.py).

Every picture path converts the palette for itself (pack_color into the config tables, pix_of<C> in each rasteriser, the gray
tables of the fused observation kernels, the resident painters), and with the default colours most of what they could get wrong
is invisible: every background is black, Breakout's paddle and ball share one colour, every alpha is 255.  Here:

* DISTINCT: every colour field of a game gets a colour of its own -- pairwise distinct in r, in g, in b and in the gray byte
  (77 r + 150 g + 29 b + 128) >> 8, no channel 0 or 255 (so no background is black), alphas from {0, 1, 128, 254};
* GRAY_TIES: DISTINCT with pairs that differ in RGB and share one gray byte (Breakout paddle / ball and frame / bg, Amidar
  painted / inner-painted and player / enemy, GridWorld player / floor, SpaceInvaders ship / shield 0) and one pair equal in RGB;
* states, written over mid-game records, in which one entity lies on another, so that the order they are painted in decides pixels.

A palette is written into the POD records: the config (Breakout, Amidar, GridWorld -- followed by a new game, which is where
Breakout's bricks and GridWorld's tiles take their colours from) or the state records (SpaceInvaders: ship, shields and lasers
carry their colours per env).  Nothing here asserts about an engine; the property assertions are about the palettes themselves.
"""
import functools

import numpy as np

from support import DONOR_FRAMES, donor_records, synthetic_actions
from toybox_amd import Engine, _abi

ALPHAS = (0, 1, 128, 254)
N_ENVS = 257                                   # ragged for 64-lane waves and 256-thread blocks
SEED, ACTION_SEED = 4711, 1337

BRK_ROWS = 14                                  # TBX_BRK_MAX_ROWS: every row colour of the record is on the screen
BRK_ROW_SCORES = [7, 7, 7, 7, 4, 4, 4, 4, 4, 1, 1, 1, 1, 1]
AMI_FIELDS = ("bg_color", "player_color", "unpainted_color", "painted_color", "enemy_color", "inner_painted_color")
BRK_FIELDS = ("bg_color", "frame_color", "paddle_color", "ball_color")
SI_ROLES = ("ship", "shield0", "shield1", "shield2", "ship_laser") + tuple("enemy_laser%d" % k for k in range(8))
GW_TILES = 4                                   # the default board's tile table


def luma(rgb):
    """the gray byte of SPEC.md: (77 r + 150 g + 29 b + 128) >> 8, over the last axis"""
    c = np.asarray(rgb, np.int64)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def distinct_colors(k, seed):
    """uint8[k][4] rgba: per channel k different values from 1 .. 254, k different gray bytes, alphas from ALPHAS in turn"""
    rng = np.random.default_rng(seed)
    while True:
        rgb = np.stack([rng.permutation(np.arange(1, 255))[:k] for _ in range(3)], axis=1)
        if len(set(luma(rgb).tolist())) == k:
            break
    return np.concatenate([rgb, np.asarray(ALPHAS)[(np.arange(k) + seed) % 4][:, None]], axis=1).astype(np.uint8)


def assert_distinct(colors):
    """the properties of a DISTINCT palette, colors uint8[k][4]"""
    c = np.asarray(colors)
    k = len(c)
    for ch, name in enumerate("rgb"):
        assert len(set(c[:, ch].tolist())) == k, "%s values repeat" % name
    assert len(set(luma(c[:, :3]).tolist())) == k, "gray bytes repeat"
    assert ((c[:, :3] > 0) & (c[:, :3] < 255)).all(), "a channel is 0 or 255"
    assert set(c[:, 3].tolist()) <= set(ALPHAS) and 255 not in c[:, 3], "alphas must come from %r" % (ALPHAS,)
    assert c[:, :3].any(axis=1).all(), "black"


def gray_twin(color, taken=()):
    """another rgba with the same gray byte, no channel 0 or 255 and another RGB than `color` and everything in `taken`"""
    r, g, b, a = (int(v) for v in color)
    want = int(luma([r, g, b]))
    used = {tuple(int(v) for v in t[:3]) for t in taken} | {(r, g, b)}
    for dr in range(3, 60):
        for sign in (1, -1):
            r2 = r + sign * dr
            for b2 in range(1, 255):
                if 1 <= r2 <= 254 and (r2, g, b2) not in used and int(luma([r2, g, b2])) == want and b2 != b:
                    return np.asarray([r2, g, b2, ALPHAS[(a + 1) % 4 if a in ALPHAS else 0]], np.uint8)
    raise AssertionError("no gray twin for %r" % (color,))


def assert_gray_tie(a, b):
    assert tuple(a[:3]) != tuple(b[:3]) and luma(a[:3]) == luma(b[:3]), (a, b)


# ---------------------------------------------------------------- the palettes, by game
# A palette is a dict role -> uint8[4] (Breakout, Amidar, GridWorld) or role -> uint8[N][4] (SpaceInvaders: per env).

def _named(names, colors):
    return {n: np.asarray(c, np.uint8) for n, c in zip(names, colors)}


def breakout_roles():
    return BRK_FIELDS + tuple("row%d" % r for r in range(BRK_ROWS))


def gridworld_roles():
    return ("player_color",) + tuple("tile%d" % t for t in range(GW_TILES))


@functools.lru_cache(maxsize=None)
def palette(game, name, n=N_ENVS):
    """DISTINCT, GRAY_TIES or a second DISTINCT one ("OTHER", what tbx_set_config switches to between calls)"""
    seed = {"DISTINCT": 11, "GRAY_TIES": 11, "OTHER": 29}[name]
    if game == "space_invaders":
        per_env = np.stack([distinct_colors(len(SI_ROLES), seed * 1000 + i) for i in range(n)])      # [n][roles][4]
        for i in range(n):
            assert_distinct(per_env[i])
        first = per_env[:, :4].reshape(n, -1)
        assert len({bytes(r) for r in first}) == n, "ship and shield colours repeat from env to env"
        pal = {role: per_env[:, k].copy() for k, role in enumerate(SI_ROLES)}
        if name == "GRAY_TIES":
            pal["shield0"] = np.stack([gray_twin(c) for c in pal["ship"]])
            pal["shield2"] = pal["shield1"].copy()
            pal["enemy_laser0"] = np.stack([gray_twin(c) for c in pal["shield1"]])
            for i in (0, n - 1):
                assert_gray_tie(pal["ship"][i], pal["shield0"][i])
        return pal
    roles = {"breakout": breakout_roles(), "amidar": AMI_FIELDS, "gridworld": gridworld_roles()}[game]
    colors = distinct_colors(len(roles), seed + len(roles))
    assert_distinct(colors)
    pal = _named(roles, colors)
    if name == "GRAY_TIES":
        taken = list(pal.values())
        if game == "breakout":
            pal["ball_color"] = gray_twin(pal["paddle_color"], taken)
            pal["bg_color"] = gray_twin(pal["frame_color"], taken)
            pal["row1"] = pal["row0"].copy()
            pal["row3"] = gray_twin(pal["row2"], taken)
            ties = [("paddle_color", "ball_color"), ("frame_color", "bg_color"), ("row2", "row3")]
        elif game == "amidar":
            pal["inner_painted_color"] = gray_twin(pal["painted_color"], taken)
            pal["enemy_color"] = gray_twin(pal["player_color"], taken)
            pal["bg_color"] = pal["unpainted_color"].copy()
            pal["bg_color"][3] = ALPHAS[0]
            ties = [("painted_color", "inner_painted_color"), ("player_color", "enemy_color")]
        else:
            pal["player_color"] = gray_twin(pal["tile0"], taken)
            pal["tile3"] = pal["tile2"].copy()
            ties = [("tile0", "player_color")]
        for a, b in ties:
            assert_gray_tie(pal[a], pal[b])
        assert all(((c[:3] > 0) & (c[:3] < 255)).all() and c[3] in ALPHAS for c in pal.values())
    return pal


def _color(c):
    return _abi.Color(*(int(v) for v in c))


def palette_config(e, pal):
    """the engine's config record with the palette written into it (Breakout: on a wall of 14 rows, so that every row colour is
    on the screen; SpaceInvaders has no colour in its config)"""
    cfg = e.get_config()
    if e.game == "breakout":
        for f in BRK_FIELDS:
            setattr(cfg, f, _color(pal[f]))
        cfg.n_rows = BRK_ROWS
        for r in range(BRK_ROWS):
            cfg.row_scores[r] = BRK_ROW_SCORES[r]
            cfg.row_colors[r] = _color(pal["row%d" % r])
    elif e.game == "amidar":
        for f in AMI_FIELDS:
            setattr(cfg, f, _color(pal[f]))
    elif e.game == "gridworld":
        assert cfg.n_tiles == GW_TILES
        cfg.player_color = _color(pal["player_color"])
        for t in range(GW_TILES):
            cfg.tiles[t].color = _color(pal["tile%d" % t])
    return cfg


def _put(field, colors):
    """a colour field of a numpy record view <- uint8[..., 4]"""
    c = np.asarray(colors, np.uint8)
    for k, ch in enumerate("rgba"):
        field[ch] = c[..., k]


def si_write_palette(st, pal):
    """ship, shields and every laser slot of the records st (env i: row i of the palette)"""
    n = len(st)
    _put(st["ship_color"], pal["ship"][:n])
    for k in range(3):
        _put(st["shield_color"][:, k], pal["shield%d" % k][:n])
    _put(st["ship_laser"]["color"], pal["ship_laser"][:n])
    for k in range(8):
        _put(st["enemy_lasers"]["color"][:, k], pal["enemy_laser%d" % k][:n])


# ---------------------------------------------------------------- states in which the draw order shows
# env i belongs to class i % CLASSES; each class is one overlap, the last ones are left as the game played them.
CLASSES = 8
OVERLAPS = {"breakout": ("ball on paddle", "ball on side wall", "ball in brick row", "two balls", "hud digits"),
            "amidar": ("player on enemy", "two enemies on one tile", "mover on painted tile", "mover on box interior"),
            "space_invaders": ("laser on shield", "laser on ship", "ship dying", "ship laser on shield", "eight lasers"),
            "gridworld": ()}


def _f2i(v):
    return np.trunc(np.clip(v, -1.0e6, 1.0e6)).astype(np.int64)          # (the painters' float -> int: truncation)


def _cls(n, k):
    return np.arange(n) % CLASSES == k


def breakout_overlaps(st):
    n = len(st)
    live = _cls(n, 0) | _cls(n, 1) | _cls(n, 2) | _cls(n, 3)
    st["n_balls"][live] = np.maximum(st["n_balls"][live], 1)
    st["is_dead"][live] = 0
    st["ball_radius"][live] = 2.0
    m = _cls(n, 0)                                                          # the ball's lower half inside the paddle
    st["paddle_x"][m] = 40.0 + 7.0 * (np.arange(n)[m] % 23)
    st["ball_x"][m, 0] = st["paddle_x"][m] + 3.0
    st["ball_y"][m, 0] = st["paddle_y"][m] + 1.0
    st["ball_vx"][m, 0], st["ball_vy"][m, 0] = 0.5, -1.0
    m = _cls(n, 1)                                                          # inside a side wall's columns, left and right in turn
    right = m & (np.arange(n) % (2 * CLASSES) >= CLASSES)
    st["ball_x"][m, 0] = 9.0
    st["ball_x"][right, 0] = 231.0
    st["ball_y"][m, 0] = 100.0 + (np.arange(n)[m] % 40)
    st["ball_vx"][m, 0], st["ball_vy"][m, 0] = 0.0, 1.0
    m = np.flatnonzero(_cls(n, 2))                                          # the centre of a brick that is alive
    for i in m:
        alive = np.flatnonzero(st["bricks"]["alive"][i, :st["n_bricks"][i]])
        j = alive[(7 * i) % len(alive)]
        b = st["bricks"][i, j]
        st["ball_x"][i, 0], st["ball_y"][i, 0] = b["x"] + 6.0, b["y"] + 2.0
        st["ball_vx"][i, 0], st["ball_vy"][i, 0] = 0.25, 0.25
    m = _cls(n, 3)                                                          # a second ball two pixels off the first, in the open
    st["n_balls"][m] = 2
    st["ball_x"][m, 0], st["ball_y"][m, 0] = 60.0 + (np.arange(n)[m] % 100), 120.0
    st["ball_x"][m, 1], st["ball_y"][m, 1] = st["ball_x"][m, 0] + 2.0, st["ball_y"][m, 0] + 1.0
    st["ball_vx"][m, 0], st["ball_vy"][m, 0] = 1.0, 1.0
    st["ball_vx"][m, 1], st["ball_vy"][m, 1] = -0.5, 1.5
    m = _cls(n, 4)                                                          # every digit glyph somewhere in the HUD
    d = (np.arange(n)[m] // CLASSES) % 10                                   # five consecutive digits, the sixth as lives, the seventh as level
    st["score"][m] = sum(((d + j) % 10) * 10 ** (4 - j) for j in range(5))
    st["lives"][m] = np.where((d + 5) % 10 == 0, 1, (d + 5) % 10)
    st["level"][m] = (d + 6) % 10
    return st


def _ball_rects(st, b):
    r = st["ball_radius"]
    x0, y0 = _f2i(st["ball_x"][:, b] - r), _f2i(st["ball_y"][:, b] - r)
    side = _f2i(r * 2.0)
    return x0, y0, x0 + side, y0 + side


def _meet(a, b):
    return (a[0] < b[2]) & (b[0] < a[2]) & (a[1] < b[3]) & (b[1] < a[3])


def hud_digits(st):
    """int[n][7]: the digits Breakout's HUD shows -- the score's five, lives, level"""
    sc = np.clip(st["score"], 0, None) % 100000
    return np.stack([(sc // 10 ** p) % 10 for p in (4, 3, 2, 1, 0)] + [np.clip(st["lives"], 0, 9), np.clip(st["level"], 0, None) % 10], axis=1)


def hud_full(st):
    """bool[n]: the HUD shows five different score digits and at least a sixth glyph as lives or level -- what the class written
    for the HUD holds and a record 400 frames into its game does not (its score has leading zeros)"""
    d = hud_digits(st)
    return np.asarray([len(set(row[:5].tolist())) == 5 and len(set(row.tolist())) >= 6 for row in d])


def breakout_overlap_counts(st):
    """envs in which each overlap of OVERLAPS["breakout"] holds, from the state records alone"""
    has = st["n_balls"] >= 1
    ball = _ball_rects(st, 0)
    px0 = _f2i(st["paddle_x"] - st["paddle_width"] * 0.5)
    paddle = (px0, _f2i(st["paddle_y"]), px0 + _f2i(st["paddle_width"]), _f2i(st["paddle_y"]) + 3)
    in_frame = (ball[1] >= 25) & (ball[3] <= 160)
    wall = has & in_frame & (((ball[0] < 12) & (ball[2] > 0)) | ((ball[2] > 228) & (ball[0] < 240)))
    brick = np.zeros(len(st), bool)
    for i in np.flatnonzero(has):
        k = st["bricks"][i, :st["n_bricks"][i]]
        k = k[k["alive"] != 0]
        rect = (_f2i(k["x"]), _f2i(k["y"]), _f2i(k["x"]) + _f2i(k["w"]), _f2i(k["y"]) + _f2i(k["h"]))
        brick[i] = _meet(tuple(v[i] for v in ball), rect).any()
    two = (st["n_balls"] >= 2) & _meet(ball, _ball_rects(st, 1))
    return {"ball on paddle": int((has & _meet(ball, paddle)).sum()), "ball on side wall": int(wall.sum()),
            "ball in brick row": int(brick.sum()), "two balls": int(two.sum()), "hud digits": int(hud_full(st).sum())}


def breakout_custom_table(st, pal):
    """the same states on per-env brick tables (the CUSTOM kernels): brick j painted in the colour of row (row + col) % 14"""
    rows = np.stack([pal["row%d" % r] for r in range(BRK_ROWS)])
    pick = (st["bricks"]["row"] + st["bricks"]["col"]) % BRK_ROWS
    slot = np.arange(st["bricks"].shape[1])[None, :] < st["n_bricks"][:, None]
    for k, ch in enumerate("rgba"):
        st["bricks"]["color"][ch] = np.where(slot, rows[pick, k], st["bricks"]["color"][ch])
    return st


AMI_PAINTED = 2


def _ami_put(m, rows, slot, tx, ty):
    """mover `slot` (None: the player) of the envs `rows` onto tile (tx, ty), at rest"""
    who = m["player"] if slot is None else m["enemies"]
    idx = rows if slot is None else (rows, slot)
    who["x"][idx], who["y"][idx] = 64 * tx, 80 * ty
    who["step_tx"][idx], who["step_ty"][idx] = tx, ty
    who["caught"][idx] = 0


def amidar_overlaps(st):
    n = len(st)
    ptx, pty = st["player"]["x"] // 64, st["player"]["y"] // 80
    m = np.flatnonzero(_cls(n, 0))                                          # enemy 0 exactly on the player
    for f in ("x", "y", "step_tx", "step_ty"):
        st["enemies"][f][m, 0] = st["player"][f][m]
    st["enemies"]["caught"][m, 0] = 0
    m = np.flatnonzero(_cls(n, 1))                                          # enemy 1 on enemy 2's tile, half a tile off
    st["enemies"]["x"][m, 1], st["enemies"]["y"][m, 1] = st["enemies"]["x"][m, 2] + 32, st["enemies"]["y"][m, 2]
    st["enemies"]["caught"][m, 1] = st["enemies"]["caught"][m, 2] = 0
    m = np.flatnonzero(_cls(n, 2))                                          # the player's tile and its row neighbours painted
    for i in m:
        row = st["tiles"][i, pty[i]]
        near = np.arange(max(0, ptx[i] - 2), min(32, ptx[i] + 3))
        row[near] = np.where(row[near] != 0, AMI_PAINTED, 0)
    m = np.flatnonzero(_cls(n, 3))                                          # enemy 3 on the top-left corner of a painted box
    for i in m:
        b = 1 + (i // CLASSES) % (st["n_boxes"][i] - 1)
        st["boxes"]["painted"][i, b] = 1
        _ami_put(st, np.asarray([i]), 3, st["boxes"]["tl_tx"][i, b], st["boxes"]["tl_ty"][i, b])
    return st


def _ami_rect(x, y):
    x0, y0 = 16 + x // 16 - 1, 37 + y // 16 - 1                              # (world -> pixel: floor(v / 16), positions are >= 0)
    return x0, y0, x0 + 6, y0 + 7


def amidar_pixel(st, i, x, y, pal):
    """the RGB of pixel (x, y) of env i by SPEC.md's order, from the record alone: background, the interiors of painted boxes, the
    track, the enemies in index order, the player (the HUD rows are not asked for)"""
    col = pal["bg_color"]
    for b in range(st["n_boxes"][i]):
        bx = st["boxes"][i, b]
        if bx["painted"] and 16 + 4 * (bx["tl_tx"] + 1) <= x < 16 + 4 * bx["br_tx"] and 37 + 5 * (bx["tl_ty"] + 1) <= y < 37 + 5 * bx["br_ty"]:
            col = pal["inner_painted_color"]
    tx, ty = (x - 16) // 4, (y - 37) // 5
    if 0 <= tx < 32 and 0 <= ty < 31 and x >= 16 and y >= 37 and st["tiles"][i, ty, tx] != 0:
        col = pal["painted_color"] if st["tiles"][i, ty, tx] == AMI_PAINTED else pal["unpainted_color"]
    for k in range(st["n_enemies"][i]):
        r = _ami_rect(int(st["enemies"]["x"][i, k]), int(st["enemies"]["y"][i, k]))
        if not st["enemies"]["caught"][i, k] and r[0] <= x < r[2] and r[1] <= y < r[3]:
            col = pal["enemy_color"]
    r = _ami_rect(int(st["player"]["x"][i]), int(st["player"]["y"][i]))
    if r[0] <= x < r[2] and r[1] <= y < r[3]:
        col = pal["player_color"]
    return tuple(int(v) for v in col[:3])


def amidar_overlap_counts(st):
    n = len(st)
    en = st["enemies"]
    shown = (np.arange(8)[None, :] < st["n_enemies"][:, None]) & (en["caught"] == 0)
    player = _ami_rect(st["player"]["x"], st["player"]["y"])
    rect = _ami_rect(en["x"], en["y"])
    on_enemy = (shown & _meet(tuple(v[:, None] for v in player), rect)).any(axis=1)
    pair = np.zeros(n, bool)
    for a in range(8):
        for b in range(a + 1, 8):
            pair |= shown[:, a] & shown[:, b] & _meet(tuple(v[:, a] for v in rect), tuple(v[:, b] for v in rect)) & \
                ((en["x"][:, a] != en["x"][:, b]) | (en["y"][:, a] != en["y"][:, b]))
    ptx, pty = np.clip(st["player"]["x"] // 64, 0, 31), np.clip(st["player"]["y"] // 80, 0, 30)
    painted = st["tiles"][np.arange(n), pty, ptx] == AMI_PAINTED
    inner = np.zeros(n, bool)
    for i in range(n):
        for b in np.flatnonzero(st["boxes"]["painted"][i, :st["n_boxes"][i]]):
            bx = st["boxes"][i, b]
            box = (16 + 4 * (bx["tl_tx"] + 1), 37 + 5 * (bx["tl_ty"] + 1), 16 + 4 * bx["br_tx"], 37 + 5 * bx["br_ty"])
            movers = [tuple(v[i] for v in player)] + [tuple(v[i, k] for v in rect) for k in np.flatnonzero(shown[i])]
            inner[i] |= any(_meet(mv, box) for mv in movers)
    return {"player on enemy": int(on_enemy.sum()), "two enemies on one tile": int(pair.sum()),
            "mover on painted tile": int(painted.sum()), "mover on box interior": int(inner.sum())}


SI_DOWN, SI_UP = 1, 0


def _si_laser(l, idx, x, y, movement, speed):
    l["x"][idx], l["y"][idx], l["w"][idx], l["h"][idx] = x, y, 2, 8
    l["t"][idx], l["movement"][idx], l["speed"][idx] = 0, movement, speed


def si_overlaps(st):
    n = len(st)
    env = np.arange(n)
    st["n_shields"][:] = 3
    m = np.flatnonzero(_cls(n, 0))                                          # an enemy laser inside a whole shield
    k = (m // CLASSES) % 3
    st["shield_rows"][m, k] = 0xFFFF
    st["n_enemy_lasers"][m] = np.maximum(st["n_enemy_lasers"][m], 1)
    _si_laser(st["enemy_lasers"], (m, 0), st["shield_x"][m, k] + 7, st["shield_y"][m, k] + 3, SI_DOWN, 3)
    m = np.flatnonzero(_cls(n, 1))                                          # an enemy laser reaching into the ship
    st["ship_alive"][m], st["ship_death_counter"][m] = 1, -1
    st["n_enemy_lasers"][m] = np.maximum(st["n_enemy_lasers"][m], 1)
    _si_laser(st["enemy_lasers"], (m, 0), st["ship_x"][m] + 7, st["ship_y"][m] - 3, SI_DOWN, 3)
    m = np.flatnonzero(_cls(n, 2))                                          # the ship dying, both explosion sprites
    st["ship_alive"][m], st["ship_death_counter"][m] = 0, 6 + env[m] % 20
    st["ship_death_hit_1"][m] = (env[m] // CLASSES) % 2
    m = np.flatnonzero(_cls(n, 3))                                          # the ship's laser inside a whole shield
    k = (m // CLASSES) % 3
    st["shield_rows"][m, k] = 0xFFFF
    st["has_ship_laser"][m] = 1
    _si_laser(st["ship_laser"], m, st["shield_x"][m, k] + 3, st["shield_y"][m, k] + 8, SI_UP, 6)
    # all eight laser slots in the open, between the shields' columns, and a ship laser left of the formation's field -- one pixel
    # per frame, so that they are still in flight 48 frames on (the agent window)
    m = np.flatnonzero(_cls(n, 4))
    st["n_enemy_lasers"][m] = 8
    for q, x in enumerate((26, 40, 54, 68, 110, 124, 138, 176)):
        _si_laser(st["enemy_lasers"], (m, q), x + env[m] % 5, 96 + 4 * q, SI_DOWN, 1)
    m = np.flatnonzero(_cls(n, 4) | _cls(n, 5))
    st["has_ship_laser"][m] = 1
    _si_laser(st["ship_laser"], m, 10 + env[m] % 5, 170, SI_UP, 1)
    return st


def _si_rect(l, q=None):
    x, y, w, h = (l[f] if q is None else l[f][:, q] for f in ("x", "y", "w", "h"))
    return x, y, x + w, y + h


def si_overlap_counts(st):
    n = len(st)
    ship = (st["ship_x"], st["ship_y"], st["ship_x"] + 16, st["ship_y"] + 8)

    def on_shield(rect, on):
        hit = np.zeros(n, bool)
        for i in np.flatnonzero(on):
            for k in range(st["n_shields"][i]):
                for y in range(max(rect[1][i], st["shield_y"][i, k]), min(rect[3][i], st["shield_y"][i, k] + 18)):
                    bits = int(st["shield_rows"][i, k, y - st["shield_y"][i, k]])
                    for x in range(max(rect[0][i], st["shield_x"][i, k]), min(rect[2][i], st["shield_x"][i, k] + 16)):
                        hit[i] |= bool((bits >> (x - st["shield_x"][i, k])) & 1)
        return hit

    laser_shield, laser_ship = np.zeros(n, bool), np.zeros(n, bool)
    for q in range(8):
        on = st["n_enemy_lasers"] > q
        r = _si_rect(st["enemy_lasers"], q)
        laser_shield |= on_shield(r, on)
        laser_ship |= on & (st["ship_alive"] != 0) & _meet(r, ship)
    dying = (st["ship_alive"] == 0) & (st["ship_death_counter"] >= 0)
    return {"laser on shield": int(laser_shield.sum()), "laser on ship": int(laser_ship.sum()), "ship dying": int(dying.sum()),
            "ship laser on shield": int(on_shield(_si_rect(st["ship_laser"]), st["has_ship_laser"] != 0).sum()),
            "eight lasers": int((st["n_enemy_lasers"] == 8).sum())}


def si_off_grid(st):
    """every fifth env's formation off its grid (one enemy five pixels to the right): the state-reading rasteriser paints"""
    m = (np.arange(len(st)) % 5 == 2) & (st["n_enemies"] >= 2)
    st["enemies"]["x"][m, 1] += 5
    return st


OVERLAP_EDIT = {"breakout": breakout_overlaps, "amidar": amidar_overlaps, "space_invaders": si_overlaps, "gridworld": lambda st: st}
OVERLAP_COUNTS = {"breakout": breakout_overlap_counts, "amidar": amidar_overlap_counts, "space_invaders": si_overlap_counts,
                  "gridworld": lambda st: {}}
VARIANTS = {"breakout": ("canonical", "custom"), "space_invaders": ("records", "off_grid"), "amidar": ("plain",), "gridworld": ("plain",)}


@functools.lru_cache(maxsize=None)
def _prepared(game, name, variant, n, oracle_lib):
    """-> (config record or None, state records [n]): mid-game states under the palette with the overlaps written in.
    Breakout plays its own 400 frames under the palette's config, because the wall (14 rows, the bricks' colours) is part of the
    state; Amidar and SpaceInvaders start from support.donor_records, whose states hold nothing of the config's palette;
    GridWorld plays 9 frames from its reset."""
    pal = palette(game, name, n)
    with Engine(game, n, lib=oracle_lib) as o:
        cfg = None if game == "space_invaders" else palette_config(o, pal)
        if cfg is not None:
            o.set_config(cfg)
        o.seed(SEED)
        o.new_game()
        if game in ("amidar", "space_invaders"):
            rec = donor_records(game, oracle_lib)
            o.set_states_np(0, rec[np.arange(n) % len(rec)])
        else:
            for t in range(DONOR_FRAMES[game] or 9):
                o.step(synthetic_actions(game, n, t, seed=7), auto_reset=True)
        st = OVERLAP_EDIT[game](o.get_states_np())
    if game == "space_invaders":
        si_write_palette(st, pal)
        if variant == "off_grid":
            si_off_grid(st)
    if game == "breakout" and variant == "custom":
        breakout_custom_table(st, pal)
    st.flags.writeable = False
    return cfg, st


def prepared(game, name, variant, oracle_lib, n=N_ENVS):
    return _prepared(game, name, variant or VARIANTS[game][0], n, oracle_lib)


def palette_engines(game, name, variant, libs, oracle_lib, n=N_ENVS, options=(), first_env=0):
    """one engine per library under the palette's config, at the prepared states (env i of an n-env engine: record
    first_env + i); options: (option, value) pairs for every engine that is not the oracle's"""
    cfg, st = prepared(game, name, variant, oracle_lib)
    es = []
    for lib in libs:
        e = Engine(game, n, lib=lib)
        if lib is not oracle_lib:
            for opt, value in options:
                e.set_option(opt, value)
        if cfg is not None:
            e.set_config(cfg)
        e.seed(SEED)
        e.new_game()
        e.set_states_np(0, st[first_env:first_env + n])
        es.append(e)
    return es


# ---------------------------------------------------------------- which palette entries a frame shows

def shown_counts(game, pal, rgb):
    """role -> the number of envs whose RGB frame (uint8[n][H][W][3]) holds a pixel of the role's colour; a role whose entry is a
    tuple of colours (palette_in_force) counts an env that shows any of them"""
    n = len(rgb)
    flat = rgb.reshape(n, -1, 3).astype(np.uint32)
    key = flat[..., 0] | (flat[..., 1] << 8) | (flat[..., 2] << 16)
    out = {}
    for role, colors in pal.items():
        seen = np.zeros(n, bool)
        for c in (colors if isinstance(colors, tuple) else (colors,)):
            c = np.broadcast_to(np.asarray(c, np.uint32), (n, 4))
            want = c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16)
            seen |= (key == want[:, None]).any(axis=1)
        out[role] = int(seen.sum())
    return out


def palette_in_force(game, before, keep_wall):
    """what is to be on the screen once tbx_set_config has switched from the palette `before` to OTHER with no new game: the
    colours the config alone holds are OTHER's at once (Breakout bg / frame / paddle / ball, Amidar's six); what a running game
    holds in its state (Breakout's bricks, GridWorld's tiles and player) stays until that env's next game or wall, so those
    roles are met by the old colour or the new one"""
    other = palette(game, "OTHER")
    if game == "amidar":
        return dict(other)
    if game == "breakout":
        pal = {f: other[f] for f in BRK_FIELDS}
        for r in range(BRK_ROWS):
            role = "row%d" % r
            pal[role] = (before[role],) if keep_wall else (before[role], other[role])
        return pal
    return {role: (before[role], other[role]) for role in before}


DEFAULT_SI = {"ship": (35, 129, 59), "shield": (172, 80, 48), "ship_laser": (142, 142, 142), "enemy_laser": (255, 255, 255)}


def default_of(game, role, default_cfg):
    """the default palette's RGB for a role (the remap twin's target)"""
    if game == "space_invaders":
        return DEFAULT_SI["shield" if role.startswith("shield") else "enemy_laser" if role.startswith("enemy_laser") else role]
    if role.startswith("row"):
        c = default_cfg.row_colors[int(role[3:]) % 6]
    elif role.startswith("tile"):
        c = default_cfg.tiles[int(role[4:])].color
    else:
        c = getattr(default_cfg, role)
    return (c.r, c.g, c.b)


def other_config(e, game, keep_wall):
    """the config tbx_set_config switches to between calls: the OTHER palette; keep_wall (Breakout): only the four colours the
    config alone holds change, the rows -- whose colours the bricks on the screen carry in their state -- stay"""
    pal = dict(palette(game, "OTHER"))
    if game == "breakout" and keep_wall:
        cur = e.get_config()
        for r in range(BRK_ROWS):
            c = cur.row_colors[r]
            pal["row%d" % r] = np.asarray([c.r, c.g, c.b, c.a], np.uint8)
    return palette_config(e, pal)


def default_twin(game, name, variant, oracle_lib, n=N_ENVS):
    """(config, records, colour map): the prepared states under the DEFAULT palette -- the default config (Breakout: its six row
    colours repeated down the 14 rows) and, where the state carries colours, the default ones written over the palette's -- and
    the map role -> default RGB that takes a frame under the palette to the frame under the default one"""
    pal = palette(game, name, n)
    cfg, st = prepared(game, name, variant, oracle_lib, n)
    st = st.copy()
    with Engine(game, 1, lib=oracle_lib) as d:
        dflt = d.get_config()
    rgb = {role: default_of(game, role, dflt) for role in pal}
    if game == "space_invaders":
        dpal = {role: np.broadcast_to(np.asarray(rgb[role] + (255,), np.uint8), (n, 4)) for role in pal}
        si_write_palette(st, dpal)
        return None, st, rgb
    new = _abi.CONFIG_TYPES[_abi.GAME_IDS[game]].from_buffer_copy(bytes(cfg))
    dpal = {role: np.asarray(rgb[role] + (255,), np.uint8) for role in pal}
    with Engine(game, 1, lib=oracle_lib) as d:
        d.set_config(new)
        new = palette_config(d, dpal)
    if game == "breakout":
        rows = np.stack([dpal["row%d" % r] for r in range(BRK_ROWS)])
        pick = st["bricks"]["row"] % BRK_ROWS if variant != "custom" else (st["bricks"]["row"] + st["bricks"]["col"]) % BRK_ROWS
        slot = np.arange(st["bricks"].shape[1])[None, :] < st["n_bricks"][:, None]
        for k, ch in enumerate("rgba"):
            st["bricks"]["color"][ch] = np.where(slot, rows[pick, k], st["bricks"]["color"][ch])
    if game == "gridworld":
        _put(st["player_color"], np.broadcast_to(dpal["player_color"], (n, 4)))
        for t in range(GW_TILES):
            _put(st["tiles"]["color"][:, t], np.broadcast_to(dpal["tile%d" % t], (n, 4)))
    return new, st, rgb
