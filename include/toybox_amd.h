/*
 * toybox_amd.h -- C-ABI boundary of the MI355X-native batched Toybox engine.
 *
 * What this replaces.  In the reference (toybox-rs/Toybox) every game-step call goes
 * through the Python module `ctoybox` (cffi over the Rust cdylib of ctoybox==0.5.0,
 * /root/reference/REQUIREMENTS.txt:12), one opaque pointer per env, one FFI call per
 * operation.  The call sites that define the contract are cited per entry point below
 * (paths relative to /root/reference).  This header is the batched, device-resident
 * replacement of that per-env FFI: one engine handle owns N envs of one game on one GPU.
 *
 * Conventions (all entry points):
 *   - return int: 0 = TBX_OK, <0 = error (never abort / throw across the ABI);
 *     tbx_last_error() returns an engine-owned message valid until the next call;
 *   - plain pointers and sizes only; buffers are caller-allocated;
 *   - "_host" arguments are host pointers (call is synchronous), "_dev" arguments are
 *     device (HBM) pointers (call is asynchronous on the given hipStream_t, passed as void*);
 *   - calls on one handle take effect in program order whatever streams they name: when an entry point uses another stream
 *     than the previous one did (the host-pointer forms run on an engine-owned non-blocking stream), the new stream first
 *     waits for an event recorded on the old one -- no tbx_sync is needed between the two API families.  STREAM LIFETIME: to
 *     record that event the library keeps the handle of the stream the LAST call named until the next call on the handle;
 *     a stream passed to a call must therefore stay alive until the next call on the handle has returned, or until
 *     tbx_sync(), which forgets it (so: tbx_sync, then hipStreamDestroy).  The engine-owned output buffers (TBX_BUF_*) keep their addresses and a result in
 *     them stays valid for whatever the caller queues on the stream of the call that produced it before its next call on the
 *     handle -- unless the pipelined mode is switched on (TBX_OPT_PIPELINE below), which double-buffers them;
 *   - a handle is not thread-safe; different handles may be used concurrently;
 *   - there is NO CPU fallback: tbx_create fails with TBX_E_NO_DEVICE when no gfx950
 *     device is visible.
 *
 * The POD structs below are the lossless per-env state/config records that the Python
 * host turns into the interventions JSON schema
 * (toybox/interventions/{core,breakout,amidar,space_invaders}.py) and back.
 */
#ifndef TOYBOX_AMD_H
#define TOYBOX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ constants */

#define TBX_ABI_VERSION 1

#define TBX_GAME_BREAKOUT       0
#define TBX_GAME_AMIDAR         1
#define TBX_GAME_SPACE_INVADERS 2
#define TBX_GAME_GRIDWORLD      3   /* toybox/envs/atari/gridworld.py:8-13; not gym-registered by the reference */
#define TBX_NUM_GAMES           4

#define TBX_OK            0
#define TBX_E_INVALID    -1   /* bad argument (range, NULL, size mismatch)          */
#define TBX_E_NO_DEVICE  -2   /* no usable gfx950 device / HIP runtime error        */
#define TBX_E_NOMEM      -3
#define TBX_E_UNSUPPORTED -4  /* state/config outside what the device engine holds  */
#define TBX_E_ACTION     -5   /* an illegal ALE action id was seen (treated as NOOP) */
#define TBX_E_NEEDS_RESET -6  /* agent layer: an env was stepped although its game had ended inside EpisodicLifeEnv's no-op
                                 step -- where bench.Monitor raises "Tried to step environment that needs reset"
                                 (baselines/bench/monitor.py:52-53).  The step is carried out as the wrapper stack does
                                 without a Monitor (the finished game reports done at once and is reset). */

/* Input buttons bitmask == ctoybox.Input fields
 * (scripts/utils/test_games.py:13, test/interventions/test_breakout_interventions.py:12-15). */
#define TBX_BTN_LEFT    1u
#define TBX_BTN_RIGHT   2u
#define TBX_BTN_UP      4u
#define TBX_BTN_DOWN    8u
#define TBX_BTN_BUTTON1 16u
#define TBX_BTN_BUTTON2 32u

/* tbx_step flags */
#define TBX_STEP_AUTO_RESET 1u  /* VecEnv semantics: a done env is reset inside the step
                                   (baselines/common/vec_env/dummy_vec_env.py:51-54) */

/* device buffers addressable with tbx_device_buffer() */
#define TBX_BUF_REWARD  0   /* int32[N]  max(score - prev_score, 0) of the last step (envs/atari/base.py:136-138) */
#define TBX_BUF_DONE    1   /* uint8[N]  lives <= 0 after the last step (envs/atari/base.py:25-27,142)          */
#define TBX_BUF_LIVES   2   /* int32[N]  (pre-reset value when auto-reset fired)                                */
#define TBX_BUF_SCORE   3   /* int32[N]  (pre-reset value when auto-reset fired)                                */
#define TBX_BUF_FRAME   4   /* uint8[N,H,W,C] the last frame rasterised into an engine-owned buffer -- see below   */
#define TBX_BUF_PACKED  5   /* uint64[N] {reward:i32, done:u8, lives:u8, pad:u16} record for the multi-GPU gather */

/* What TBX_BUF_FRAME names, and how many bytes tbx_device_buffer reports for it.
 *   - After a call that rasterises every env into an engine-owned buffer -- tbx_render_device(out_dev = NULL),
 *     tbx_render_step_synthetic(out_dev = NULL), tbx_step_begin with a frame, and the host-pointer tbx_render, which paints there and
 *     copies out of it -- the id names the frame of that call, in that call's channel count.
 *   - After tbx_rollout_synthetic it names the chunk's LAST frame (frame k - 1: the state before the chunk's last step), in whichever
 *     form the chunk ran.
 *   - Every other call leaves the id as it was: calls that rasterise into a caller's buffer (tbx_render_device / tbx_render_step_synthetic
 *     with out_dev != NULL, tbx_render_env, tbx_step1_frame), steps, new games, state writes, edits.
 *   - The size reported is that of the frame the id names, N * H * W * channels of the call that produced it -- never the capacity of
 *     the allocation behind it (a gray frame after an RGBA one reports the gray size).  Before the first such call: NULL, 0 bytes.
 * The address may change with every such call (pipelined mode, overlapped fused launches, chunks): ask again after each.
 * TBX_BUF_ROLLOUT_FRAMES / TBX_BUF_ROLLOUT_PACKED keep the last chunk's k frames and k rows of records until the next chunk, whatever
 * is called in between (rows that ARE a record ring: until that ring is opened again, K steps later). */

/* RGBA colour, memory order r,g,b,a (interventions/core.py:179-187) */
typedef struct tbx_color { uint8_t r, g, b, a; } tbx_color_t;

/* ------------------------------------------------------------------ Breakout POD */

#define TBX_BRK_MAX_BALLS    4
#define TBX_BRK_COLS         18
#define TBX_BRK_MAX_ROWS     14
#define TBX_BRK_MAX_BRICKS   256   /* >= 18 * 14 */
#define TBX_BRK_MAX_STARTS   8
#define TBX_BRK_MAX_SEGMENTS 16

/* Breakout world (pixels == world units).  Anchored on the golden dump
 * toybox/interventions/defaults/breakout_state_default.json: bricks at (12+12c, 43+4r),
 * paddle (120,143), 18 columns => field x in [12,228). */
#define TBX_BRK_W            240
#define TBX_BRK_H            160
#define TBX_BRK_LEFT         12.0
#define TBX_BRK_RIGHT        228.0
#define TBX_BRK_TOP          25.0
#define TBX_BRK_BOTTOM       160.0
#define TBX_BRK_WALL_Y0      13
#define TBX_BRK_BRICK_Y0     43.0
#define TBX_BRK_BRICK_W      12.0
#define TBX_BRK_BRICK_H      4.0
#define TBX_BRK_PADDLE_H     3.0

typedef struct tbx_breakout_config {
    uint64_t rand[2];                 /* simulator RNG == config_to_json()['rand']['state'] */
    int32_t  start_lives;
    int32_t  n_rows;                  /* len(row_scores) == len(row_colors) */
    int32_t  row_scores[TBX_BRK_MAX_ROWS];
    tbx_color_t row_colors[TBX_BRK_MAX_ROWS];
    int32_t  ball_speed_row_depth;
    int32_t  n_starts;
    double   ball_speed_slow, ball_speed_fast;
    double   start_x[TBX_BRK_MAX_STARTS], start_y[TBX_BRK_MAX_STARTS];
    double   start_angle_deg[TBX_BRK_MAX_STARTS];
    /* host-evaluated trig (libm), so that no transcendental runs on the device:
       start_dir = (cos a, sin a) of start_angle_deg */
    double   start_dir_x[TBX_BRK_MAX_STARTS], start_dir_y[TBX_BRK_MAX_STARTS];
    int32_t  paddle_discrete_segments;   /* 1..16 */
    int32_t  _pad0;
    /* paddle_dir[i] = (cos a_i, -sin a_i), a_i = 150 - i*120/(S-1) degrees (S==1: 90) */
    double   paddle_dir_x[TBX_BRK_MAX_SEGMENTS], paddle_dir_y[TBX_BRK_MAX_SEGMENTS];
    tbx_color_t bg_color, frame_color, paddle_color, ball_color;
} tbx_breakout_config_t;

typedef struct tbx_brick {
    double   x, y, w, h;              /* position, size */
    int32_t  points, depth, row, col;
    tbx_color_t color;
    uint8_t  alive, destructible, _pad[2];
} tbx_brick_t;

typedef struct tbx_breakout_state {
    uint64_t rand[2];
    int32_t  score, lives, level;
    uint8_t  is_dead, reset, _pad0[2];
    double   paddle_x, paddle_y, paddle_vx, paddle_vy;
    double   paddle_width, paddle_speed, ball_radius;
    int32_t  n_balls, n_bricks;
    double   ball_x[TBX_BRK_MAX_BALLS], ball_y[TBX_BRK_MAX_BALLS];
    double   ball_vx[TBX_BRK_MAX_BALLS], ball_vy[TBX_BRK_MAX_BALLS];
    tbx_brick_t bricks[TBX_BRK_MAX_BRICKS];
} tbx_breakout_state_t;

/* ------------------------------------------------------------------ SpaceInvaders POD */

#define TBX_SI_W            320
#define TBX_SI_H            210
#define TBX_SI_COLS         6
#define TBX_SI_MAX_ROWS     10
#define TBX_SI_MAX_ENEMIES  64    /* one lane per enemy; 6 x 10 = 60 */
#define TBX_SI_MAX_SHIELDS  3
#define TBX_SI_SHIELD_W     16
#define TBX_SI_SHIELD_H     18
#define TBX_SI_MAX_LASERS   8

/* interventions/core.py:125-135 Direction.directions order */
#define TBX_DIR_UP    0
#define TBX_DIR_DOWN  1
#define TBX_DIR_LEFT  2
#define TBX_DIR_RIGHT 3

typedef struct tbx_si_config {
    uint64_t rand[2];
    double   jitter;                  /* probability of a random (vs player-targeted) firing column */
    int32_t  start_lives, n_rows, n_shields;
    int32_t  enemy_protocol;          /* 0 = "TargetPlayer" */
    int32_t  row_scores[TBX_SI_MAX_ROWS];
    int32_t  shield_x[TBX_SI_MAX_SHIELDS], shield_y[TBX_SI_MAX_SHIELDS];
} tbx_si_config_t;

typedef struct tbx_si_laser {
    int32_t  x, y, w, h, t, movement, speed;
    tbx_color_t color;
} tbx_si_laser_t;

typedef struct tbx_si_enemy {
    int32_t  x, y, row, col, id, points;
    int32_t  death_counter;           /* -1 == None */
    uint8_t  alive, _pad[3];
} tbx_si_enemy_t;

typedef struct tbx_si_state {
    uint64_t rand[2];
    int32_t  score, lives, level;
    int32_t  life_display_timer, enemy_shot_delay;
    int32_t  n_enemies, n_enemy_lasers, has_ship_laser;
    int32_t  ship_x, ship_y, ship_w, ship_h, ship_speed;
    int32_t  ship_death_counter;      /* -1 == None */
    tbx_color_t ship_color;
    uint8_t  ship_alive, ship_death_hit_1, _pad0[2];
    int32_t  ufo_x, ufo_y, ufo_appearance_counter;
    int32_t  ufo_death_counter;       /* -1 == None */
    int32_t  move_counter, move_dir;
    uint8_t  visual_orientation, _pad1[3];
    int32_t  n_shields;
    int32_t  shield_x[TBX_SI_MAX_SHIELDS], shield_y[TBX_SI_MAX_SHIELDS];
    tbx_color_t shield_color[TBX_SI_MAX_SHIELDS];
    uint16_t shield_rows[TBX_SI_MAX_SHIELDS][TBX_SI_SHIELD_H];   /* bit c of row r = pixel (c,r) present */
    tbx_si_laser_t ship_laser;
    tbx_si_laser_t enemy_lasers[TBX_SI_MAX_LASERS];
    tbx_si_enemy_t enemies[TBX_SI_MAX_ENEMIES];
} tbx_si_state_t;

/* ------------------------------------------------------------------ Amidar POD */

#define TBX_AMI_W             160
#define TBX_AMI_H             250
#define TBX_AMI_BOARD_W       32
#define TBX_AMI_BOARD_H       31
#define TBX_AMI_MAX_ENEMIES   8
#define TBX_AMI_MAX_BOXES     64
#define TBX_AMI_MAX_HISTORY   16
#define TBX_AMI_MAX_CHASE_J   8
#define TBX_AMI_TILE_WX       64    /* world units per tile: player_start {31,15} <-> position {1984,1200} in the goldens */
#define TBX_AMI_TILE_WY       80

/* tile tags (interventions/amidar.py:55-59) */
#define TBX_TILE_EMPTY        0
#define TBX_TILE_UNPAINTED    1
#define TBX_TILE_PAINTED      2
#define TBX_TILE_CHASE_MARKER 3

/* movement protocols (interventions/amidar.py:101-112) */
#define TBX_AI_PLAYER          0
#define TBX_AI_LOOKUP          1   /* EnemyLookupAI     {next, default_route_index}                       */
#define TBX_AI_PERIMETER       2   /* EnemyPerimeterAI  {start}                                           */
#define TBX_AI_AMIDAR          3   /* EnemyAmidarMvmt   {vert, horiz, start_vert, start_horiz, start}     */
#define TBX_AI_TARGET_PLAYER   4   /* EnemyTargetPlayer {start, start_dir, vision_distance, dir, player_seen} */
#define TBX_AI_RANDOM          5   /* EnemyRandomMvmt   {start, start_dir, dir}                           */

typedef struct tbx_amidar_ai {
    int32_t kind;
    int32_t next, default_route_index;
    int32_t start_tx, start_ty;
    int32_t vert, horiz, start_vert, start_horiz;
    int32_t start_dir, dir;
    int32_t vision_distance;
    int32_t seen_tx, seen_ty;          /* player_seen; -1,-1 == None */
} tbx_amidar_ai_t;

typedef struct tbx_amidar_mover {
    int32_t x, y, speed;
    int32_t step_tx, step_ty;          /* step; -1,-1 == None */
    int32_t n_history;
    int32_t history[TBX_AMI_MAX_HISTORY];
    int32_t caught;
    tbx_amidar_ai_t ai;
} tbx_amidar_mover_t;

typedef struct tbx_amidar_box {
    int32_t tl_tx, tl_ty, br_tx, br_ty;
    uint8_t painted, triggers_chase, _pad[2];
} tbx_amidar_box_t;

typedef struct tbx_amidar_config {
    uint64_t rand[2];
    int32_t  start_lives, start_jumps, jump_time, chase_time, box_bonus, chase_score_bonus;
    int32_t  player_start_tx, player_start_ty;
    int32_t  n_enemies;
    uint8_t  render_images, default_board_bugs, _pad0[2];
    tbx_amidar_ai_t enemies[TBX_AMI_MAX_ENEMIES];
    tbx_color_t bg_color, player_color, unpainted_color, painted_color, enemy_color, inner_painted_color;
    uint8_t  board[TBX_AMI_BOARD_H][TBX_AMI_BOARD_W];   /* tile tags */
} tbx_amidar_config_t;

typedef struct tbx_amidar_state {
    uint64_t rand[2];
    int32_t  score, lives, level;
    int32_t  jumps, jump_timer, chase_timer;
    int32_t  n_enemies, n_boxes, n_chase_junctions;
    int32_t  chase_junctions[TBX_AMI_MAX_CHASE_J];
    tbx_amidar_mover_t player;
    tbx_amidar_mover_t enemies[TBX_AMI_MAX_ENEMIES];
    tbx_amidar_box_t boxes[TBX_AMI_MAX_BOXES];
    uint8_t  tiles[TBX_AMI_BOARD_H][TBX_AMI_BOARD_W];
} tbx_amidar_state_t;

/* ------------------------------------------------------------------ GridWorld POD */

/* The reference only ships this game's two golden dumps (toybox/interventions/defaults/gridworld_{config,state}_default.json)
 * and the env class envs/atari/gridworld.py:8-13; the records below hold exactly the fields of those dumps.  The rules
 * and the picture are this repo's own (SPEC.md, "GridWorld"): a fixed 160x128 frame divided into
 * game_size cells of floor(160/w) x floor(128/h) pixels. */
#define TBX_GW_W          160
#define TBX_GW_H          128
#define TBX_GW_MAX_DIM    32    /* game_size <= 32 x 32; grid rows have a stride of 32 cells */
#define TBX_GW_MAX_TILES  16

typedef struct tbx_gw_tile {
    tbx_color_t color;
    int32_t  reward;
    uint8_t  goal, walkable, _pad[2];
} tbx_gw_tile_t;

typedef struct tbx_gridworld_config {
    uint64_t rand[2];                 /* simulator RNG words (kept for a uniform seeding surface; the rules draw nothing) */
    int32_t  width, height;           /* "game_size" */
    int32_t  n_tiles;
    int32_t  player_start_x, player_start_y;
    int32_t  reward_becomes;          /* tile index a collected reward cell turns into */
    tbx_color_t player_color;
    uint8_t  tile_keys[TBX_GW_MAX_TILES];   /* the one-character names the JSON config gives the tiles */
    tbx_gw_tile_t tiles[TBX_GW_MAX_TILES];
    uint8_t  grid[TBX_GW_MAX_DIM * TBX_GW_MAX_DIM];   /* tile index of cell (x, y) at [y * 32 + x] */
} tbx_gridworld_config_t;

typedef struct tbx_gridworld_state {
    int32_t  score, game_over;
    int32_t  player_x, player_y;
    int32_t  reward_becomes;
    int32_t  width, height, n_tiles;
    tbx_color_t player_color;
    tbx_gw_tile_t tiles[TBX_GW_MAX_TILES];
    uint8_t  grid[TBX_GW_MAX_DIM * TBX_GW_MAX_DIM];
} tbx_gridworld_state_t;

/* ------------------------------------------------------------------ engine */

typedef struct tbx_engine tbx_engine;

/* ABI version of the loaded library. */
int tbx_abi_version(void);

/* Last error text; engine may be NULL (errors of tbx_create). */
const char* tbx_last_error(const tbx_engine* engine);

/* Static game metadata.
 * replaces Toybox.get_height/get_width (envs/atari/base.py:64-65) and
 * Toybox.get_legal_action_set (envs/atari/base.py:57, test/benchmark.py:48). */
int tbx_frame_dims(int game, int* height, int* width);
int tbx_legal_actions(int game, int32_t* out_actions, int cap);   /* returns count or <0 */
/* ALE action id (envs/atari/constants.py:16-35) -> TBX_BTN_* mask; <0 if out of 0..17. */
int tbx_ale_action_to_buttons(int ale_action);
size_t tbx_state_size(int game);
size_t tbx_config_size(int game);

/* Which device an engine drives: one process per GPU shards the batch (cmd_util.py:31 gives every worker its own rank and seed),
 * and a benchmark line has to show that N ranks drove N DISTINCT GPUs -- bench.py gathers one of these per rank and refuses
 * (rc 7) when two ranks of an RCCL run report the same PCI address. */
typedef struct tbx_device_identity {
    int32_t  ordinal;                 /* HIP device ordinal inside this process (HIP_VISIBLE_DEVICES applied) */
    int32_t  pci_domain, pci_bus, pci_device;
    uint64_t total_memory;            /* bytes of device memory */
    int32_t  compute_units;
    int32_t  _pad;
    char     arch[64];                /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
    char     name[64];                /* marketing name */
} tbx_device_identity_t;
int tbx_device_identity(tbx_engine* engine, tbx_device_identity_t* out);

/* Create an engine of n_envs envs of one game on HIP device `device`.
 * config_pod may be NULL (game defaults == interventions/defaults/<game>_config_default.json).
 * Every env's simulator RNG starts at config.rand; all envs are then given a first game.
 * replaces ctoybox.Toybox(name) (envs/atari/breakout.py:8, interventions/breakout.py:38). */
int tbx_create(int game, int n_envs, int device, const void* config_pod, size_t config_size,
               tbx_engine** out_engine);
int tbx_destroy(tbx_engine* engine);
int tbx_num_envs(const tbx_engine* engine);
int tbx_game(const tbx_engine* engine);

/* Re-seed the simulator RNG: env >= 0 -> that env gets `seed`; env == -1 -> env i gets seed+i.
 * Takes effect at the next new game, as in the reference (envs/atari/base.py:95-97).
 * replaces Toybox.set_seed (envs/atari/base.py:95, scripts/utils/test_games.py:30). */
int tbx_seed(tbx_engine* engine, int env, uint32_t seed);
/* Per-env seeds in one upload + one launch: env i gets seeds_host[i].  This is how a vectorised env applies the reference's
 * per-worker derivation seed2_i = hash_seed(seed + rank_i + 1) % 2**31 (envs/atari/base.py:84-98 under
 * baselines/common/cmd_util.py:31) without N calls. */
int tbx_seed_array(tbx_engine* engine, const uint32_t* seeds_host);
int tbx_get_sim_rng(tbx_engine* engine, int env, uint64_t out_state[2]);
int tbx_set_sim_rng(tbx_engine* engine, int env, const uint64_t state[2]);

/* Start a new game in the envs whose mask byte is non-zero (mask_host == NULL: all).
 * replaces Toybox.new_game (envs/atari/base.py:97,153; test/benchmark.py:54). */
int tbx_new_game(tbx_engine* engine, const uint8_t* mask_host);

/* One game frame for every env.  actions are ALE action ids.  Host-pointer form: synchronous,
 * any output pointer may be NULL.
 * replaces Toybox.apply_ale_action + get_score/get_lives/game_over
 * (envs/atari/base.py:126,136,142,145; test/benchmark.py:52-56). */
int tbx_step(tbx_engine* engine, const int32_t* ale_actions_host, uint32_t flags,
             int32_t* reward_host, uint8_t* done_host, int32_t* lives_host, int32_t* score_host);
/* Device-pointer form: asynchronous on `stream`; results land in the TBX_BUF_* buffers. */
int tbx_step_device(tbx_engine* engine, const int32_t* ale_actions_dev, uint32_t flags, void* stream);
/* Same, with the actions generated on the device: env e at time t plays
 * legal[ splitmix64(action_seed ^ (e_global << 32) ^ t) mod n_legal ], e_global = env_offset + e.
 * (Such a step depends on nothing a rasteriser produces: with TBX_OPT_PIPELINE it runs beside the previous frame's
 * tbx_render_device.) */
int tbx_step_synthetic(tbx_engine* engine, uint64_t action_seed, uint64_t t, uint64_t env_offset,
                       uint32_t flags, void* stream);
/* One frame for ONE env by ALE action id, with the outputs of tbx_step: out[4] = {reward, done, lives, score} (may be NULL).
 * replaces the reference's per-frame call sequence Toybox.apply_ale_action + get_score / get_lives / game_over on a single
 * env (envs/atari/base.py:126-145, test/benchmark.py:50-56).  On a ONE-env engine this call does not launch anything: a
 * resident kernel (one wave) waits on a mailbox in host-coherent pinned memory, steps env 0 and posts the outputs back --
 * two PCIe hops per frame.  The wave leaves after 50 ms without a request and every other entry point of the handle stops it
 * first, so the two never run side by side.  On batch engines it is tbx_apply_input plus a read-back of the outputs
 * (TBX_OPT_RESIDENT_STEP = 0 forces that second form everywhere). */
int tbx_step1(tbx_engine* engine, int env, int32_t ale_action, uint32_t flags, int32_t out[4]);
/* The same step plus the env's picture, i.e. the whole of ToyboxBaseEnv.step (apply_ale_action, then get_state / get_rgb_frame:
 * envs/atari/base.py:126,109,131-145; the env.step() arm of test/benchmark.py:83-97).  *frame_host receives the address of an
 * engine-owned buffer of H * W * channels bytes (channels 1, 3 or 4) that holds the frame of the state AFTER the step and stays
 * valid until the next call on the handle.  On a one-env engine the resident kernel rasterises straight into that buffer
 * (pinned host memory mapped into the device): still no launch, no copy, no synchronisation.  Elsewhere it is tbx_step1
 * followed by tbx_render_env into the same buffer. */
int tbx_step1_frame(tbx_engine* engine, int env, int32_t ale_action, uint32_t flags, int channels, int32_t out[4],
                    const uint8_t** frame_host);
/* One frame for one env with a raw button mask.
 * replaces Toybox.apply_action(Input) (scripts/utils/test_games.py:13). */
int tbx_apply_input(tbx_engine* engine, int env, uint32_t buttons);

/* Scalar reads for every env (any pointer may be NULL).
 * replaces get_score/get_lives/get_level/game_over (envs/atari/base.py:20-27). */
int tbx_get_scalars(tbx_engine* engine, int32_t* score_host, int32_t* lives_host,
                    int32_t* level_host, uint8_t* game_over_host);

/* Rasterise every env's current state: out[N][H][W][channels], channels 1 (gray), 3 (RGB), 4 (RGBA).
 * replaces Toybox.get_state / get_rgb_frame (envs/atari/base.py:109,164). */
int tbx_render(tbx_engine* engine, uint8_t* out_host, int channels);   /* (paints the engine-owned buffer: TBX_BUF_FRAME names this frame) */
/* out_dev == NULL renders into the engine-owned TBX_BUF_FRAME buffer. */
int tbx_render_device(tbx_engine* engine, uint8_t* out_dev, int channels, void* stream);
/* The random-rollout loop body as ONE call: rasterise every env's CURRENT state into out_dev (NULL: TBX_BUF_FRAME) and step
 * every env one frame with device-generated actions (the rule of tbx_step_synthetic) -- i.e. tbx_render_device followed by
 * tbx_step_synthetic, asynchronous on `stream`, same results bit for bit: the frame shows the state BEFORE the step, the
 * TBX_BUF_* outputs and the state are the step's.  Where the rasteriser reads step-written render records (Breakout with the
 * canonical wall; RGB / RGBA) both halves are ONE launch: the step's few blocks ride in front of the rasteriser's, write the
 * other records buffer and hide in the launch's ramp-up, so a loop of these calls runs like a render-only loop -- no kernel
 * boundary per frame, no rasteriser that starts in lockstep behind a short kernel (8 192 envs + gather, the per-GPU share of
 * the strong-scaled headline batch: see DESIGN.md section 6).  Only a loop whose actions do not depend on the frame can use
 * it (the north star's random-action rollouts; replaces the loop body of test/benchmark.py:50-56 plus the frame);
 * a policy-driven loop calls tbx_step_device and tbx_render_device.  Everywhere else it is the two launches in stream order. */
int tbx_render_step_synthetic(tbx_engine* engine, uint8_t* out_dev, int channels, uint64_t action_seed, uint64_t t,
                              uint64_t env_offset, uint32_t flags, void* stream);
/* A rollout CHUNK: k consecutive tbx_render_step_synthetic calls (t = t0 .. t0 + k - 1; with a K-step record ring each followed by
 * tbx_gather) as one call -- what the reference's learners consume is a K-step rollout anyway (A2C nsteps = 5, PPO2 128:
 * baselines/baselines/a2c/runner.py:16, ppo2/ppo2.py:103).  Results bit for bit those of the k single calls:
 *   TBX_BUF_ROLLOUT_FRAMES  uint8[k][N][H][W][channels]: frame j shows the state BEFORE step t0 + j;
 *   TBX_BUF_ROLLOUT_PACKED  uint64[k][stride] step records (reward, done, lives) of step j in row j -- with a K-step record ring
 *                           in force (TBX_OPT_GATHER_EVERY = K; k must equal K and the ring must be empty) the rows ARE the ring
 *                           (stride = records_per_rank) and the call queues the collective itself: no tbx_gather for these steps;
 *                           otherwise an engine-owned array with stride = N;
 *   TBX_BUF_REWARD / DONE / LIVES / SCORE / PACKED and the state: those of the chunk's LAST step; TBX_BUF_FRAME: its last frame.
 * Where the rasteriser reads step-written records (Breakout, canonical wall, RGB / RGBA; TBX_OPT_ROLLOUT_CHUNKS) a chunk is ONE step
 * launch on an internal stream -- every env k frames with its state in registers, writing k render records, the k step records and
 * the state once -- and rasteriser launches that depend on that step launch alone, in one of two forms: ONE launch for the chunk's
 * k x N frames (the records and the frames of a chunk lie one behind the other), chunk behind chunk on a second internal stream --
 * a render-only loop of launches k times as long as a frame's --, or k launches of one frame each that alternate between two
 * internal streams and overlap freely.  Either way the next chunk's step launch runs beside this chunk's rasterisers (a whole
 * chunk ahead of its own), and with a ring the collective waits for the step launch only.  That is what N
 * worker processes stepping independently of each other give the reference (baselines/baselines/common/vec_env/subproc_vec_env.py:49-74),
 * and what the per-GPU share of a strong-scaled batch (8 192 envs) loses to ramp-up and tail between launches in stream order.
 * Contract in that form: as for overlapped fused launches (TBX_OPT_FUSED_OVERLAP) -- two chunk buffers alternate; ask
 * tbx_device_buffer after the call for what is to be read, and it is that call which makes `stream` wait for the chunk (lazy
 * join); results stay valid for readers queued on `stream` before the next chunk.  Everywhere else (other games, gray frames,
 * one collective per step, the option off) the call is the k single calls in stream order. */
int tbx_rollout_synthetic(tbx_engine* engine, int channels, uint64_t action_seed, uint64_t t0, int k, uint64_t env_offset,
                          uint32_t flags, void* stream);
#define TBX_BUF_ROLLOUT_FRAMES 15
#define TBX_BUF_ROLLOUT_PACKED 16
/* Rasterise one env (host pointer, synchronous). */
int tbx_render_env(tbx_engine* engine, int env, uint8_t* out_host, int channels);

/* Per-env lossless state record (tbx_<game>_state_t).
 * replaces Toybox.to_state_json / write_state_json (interventions/base.py:391,406).
 * tbx_set_state stores the CANONICAL form of the record and tbx_get_state returns it: slots beyond the counts (balls,
 * bricks, enemies, lasers, shields, boxes) zeroed, flags 0 / 1, an absent counter -1, direction fields two bits wide,
 * Amidar tile tags two bits wide, paddings zero.  Records a game produces itself are canonical already.
 * Capacity: counts beyond the fixed tables (TBX_*_MAX_*) and SpaceInvaders enemies whose row / col leave 0..255 or whose id
 * leaves 0..65535 (the device packs the three into one word) are refused with TBX_E_UNSUPPORTED, never truncated. */
int tbx_get_state(tbx_engine* engine, int env, void* pod_out, size_t size);
int tbx_set_state(tbx_engine* engine, int env, const void* pod, size_t size);
/* Batched forms for intervention sweeps over many envs: `count` consecutive records of
 * record_size bytes for envs [first_env, first_env + count), one pack/unpack launch and one copy. */
int tbx_get_states(tbx_engine* engine, int first_env, int count, void* pods_out, size_t record_size);
int tbx_set_states(tbx_engine* engine, int first_env, int count, const void* pods, size_t record_size);
/* Batch-wide config record (tbx_<game>_config_t).  `rand` is env 0's simulator RNG on get.  On set, a `rand` equal to
 * env 0's current simulator RNG (i.e. the caller did not edit it) leaves every env's simulator RNG untouched -- a config
 * edit must not put a seeded batch onto one random stream; any other value is written to every env.  For a one-env engine
 * both cases coincide with the reference.  Does not start a new game: what a running game holds in its state record stays as it is
 * until that env's next game -- Breakout's bricks keep the colour and the points they were made with, GridWorld's tiles and player
 * theirs -- while the colours only the config holds (Breakout bg / frame / paddle / ball, Amidar's six) change with the next picture.
 * A Breakout config with other rows, row scores or row colours takes a running device engine to its per-env brick tables, as a
 * written non-canonical brick does: every result stays the reference's, at the wave-per-env step's and the generic observation
 * path's rates, and -- as on any engine with written bricks -- the agent layer's episodic-life / fire-reset / no-op-reset wrappers
 * are not available there: tbx_agent_step* and tbx_agent_reset return TBX_E_UNSUPPORTED and change nothing.  A tbx_new_game for
 * every env (mask NULL; write_config_json + new_game, the reference's way to another wall) brings the engine back to the
 * canonical wall, with or without an agent layer.
 * replaces Toybox.config_to_json / write_config_json (interventions/base.py:390,402). */
int tbx_get_config(tbx_engine* engine, void* pod_out, size_t size);
int tbx_set_config(tbx_engine* engine, const void* pod, size_t size);

/* Integer state queries.  Amidar: TBX_QUERY_TILE_TO_WORLD {tx,ty} -> {x,y}, TBX_QUERY_WORLD_TO_TILE {x,y} -> {tx,ty}.
 * replaces Toybox.query_state_json('tile_to_world' / 'world_to_tile') (interventions/amidar.py:510,518). */
#define TBX_QUERY_TILE_TO_WORLD 1
#define TBX_QUERY_WORLD_TO_TILE 2
int tbx_query(tbx_engine* engine, int env, int query_id, const int32_t* args, int n_args, int32_t* out, int n_out);

/* ------------------------------------------------------------------ batched interventions on the device
 * The reference's per-game intervention classes are helper methods over ONE env's decoded JSON state
 * (toybox/interventions/breakout.py:303-429, amidar.py:360-615, space_invaders.py:165-176).  Their batched forms here act on
 * the struct-of-arrays state in HBM directly -- one kernel over every selected env, no state record leaves the device:
 *   tbx_edit    a field write ("add_channel", "set_mode", "set_tile_tag", "set_enemy_protocol", ...) in the envs whose mask
 *               byte is non-zero (mask NULL: every env);
 *   tbx_reduce  a per-env feature ("num_bricks_remaining", "channel_count", "player_enemy_distances", ...) as
 *               out[N][tbx_reduce_width(game, query)] doubles (integers are exact in binary64; Breakout's positions are
 *               binary64 anyway); entries that do not exist (a fifth enemy of four, a tile outside the board) read -1.
 * args: up to TBX_EDIT_MAX_ARGS doubles, the same for every env (per_env = 0) or one row per env, args[N][n_args]
 * (per_env = 1: a sweep in which env i gets its own column, tile, timer ...).  The "_device" forms take device pointers for
 * mask / per-env args / out and are asynchronous on `stream`; args with per_env = 0 are always a host pointer.
 * Helpers that take a Python predicate have a MASK form here: find_brick(pred) -> TBX_QUERY_BRK_FIND_BRICK over a bit mask of
 * brick indices (the host evaluates the predicate once over the brick table, whose attributes other than `alive` are the same
 * in every env) plus the wanted `alive`; filter_tiles(pred) for predicates on the tag -> TBX_QUERY_AMI_TILES_MASK over a mask
 * of tags.  Helpers that sample with Python's `random` (get_random_tile, get_random_track_position, set_player_random_start,
 * get_random_dir_for_tile: amidar.py:360-399,541-583) have COUNTER-RNG forms: draw number k of env e is
 * splitmix64(seed ^ (e_global << 32) ^ k) -- the rule of tbx_step_synthetic -- taken modulo the number of candidates, and
 * the candidates are exactly the elements the reference's predicate accepts, in the order its loops visit them (tiles row by
 * row, directions Up, Down, Left, Right).  Not `random`-compatible (the reference's draws depend on Python's global
 * Mersenne Twister and on rejection sampling); uniform over the same candidate set, reproducible, and independent of the batch
 * layout.  Config-level helpers (set_jitter, add_row) go through tbx_set_config like the reference's dirty_config path. */
#define TBX_EDIT_MAX_ARGS 16
/* every game -- `intervention.game.lives = v` (interventions/space_invaders.py:199, test_breakout_interventions.py) */
#define TBX_EDIT_SET_LIVES          1   /* {lives} */
#define TBX_EDIT_SET_SCORE          2   /* {score} */
#define TBX_EDIT_SET_LEVEL          3   /* {level} */
/* Breakout (interventions/breakout.py) */
#define TBX_EDIT_BRK_COLUMN_ALIVE  10   /* {col, alive}: add_channel :392-396 (alive 0), fill_column :398-402 (alive 1) */
#define TBX_EDIT_BRK_ROW_ALIVE     11   /* {row, alive} */
#define TBX_EDIT_BRK_ALL_ALIVE     12   /* {alive}: clear_board :412-415 (alive 0) */
#define TBX_EDIT_BRK_BRICK_ALIVE   13   /* {brick index, alive} (test_breakout_interventions.py:48) */
#define TBX_EDIT_BRK_PADDLE        14   /* {x[, y]} paddle.position (get_paddle_position :379; test :111-118) */
#define TBX_EDIT_BRK_BALL          15   /* {ball, x, y, vx, vy} balls[ball] position and velocity (:365-377) */
/* Amidar (interventions/amidar.py) */
#define TBX_EDIT_AMI_TIMERS        20   /* {jump_timer, chase_timer}, -1 = leave: set_mode :402-416 */
#define TBX_EDIT_AMI_JUMPS         21   /* {jumps} (test_amidar_interventions.py:174) */
#define TBX_EDIT_AMI_TILE          22   /* {tx, ty, tag}: set_tile_tag :476-478 */
#define TBX_EDIT_AMI_ENEMY_AI      23   /* {enemy, the 14 fields of tbx_amidar_ai_t}: set_enemy_protocol :418-471 */
#define TBX_EDIT_AMI_PLAYER_TILE   24   /* {tx, ty}: player.position = tile_to_world(tile), the write of set_player_random_start :531-538 */
#define TBX_EDIT_AMI_PLAYER_RANDOM_START 25  /* {seed, draw, env_offset, min_enemy_distance}: set_player_random_start :541-548 -- the player goes
                                              * to the tile TBX_QUERY_AMI_RANDOM_TILE {seed, draw, env_offset, 15, min_enemy_distance} names
                                              * (ANY tag, as the reference draws it; no candidate: the env is left alone) */
/* SpaceInvaders (interventions/space_invaders.py) */
#define TBX_EDIT_SI_UFO_APPEARANCE 30   /* {appearance_counter}: remove_mothership :172-173 (-1) */
/* every game -- FORK: the selected envs become copies of other envs of the batch, on the device.  It replaces the reference's
 * to_state_json -> write_state_json onto a second Toybox (interventions/base.py:391-406) and the tbx_get_states -> host ->
 * tbx_set_states round trip, which leaves prev_score, the simulator RNG and the agent layer behind.
 *   args {src[, salt]}: the same for every env (one source fanned out) or one row per env; the mask selects the DESTINATIONS.
 *   Simultaneous assignment: every selected env i becomes a copy of env src_i AS IT WAS BEFORE THE CALL -- swaps, reversals,
 *   src_i == i and sources that are destinations themselves all work.
 *   Copied: the complete game state (every byte tbx_get_state reports, the game's own `rand` included) with its device-only
 *   mirrors (Breakout's per-env brick table in custom mode, Amidar's mover mirror, SpaceInvaders' formation origin), the
 *   simulator RNG and prev_score; and after tbx_agent_init the wrapper stack's per-env state: Monitor's return, length and
 *   needs_reset, EpisodicLifeEnv's lives and was_real_done, the episode counter behind the no-op rule, MaxAndSkipEnv's two
 *   buffer slots with their validity, the generic path's gray frames, and the observation -- the env's row of
 *   TBX_BUF_AGENT_OBS, of TBX_BUF_AGENT_PLANE and of EVERY slot of TBX_BUF_AGENT_RING (the ring's head is batch-wide and stays).
 *   The copy's next tbx_agent_step with the same action returns what the source's returns.
 *   Not copied: the outputs of the last step (TBX_BUF_REWARD .. TBX_BUF_PACKED, TBX_BUF_AGENT_REWARD .. EP_LENGTH), the gather
 *   ring, the batch-wide config, per-slot configuration (tbx_agent_set_noops counts, env_offset) and the engine-wide mode flags.
 *   salt (an integer below 2^32; absent or 0: none): every RNG word of the destination -- both words of the game's `rand` where
 *   the game has one, both of the simulator RNG -- becomes splitmix64(word ^ salt): the same fork point, fresh randomness.
 *   tbx_edit returns TBX_E_INVALID for a selected row whose src is outside 0 .. N-1 (it names the first such env and changes
 *   nothing); tbx_edit_device cannot see the rows: such an env is left untouched.
 *   The host form copies in one pass when no selected destination is another selected row's source; otherwise, and always in
 *   the device form, the rows are gathered into a scratch copy first (allocated on first use, as large as the copied arrays). */
#define TBX_EDIT_COPY_ENV          40   /* {src[, salt]} */
/* every game -- CHECKPOINTS: env states set aside on the device and taken up again later.  The fork branches inside the batch,
 * but every call steps every env, so no slot of the batch can hold a state still; a store of cells beside the batch can.  It
 * replaces to_state_json ... write_state_json LATER (interventions/base.py:391-406) for tree search, archives of start states
 * and "same state, K policies" sweeps, with nothing leaving HBM.
 *   TBX_EDIT_CHECKPOINT_SLOTS {slots}, tbx_edit only, mask NULL, per_env 0: makes the engine's checkpoint store -- `slots` >= 1
 *   planes of N cells, all empty; cell (slot, row) holds one env.  0 releases the store.  An existing store is released first
 *   (its contents are lost); on TBX_E_NOMEM the engine has no store.  tbx_edit_device returns TBX_E_INVALID for this op.
 *   tbx_destroy frees the store.
 *   TBX_EDIT_CHECKPOINT_SAVE {slot}, the same for every env or one row per env: every selected env i is written into cell
 *   (slot_i, i), which becomes valid.  Saved: exactly what TBX_EDIT_COPY_ENV copies (above).  A save changes nothing in the live
 *   engine -- step-written render records stay in force, so a rollout loop that saves every K steps keeps its record path.
 *   TBX_EDIT_CHECKPOINT_RESTORE {slot[, row[, salt]]}: every selected env i becomes the env stored in cell (slot_i, row_i); row
 *   absent or -1: the env's own row i.  salt as in the fork: every RNG word of the restored env becomes splitmix64(word ^ salt),
 *   0 or absent: none.  The env's next step with the same action returns what the saved env's next step returned.  What the
 *   fork does not copy stays as it is here too: the outputs of the last step (TBX_BUF_REWARD .. TBX_BUF_AGENT_EP_LENGTH), the
 *   gather ring, the batch-wide config, tbx_agent_set_noops counts and env_offset.  The plane ring is stored oldest plane first,
 *   so a restore at another ring head than the save's puts every plane where that head expects it.  Step-written render records
 *   are stale afterwards, as after any edit.
 *   Errors: tbx_edit checks first (a small kernel and an 8-byte read-back) and changes nothing on an error: TBX_E_INVALID, naming
 *   the first offending env, when there is no store, when a selected row names a slot outside 0 .. slots-1 or a row outside
 *   0 .. N-1, or when a restore names an empty cell.  tbx_edit_device cannot report: such an env is left untouched, on save and
 *   on restore, and the others go through.
 *   A store belongs to the set of per-env arrays that existed when it was made ({planes, row bytes} of each, in order).  When
 *   that set has changed -- Breakout left the canonical wall (its per-env brick table appeared), the generic path's gray frames
 *   were allocated, tbx_agent_init was called (again, with another geometry, stack or new_plane) -- SAVE and RESTORE return
 *   TBX_E_UNSUPPORTED and touch nothing until TBX_EDIT_CHECKPOINT_SLOTS makes a new store.  Restoring under a different
 *   batch-wide config is the caller's business, as with tbx_set_state. */
#define TBX_EDIT_CHECKPOINT_SLOTS   41  /* {slots} */
#define TBX_EDIT_CHECKPOINT_SAVE    42  /* {slot} */
#define TBX_EDIT_CHECKPOINT_RESTORE 43  /* {slot[, row[, salt]]} */

#define TBX_QUERY_BRK_BRICKS_REMAINING 110  /* -> 1  num_bricks_remaining :309-310 */
#define TBX_QUERY_BRK_NUM_BRICKS       111  /* -> 1  num_bricks :312-313 */
#define TBX_QUERY_BRK_COLUMN           112  /* {col} -> 32  alive flag of each brick with that col, in brick order (get_column :349-355) */
#define TBX_QUERY_BRK_ROW              113  /* {row} -> 32  the same by row (get_row :357-359, read as documented: the ith row) */
#define TBX_QUERY_BRK_IS_CHANNEL       114  /* {col} -> 1  the column has bricks and none is alive (is_channel :340-347) */
#define TBX_QUERY_BRK_CHANNEL_COUNT    115  /* {n_columns} -> 1  channel_count :361-366 */
#define TBX_QUERY_BRK_FIND_CHANNEL     116  /* {n_columns} -> 1  first channel column or -1 (find_channel :404-410) */
#define TBX_QUERY_BRK_PADDLE           117  /* -> 4  position x, y, velocity x, y (:379-383) */
#define TBX_QUERY_BRK_BALLS            118  /* -> 17 n_balls, x[4], y[4], vx[4], vy[4] (:365-377) */
#define TBX_QUERY_BRK_FIND_BRICK       119  /* {alive (-1: either), m0 .. m7} -> 1  index of the first brick, in brick order, whose bit is set in the
                                             * mask (brick i = bit i % 32 of m[i / 32], each m an integer < 2^32) and whose alive flag is the one
                                             * asked for, else -1 (find_brick :400-404 for predicates the host has turned into a mask) */
#define TBX_QUERY_AMI_MODE             120  /* -> 2  jump_timer, chase_timer (get_regular / jump / chase_mode :385-395) */
#define TBX_QUERY_AMI_ANY_CAUGHT       121  /* -> 1  any_enemy_caught :397-399 */
#define TBX_QUERY_AMI_TILE             122  /* {tx, ty} -> 1  tag (get_tile_by_pos :480-481, is_tile_walkable :472-474) */
#define TBX_QUERY_AMI_COUNT_TILES      123  /* {tag} -> 1  len(filter_tiles(tag == ...)) :483-488 */
#define TBX_QUERY_AMI_ADJACENT         124  /* {tx, ty} -> 4  tags of the up, left, right, down neighbours -- the order filter_tiles finds them (get_adjacent_tiles :512-524) */
#define TBX_QUERY_AMI_ENEMY_DISTANCES  125  /* {tx, ty} -> 8  manhattan tile distance of every enemy (enemy_distances_from_tile :526-530) */
#define TBX_QUERY_AMI_PLAYER_TILE      126  /* -> 3  tx, ty, tag (player_tile :573-576) */
#define TBX_QUERY_AMI_PLAYER_ENEMY_DISTANCES 127  /* -> 8  player_enemy_distances :579-583 */
#define TBX_QUERY_AMI_PLAYER_ON_PAINTED 128 /* -> 1  player_on_painted :586-589 */
#define TBX_QUERY_AMI_PLAYER_NEAR_UNPAINTED 129 /* {radius} -> 1  player_near_unpainted :592-603 */
#define TBX_QUERY_SI_SHIP              130  /* -> 8  x, y, w, h, speed, alive, death_counter, death_hit_1 (get_player :175-176) */
#define TBX_QUERY_AMI_TILES_MASK       131  /* {tag_mask} -> 32  filter_tiles(pred on the tag) :494-499: [ty] = bit tx set where tile (tx, ty)'s tag is in
                                             * tag_mask (bit t = tag t), ty = 0 .. 30; [31] = their number */
#define TBX_QUERY_AMI_RANDOM_TILE      133  /* {seed, draw, env_offset, tag_mask, min_enemy_distance} -> 4  tx, ty, tag, number of candidates: the
                                             * (r mod count)-th, row by row, of the tiles whose tag is in tag_mask and -- min_enemy_distance > 0 --
                                             * for which NOT every enemy is nearer than that (the predicate of set_player_random_start :543-546
                                             * as written); get_random_tile :360-378, get_random_track_position :380-386 (tag_mask 14); -1 x 3, 0 without a candidate */
#define TBX_QUERY_AMI_RANDOM_DIR       134  /* {seed, draw, env_offset, tx, ty} -> 2  direction (TBX_DIR_*) drawn among those of Up, Down, Left, Right whose
                                             * neighbour tile is walkable, and their number (get_random_dir_for_tile :550-583); -1, 0 if none */
/* every game */
#define TBX_QUERY_CHECKPOINT_VALID     140  /* {slot[, row]} -> 1  1: cell (slot, row) holds an env, 0: it is empty, -1: no such cell or no store
                                             * (row absent or -1: the env's own row); tbx_reduce_width is 1 for every game */
/* Lookahead: what happens to every env over the next `frames` frames under an action schedule -- computed from the state as it
 * stands, in registers, and thrown away: NOTHING in the engine changes (state, sim RNGs, prev_score, step outputs, render
 * records, agent layer, checkpoint store, the error flag), so no later frame or observation differs.
 *   Schedule: the horizon (1 .. TBX_LOOKAHEAD_MAX_FRAMES frames) is cut into periods of `hold` (>= 1) frames, frame j in period
 *   p = j / hold.  Period 0 plays `first`, every later one `rest`: an ALE action id of the game's legal set, or -1 = drawn by the
 *   rule of tbx_step_synthetic with counter t + p: legal[splitmix64(seed ^ ((env_offset + env) << 32) ^ (t + p)) % n_legal],
 *   seed = seed_lo | seed_hi << 32 (seed_lo, seed_hi, t, env_offset: integers below 2^32).  hold = 1, first = rest = -1 foretells
 *   tbx_step_synthetic(seed, t + j, env_offset) without auto-reset.  Trailing arguments may be left out: hold 1, first -1,
 *   rest -1, seed 0, t 0, env_offset 0.  TBX_QUERY_LOOKAHEAD_ALL answers once per legal action a (in legal-set order: Breakout
 *   0 1 3 4, Amidar 0 .. 5, SpaceInvaders 0 1 3 4 11 12, GridWorld 0 2 3 4 5) with first = legal[a], row out[env][a][0 .. 4].
 *   Run: frames 0 .. frames-1 through the game's own step, ending after the first frame that leaves lives <= 0 (an env whose game
 *   is already over still runs frame 0); no auto-reset, no draw from the sim RNG, no wrapper of the agent layer -- raw frames
 *   (with the agent layer on pass hold = skip).
 *   Out, five doubles: [0] return = sum of max(score_j - score_{j-1}, 0), score_{-1} the state's score now; [1] score and
 *   [2] lives after the last frame run; [3] frames run; [4] index of the first frame after which lives is below the lives at
 *   the start, -1 if none.
 *   TBX_E_INVALID, nothing launched: frames outside 1 .. 1024, hold < 1, more than 8 arguments, a shared first / rest that is
 *   neither -1 nor legal.  In per-env rows such an env's output (every candidate of it) is five zeros -- frames run 0 -- and the
 *   other envs are answered. */
#define TBX_LOOKAHEAD_MAX_FRAMES 1024
#define TBX_QUERY_LOOKAHEAD      150  /* {frames, hold, first, rest, seed_lo, seed_hi, t, env_offset} -> 5 */
#define TBX_QUERY_LOOKAHEAD_ALL  151  /* {frames, hold, (ignored), rest, seed_lo, seed_hi, t, env_offset} -> 5 * n_legal(game) */
/* Plans: the lookahead with an action sequence instead of one first action, and a search over every sequence of a depth.
 *   Plan codes: with L = n_legal(game), a plan of `depth` periods is code = sum over p of digit_p * L^p, digit_p an index into the
 *   legal set in its order (above), digit_0 the first action.  Period p (frames p * hold .. (p + 1) * hold - 1, as above) plays
 *   legal[digit_p] while p < depth and `rest` from then on (-1: drawn with counter t + p, the key as above).  Everything else --
 *   the run, the exit at game over, the five fields, "nothing in the engine changes", shared or per-env rows through tbx_reduce /
 *   tbx_reduce_device -- is the lookahead's.  Trailing arguments may be left out: hold 1, depth 0 (search: 1), code 0,
 *   objective 0, rest -1, seed 0, t 0, env_offset 0.
 *   TBX_QUERY_LOOKAHEAD_PLAN plays one plan per env: depth 0 .. TBX_PLAN_MAX_DEPTH(game) (the largest with L^depth <= 2^32),
 *   0 <= code < L^depth.  depth 0 is TBX_QUERY_LOOKAHEAD with first = rest, depth 1 the same with first = legal[code].
 *   TBX_QUERY_LOOKAHEAD_SEARCH plays all L^depth plans of every env (1 <= depth, L^depth <= TBX_LOOKAHEAD_MAX_PLANS: Breakout 6,
 *   SpaceInvaders and Amidar 4, GridWorld 5) and answers, for each first action a in legal-set order, row out[env][a][0 .. 5] =
 *   {ret, score, lives, frames run, life lost at, code} of the BEST plan with digit_0 = a.  Best is a total order: with
 *   loss = life lost at < 0 ? TBX_LOOKAHEAD_MAX_FRAMES + 1 : life lost at, objective 0 (return) takes the larger ret, then the
 *   larger lives, then the larger loss, then the smaller code; objective 1 (survival) the larger lives, then the larger loss,
 *   then the larger ret, then the smaller code.  Feeding a returned code to TBX_QUERY_LOOKAHEAD_PLAN gives the row's five fields.
 *   The leaves are played one after the other by (env, first action, chunk) units and only the winners leave the GPU; large
 *   searches are cut into several launches.  Neither changes the answer.
 *   TBX_E_INVALID, nothing launched: a shared value out of the ranges above (frames, hold, depth, code, objective, rest), more
 *   than 9 arguments.  In per-env rows such an env's output is zeros -- frames run 0 -- and the other envs are answered. */
#define TBX_LOOKAHEAD_MAX_PLANS 4096
#define TBX_PLAN_MAX_DEPTH(game) ((game) == TBX_GAME_BREAKOUT ? 16 : (game) == TBX_GAME_GRIDWORLD ? 13 : 12)
#define TBX_QUERY_LOOKAHEAD_PLAN   152  /* {frames, hold, depth, code, rest, seed_lo, seed_hi, t, env_offset} -> 5 */
#define TBX_QUERY_LOOKAHEAD_SEARCH 153  /* {frames, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset} -> 6 * n_legal(game) */
/* Sampled lookahead: `samples` futures per env and legal action, summed on the device.  The columns stand where those of
 * TBX_QUERY_LOOKAHEAD_SEARCH stand, `samples` for depth and `salt` for the objective.  Trailing arguments may be left out: hold 1,
 * samples 1, salt 0, rest -1, seed 0, t 0, env_offset 0.
 *   For every env and every legal action a (legal-set order, as above) future s = 0 .. samples-1 is exactly
 *   TBX_QUERY_LOOKAHEAD {frames, hold, first = legal[a], rest, seed_s, t, env_offset} played from the env's state with its game RNG
 *   salted by salt_s:
 *     seed_s = splitmix64((seed + s) mod 2^64)  (not seed + s: the draw key is seed ^ (env << 32) ^ (t + p), so neighbouring seeds
 *       would permute one another's draws across periods);
 *     salt_s = salt == 0 ? 0 : salt + s.  salt_s == 0: the game RNG is taken as it stands; otherwise both words of the game's
 *       `rand` become splitmix64(word ^ salt_s) -- the rule of TBX_EDIT_COPY_ENV's salt, applied in registers after the load and
 *       never stored.  GridWorld has no game RNG and ignores the salt.  The simulator RNG is not read by a lookahead.
 *   The run, the stop after the first frame with lives <= 0, no auto-reset, no wrapper, "nothing in the engine changes": the
 *   lookahead's.
 *   Out, row out[env][a][0 .. 7], every field an integer summed in 64-bit integers and converted to binary64 once at the store (so
 *   the row does not depend on how the samples are cut into chunks and launches): [0] samples = futures played (0: the row was
 *   refused); [1] ret_sum = sum of the futures' return -- exact while it stays below 2^53, which any score reachable by play keeps;
 *   [2] ret_min and [3] ret_max = the smallest and the largest return; [4] lives_sum = sum of lives after the last frame run;
 *   [5] lost = futures with life lost at >= 0; [6] ended = futures that ended with lives <= 0; [7] safe_frames_sum = sum of
 *   (life lost at < 0 ? frames run : life lost at).
 *   TBX_E_INVALID, nothing launched: a shared value out of the lookahead's ranges (frames, hold, rest), samples outside
 *   1 .. TBX_LOOKAHEAD_MAX_SAMPLES, salt < 0 or above 2^32 - 1, salt > 0 with salt + samples - 1 >= 2^32, more than 9 arguments.
 *   In per-env rows such an env's whole output is zeros -- field 0 = 0 -- and the other envs are answered. */
#define TBX_LOOKAHEAD_MAX_SAMPLES 4096
#define TBX_QUERY_LOOKAHEAD_SAMPLES 154  /* {frames, hold, samples, salt, rest, seed_lo, seed_hi, t, env_offset} -> 8 * n_legal(game) */
/* Search over sampled futures: every plan of a depth, each judged on the same `samples` futures, and the best plan per first action
 * by the summed outcome.  Columns 0 .. 8 stand where TBX_QUERY_LOOKAHEAD_SEARCH has them; `samples` and `salt` are appended.
 * Trailing arguments may be left out: the search's defaults (hold 1, depth 1, objective 0, rest -1, seed 0, t 0, env_offset 0), then
 * samples 1 and salt 0.
 *   Plans as in the search: 1 <= depth, L^depth <= TBX_LOOKAHEAD_MAX_PLANS, code = sum of digit_p * L^p; in addition
 *   1 <= samples <= TBX_LOOKAHEAD_MAX_SAMPLES, L^depth * samples <= TBX_LOOKAHEAD_MAX_LEAVES, and the salt ranges of
 *   TBX_QUERY_LOOKAHEAD_SAMPLES.
 *   Future s = 0 .. samples-1 of plan `code` is exactly TBX_QUERY_LOOKAHEAD_PLAN {frames, hold, depth, code, rest, seed_s, t,
 *   env_offset} played from the env's state with its game RNG salted by salt_s; seed_s = splitmix64((seed + s) mod 2^64) and
 *   salt_s = salt == 0 ? 0 : salt + s, applied in registers and never stored, are those of TBX_QUERY_LOOKAHEAD_SAMPLES.
 *   COMMON RANDOM NUMBERS: all plans of an env are played on the SAME `samples` futures -- seed_s and salt_s depend on s alone, not
 *   on the plan -- so two plans differ by what they play and not by the luck of their draws.  That is what makes plans comparable
 *   at small sample counts.
 *   Per plan the eight sums of TBX_QUERY_LOOKAHEAD_SAMPLES are kept, 64-bit integers converted to binary64 once at the final store.
 *   Out: for each first action a in legal-set order, row out[env][a][0 .. 8] = the eight sums (samples, ret_sum, ret_min, ret_max,
 *   lives_sum, lost, ended, safe_frames_sum) of the BEST plan with digit_0 = a, then [8] its code.  Best is a total order on the
 *   sums: objective 0 (return) takes the larger ret_sum, then the smaller lost, then the larger safe_frames_sum, then the smaller
 *   code; objective 1 (survival) the smaller lost, then the larger safe_frames_sum, then the larger ret_sum, then the smaller code.
 *   With samples = 1 this is NOT the order of TBX_QUERY_LOOKAHEAD_SEARCH: the search compares `lives` after the last frame, this
 *   query compares the lost flag (life lost at >= 0) and never reads lives.
 *   Chunks of suffix codes and launches over env ranges cut the work; neither changes any output bit.  "Nothing in the engine
 *   changes" is the lookahead's sentence, verbatim.
 *   TBX_E_INVALID, nothing launched: a shared value out of the ranges above (frames, hold, depth, objective, rest, samples, salt,
 *   L^depth * samples), more than 11 arguments.  In per-env rows such an env's whole output is zeros -- field 0 = 0 -- and the
 *   other envs are answered. */
#define TBX_LOOKAHEAD_MAX_LEAVES 65536
#define TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES 155  /* {frames, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, samples, salt} -> 9 * n_legal(game) */
/* Beam search: plans deeper than full enumeration reaches.  Columns 0 .. 8 stand where TBX_QUERY_LOOKAHEAD_SEARCH has them, with the
 * same defaults for trailing arguments left out; `width` is appended and defaults to 1 (greedy search).  The ranges are the
 * search's except that there is no L^depth cap: 1 <= depth <= TBX_PLAN_MAX_DEPTH(game), 1 <= width <= TBX_BEAM_MAX_WIDTH.
 *   For every env and every first action a in legal-set order, with L = n_legal(game):
 *     B_1 = {a}, the single prefix of depth 1;
 *     for d = 2 .. depth the candidates are C_d = { c + k * L^(d-1) : c in B_(d-1), k = 0 .. L-1 };
 *     candidate x of level d is valued by the five fields of TBX_QUERY_LOOKAHEAD_PLAN {frames, hold, d, x, rest, seed, t,
 *       env_offset} -- the whole horizon, with `rest` from period d on;
 *     B_d is the min(width, |C_d|) best of C_d under the search's order for `objective` (ret / lives / loss, then the smaller
 *       code).  Codes within a level are distinct, so the order is total and the kept set does not depend on how the work is cut.
 *   With C_1 = {a} valued at depth 1, row out[env][a][0 .. 5] = {ret, score, lives, frames run, life lost at, code} of the best
 *   candidate of C_depth.  It follows that with width >= L^(depth-2), or with depth = 1, the row is the row of
 *   TBX_QUERY_LOOKAHEAD_SEARCH, and that feeding the returned code to TBX_QUERY_LOOKAHEAD_PLAN with the same depth gives the row's
 *   five fields.
 *   Every candidate is replayed from the env's live state in registers, level after level on the calling stream, and a select
 *   pass between two levels ranks a group's candidates; large batches are cut into env ranges (TBX_OPT_BEAM_RANGES).  Neither
 *   changes the answer.  "Nothing in the engine changes" is the lookahead's sentence, verbatim.
 *   TBX_E_INVALID, nothing launched: a shared value out of the ranges above (frames, hold, depth, objective, rest, width), more
 *   than 10 arguments.  In per-env rows such an env's output is zeros -- frames run 0 -- and the other envs are answered. */
#define TBX_BEAM_MAX_WIDTH 64
#define TBX_QUERY_LOOKAHEAD_BEAM 156  /* {frames, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, width} -> 6 * n_legal(game) */
/* Beam search over sampled futures: the levels of TBX_QUERY_LOOKAHEAD_BEAM, every candidate judged on the same `samples` futures
 * as TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES judges its plans -- deep plans by expected outcome.  Columns 0 .. 9 are the beam's, with the
 * same defaults for trailing arguments left out; `samples` (default 1) and `salt` (default 0) are appended.
 *   For every env and every first action a in legal-set order, with L = n_legal(game), the levels are the beam's:
 *     B_1 = {a};  C_d = { c + k * L^(d-1) : c in B_(d-1), k = 0 .. L-1 } for d = 2 .. depth (C_1 = {a});
 *     B_d = the min(width, |C_d|) best of C_d.
 *   Candidate x of level d is valued by the eight integer sums of TBX_QUERY_LOOKAHEAD_SAMPLES over the futures s = 0 .. samples-1,
 *   future s being exactly TBX_QUERY_LOOKAHEAD_PLAN {frames, hold, d, x, rest, seed_s, t, env_offset} played from the env's state
 *   with its game RNG salted by salt_s; seed_s = splitmix64((seed + s) mod 2^64) and salt_s = salt == 0 ? 0 : salt + s, applied in
 *   registers and never stored, are those of queries 154 / 155.  COMMON RANDOM NUMBERS: seed_s and salt_s depend on s alone, not on
 *   the candidate and not on the level, so all candidates of an env, at every level, meet the same futures.
 *   Best is the order of TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES: objective 0 (return) takes the larger ret_sum, then the smaller lost,
 *   then the larger safe_frames_sum, then the smaller code; objective 1 (survival) the smaller lost, then the larger
 *   safe_frames_sum, then the larger ret_sum, then the smaller code.  Codes within a level are distinct, so the order is total and
 *   the kept set does not depend on how the work is cut.
 *   Out: row out[env][a][0 .. 8] = the eight sums (samples, ret_sum, ret_min, ret_max, lives_sum, lost, ended, safe_frames_sum) of the
 *   best candidate of C_depth, 64-bit integers converted to binary64 once at the store, then [8] its code.
 *   It follows that with depth = 1 columns 0 .. 7 are the row of TBX_QUERY_LOOKAHEAD_SAMPLES {frames, hold, samples, salt, rest,
 *   seed, t, env_offset}; that with width >= L^(depth-2) and the caps of TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES met the row is that
 *   query's row, bit for bit; and that with salt = 0 the returned code fed to TBX_QUERY_LOOKAHEAD_PLAN under seed_s, summed over s,
 *   gives the row's sums.  With samples = 1 it is NOT the row of TBX_QUERY_LOOKAHEAD_BEAM: the order is another (the lost flag, not
 *   lives) and the one future is played under splitmix64(seed), not under seed.
 *   Ranges: the beam's (1 <= depth <= TBX_PLAN_MAX_DEPTH(game), 1 <= width <= TBX_BEAM_MAX_WIDTH), 1 <= samples <=
 *   TBX_LOOKAHEAD_MAX_SAMPLES, the salt ranges of TBX_QUERY_LOOKAHEAD_SAMPLES, and one cap: the candidates of the widest level times
 *   the samples, L * |B_(depth-1)| * (depth == 1 ? 1 : L) * samples with |B_0| = |B_1| = 1 and |B_d| = min(width, L * |B_(d-1)|),
 *   must not exceed TBX_LOOKAHEAD_MAX_LEAVES.
 *   Every future is replayed from the env's live state in registers, level after level on the calling stream; a select pass between
 *   two levels ranks a group's candidates; the samples of a level may be cut into chunks (TBX_OPT_BEAM_SAMPLES_CHUNKS) and large
 *   batches into env ranges (TBX_OPT_BEAM_SAMPLES_RANGES).  Neither changes any output bit.  "Nothing in the engine changes" is the
 *   lookahead's sentence, verbatim.
 *   TBX_E_INVALID, nothing launched: a shared value out of the ranges above (frames, hold, depth, objective, rest, width, samples,
 *   salt, the leaf cap), more than 12 arguments.  In per-env rows such an env's whole output is nine zeros -- field 0 = 0 -- and
 *   the other envs are answered. */
#define TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES 157  /* {frames, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, width, samples, salt} -> 9 * n_legal(game) */
/* Evolutionary plan search, warm-started: a search over WHOLE plans with a budget the caller chooses -- a population of plans of
 * one depth per env and first action, valued, ranked and bred by mutation from its elite over a number of generations, optionally
 * seeded with a plan the caller hands in (a rolling-horizon controller: last step's best plan, shifted by one period).  The search
 * is deterministic and defined in integers.  Columns 0 .. 8 stand where TBX_QUERY_LOOKAHEAD_BEAM has them, with the same defaults
 * for trailing arguments left out; appended are
 *     population P   default 1    1 .. TBX_EVOLVE_MAX_POPULATION
 *     generations G  default 0    0 .. TBX_EVOLVE_MAX_GENERATIONS
 *     elite E        default 1    1 .. P
 *     plan_seed      default 0    0 .. 2^32 - 1
 *     mutation       default 64   0 .. 256
 *     init           default -1   -1, or 0 .. L^depth - 1
 *   and depth is 1 .. TBX_PLAN_MAX_DEPTH(game): there is no L^depth cap.
 *   With L = n_legal(game) and D = depth, for every env and every first action index a in legal-set order:
 *     Individuals: an individual is a plan code of depth D with digit_0 = a (plan codes: TBX_QUERY_LOOKAHEAD_PLAN's).
 *     Base word: base = splitmix64(splitmix64(plan_seed ^ (a << 32)) ^ (env_offset + env)), the sum taken in 64 bits.
 *     Draw word: w(g, i, p) = splitmix64(base ^ (g << 40) ^ (i << 8) ^ p).  It depends on nothing but its indices -- not on G, P or E.
 *     Generation 0: individual i = 0 .. P-1 has digit_0 = a and digit_p = (w(0, i, p) >> 32) % L for p = 1 .. D-1; if init >= 0,
 *       individual 0 instead takes digits 1 .. D-1 of init (its digit_0 is still a).
 *     Valuation: the five fields of TBX_QUERY_LOOKAHEAD_PLAN {frames, hold, D, code, rest, seed, t, env_offset}.
 *     Order: the search's order for `objective` (ret / lives / loss), then the smaller code.  Two individuals with one code are the
 *       same plan with the same fields; ranks are made a permutation by the smaller index i, which no output can observe.
 *     Generation g = 1 .. G, from the ranks of generation g-1: individual i < E is the individual of rank i (an elite: its record
 *       may be carried, it need not be replayed); individual i >= E takes the code of the individual of rank
 *       (w(g, i, 0) >> 32) % E, and for p = 1 .. D-1, with x = w(g, i, p): if (x & 0xff) < mutation, digit_p becomes
 *       (x >> 32) % L, otherwise it stays the parent's.
 *   Out: row out[env][a][0 .. 5] = {ret, score, lives, frames run, life lost at, code} of rank 0 of generation G.
 *   It follows that
 *     (i)   with P = 1, G = 0 and init = c the row is TBX_QUERY_LOOKAHEAD_PLAN's row for the code c - c % L + a;
 *     (ii)  a row with G' > G and everything else equal is not worse under the order: generations 0 .. G are the same
 *           populations, and elites persist;
 *     (iii) feeding the returned code to TBX_QUERY_LOOKAHEAD_PLAN at depth D gives the row's five fields;
 *     (iv)  where TBX_QUERY_LOOKAHEAD_SEARCH accepts the depth, its row is not worse than this one;
 *     (v)   with E = P or mutation = 0 every G gives generation 0's winner;
 *     (vi)  with depth 1 the row is TBX_QUERY_LOOKAHEAD_PLAN's row for code a.
 *   Every individual is replayed from the env's live state in registers, generation after generation on the calling stream, and a
 *   select pass after each ranks a group's population and breeds the next; large batches are cut into env ranges
 *   (TBX_OPT_EVOLVE_RANGES, capped by TBX_OPT_BEAM_RANGE_ENVS).  Neither changes the answer.  "Nothing in the engine changes" is the
 *   lookahead's sentence, verbatim.
 *   TBX_E_INVALID, nothing launched: a shared value out of the ranges above (frames, hold, depth, objective, rest, population,
 *   generations, elite, plan_seed, mutation, init), more than 15 arguments.  In per-env rows such an env's rows are zeros -- frames
 *   run 0 -- and the other envs are answered. */
#define TBX_EVOLVE_MAX_POPULATION  256
#define TBX_EVOLVE_MAX_GENERATIONS 64
#define TBX_QUERY_LOOKAHEAD_EVOLVE 158  /* {frames, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, population, generations, elite, plan_seed, mutation, init} -> 6 * n_legal(game) */
/* Closed-loop planning: pick, act and carry.  Queries 153 .. 158 answer one row per env and first action; this one runs such a
 * planner, picks every env's winner among its L = n_legal(game) rows ON THE DEVICE, leaves the chosen action where the
 * device-pointer steps read it and keeps the winner's plan, shifted by one period, as the next call's warm start -- so the loop
 * plan, act, shift, plan again can be queued on one stream without the host in it.
 *   Arguments: {planner, then the planner's own columns in its own order}.  planner is TBX_QUERY_LOOKAHEAD_SEARCH (153),
 *   _SEARCH_SAMPLES (155), _BEAM (156), _BEAM_SAMPLES (157) or _EVOLVE (158): the five that carry an objective and answer a code
 *   (greedy one-step choice: 153 with depth 1; over sampled futures: 155 with depth 1).  Trailing planner columns may be left out
 *   with the planner's defaults; at most 1 + the planner's maximum (9, 11, 10, 12, 15) arguments -- for 158 that is
 *   16 = TBX_EDIT_MAX_ARGS.  SHARED ARGUMENTS ONLY: per_env = 1 answers TBX_E_INVALID with nothing launched.  Every shared value is
 *   range-checked exactly as the planner checks it.
 *   Planning: the planner's query runs from the live state, unchanged; its rows [N][L][6 or 9] go to engine-owned scratch.
 *   Pick: one winner a* per env among the L rows.  Planners 153 / 156 / 158: the search's order for `objective` on (ret, lives,
 *   loss), then the smaller code -- codes of different first actions differ in digit 0, so the order is total.  Planners 155 / 157:
 *   the order of TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES on (ret_sum, lost, safe_frames_sum), then the smaller action index.
 *   Out, width 11 for every game: out[env][0] = the ALE action legal[a*], [1] = the index a*, [2 ..] = the winner's planner row,
 *   6 or 9 doubles, zero-padded to 9.
 *   Side outputs, engine-owned (tbx_device_buffer):
 *     TBX_BUF_PLAN_ACTION int32[N]: the ALE action of [0]; its pointer is a valid ale_actions_dev for tbx_step_device and
 *       tbx_agent_step_device, and a step queued on the same stream behind the call reads the finished buffer.
 *     TBX_BUF_PLAN_CARRY uint32[N]: the winner's code shifted by one period, carry = code / L + (code % L) * L^(depth-1) in 32-bit
 *       arithmetic: the played digit wraps to the end, where the next call replaces nothing but digit 0.
 *   The carry of an engine is zero from tbx_create on (carry 0 is the all-first-action plan, a valid code at every depth); both
 *   arrays are made, zeroed, when this query is first asked with shared arguments and one of the five planners -- like the rollout
 *   ids before the first chunk, the two ids answer TBX_E_INVALID until then -- and keep their addresses from there to tbx_destroy.  They are rewritten for
 *   every env by each successful call of this query and left unchanged by a refused one.  They are NOT env state: TBX_EDIT_COPY_ENV, the
 *   checkpoint edits, tbx_new_game and tbx_set_states leave them alone -- harmless, because an init is only one seeded individual.
 *   Warm start from the carry: inside this query alone, planner 158 accepts init = -2: env e plays with
 *   init = carry[e] % L^depth, the modulus taken in 64 bits (so a carry of a deeper call is cut to the depth at hand).  The rounds,
 *   slots and env ranges are those of the shared row.  TBX_QUERY_LOOKAHEAD_EVOLVE itself keeps refusing -2.
 *   "Nothing in the engine changes" holds for state, RNGs, step outputs, records, agent layer and checkpoint store: the two buffers
 *   above and the scratch are the only writes.  On tbx_reduce_device everything runs on the caller's stream in order.
 *   It follows that
 *     (i)   out[env][2 ..] is the planner's own row for a*: feeding [1] and the code to TBX_QUERY_LOOKAHEAD_PLAN reproduces it as
 *           the planner's consequences say;
 *     (ii)  with 158 and init = -2, for every G the row of first action a is not worse than TBX_QUERY_LOOKAHEAD_PLAN's row for the
 *           carried plan with digit 0 = a (it is individual 0 of generation 0, and elites persist), and it is the row of
 *           TBX_QUERY_LOOKAHEAD_EVOLVE with per-env init = carry % L^depth;
 *     (iii) two calls with equal arguments and no step between them give equal rows and actions whenever init != -2;
 *     (iv)  env ranges (TBX_OPT_BEAM_RANGE_ENVS) and chunk options change no output bit.
 *   TBX_E_INVALID, nothing launched, both buffers unchanged: per_env = 1, a planner other than the five, more arguments than
 *   1 + the planner's maximum, whatever the planner refuses in a shared row. */
#define TBX_QUERY_LOOKAHEAD_ACT 159  /* {planner, the planner's columns} -> 11 */
/* Tree search: open-loop Monte-Carlo tree search over plan prefixes -- a budget of `simulations` stochastic futures per env and
 * first action, spent ADAPTIVELY: where queries 154 / 155 / 157 give every candidate the same samples and 156 / 158 fit deep plans
 * to one future, this one grows a tree of action prefixes and sends each new future down the branch its statistics favour.  The
 * search is deterministic and defined in integers.  Columns 0 .. 8 stand where TBX_QUERY_LOOKAHEAD_BEAM has them, with the same
 * defaults for trailing arguments left out and the same ranges (1 <= depth <= TBX_PLAN_MAX_DEPTH(game), no L^depth cap); appended are
 *     simulations M  default 1    1 .. TBX_TREE_MAX_SIMULATIONS
 *     explore        default 0    0 .. TBX_TREE_MAX_EXPLORE, an integer in units of the value (below)
 *     salt           default 0    the ranges of TBX_QUERY_LOOKAHEAD_SAMPLES with `simulations` in the place of `samples`
 *   Tree: one for every env and every first action index a in legal-set order, with L = n_legal(game).  Its nodes are plan prefixes
 *   with digit_0 = a (plan codes: TBX_QUERY_LOOKAHEAD_PLAN's); the root, node 0, is the prefix of depth 1.  A node keeps n, the
 *   completed simulations through it, v_sum, the 64-bit sum of their values, and L child links.  Nodes are numbered in creation order.
 *   Value of a simulation, from its five fields: objective 0 (return) v = ret; objective 1 (survival)
 *   v = life lost at < 0 ? frames run : life lost at -- the safe-frames term of TBX_QUERY_LOOKAHEAD_SAMPLES.  Both are
 *   non-negative integers.
 *   Selection: for simulation m = 0 .. M-1, in order, start with cur = root, d = 1, code = a.  While d < depth:
 *     if cur lacks a child: take the smallest missing digit k, create that node, code += k * L^d, d += 1, and stop -- the
 *       expansion, at most one node per simulation;
 *     otherwise choose the k that maximises P_k = Q_k + U_k over the children, the smaller k winning a tie, with
 *       Q_k = (v_sum_k * 256) / n_k (integer division), U_k = explore * isqrt(n_cur << 16) / (1 + n_k), isqrt the exact floor
 *       square root and n_cur the count of cur before this simulation -- everything in signed 64-bit arithmetic, which the ranges
 *       above keep below 2^60 -- then code += k * L^d, d += 1, cur = child_k.
 *   If the loop ends with d == depth nothing is expanded.
 *   Play: exactly TBX_QUERY_LOOKAHEAD_PLAN {frames, hold, d, code, rest, seed_m, t, env_offset} from the env's state with its game
 *   RNG salted by salt_m; seed_m = splitmix64((seed + m) mod 2^64) and salt_m = salt == 0 ? 0 : salt + m are the rules of
 *   TBX_QUERY_LOOKAHEAD_SAMPLES, applied in registers and never stored.  COMMON RANDOM NUMBERS: all L trees of an env meet the same
 *   future m.
 *   Backup: every node on the path, the root and a new node included, gets n += 1 and v_sum += v; the root also accumulates the
 *   eight integer sums of TBX_QUERY_LOOKAHEAD_SAMPLES.
 *   Out: row out[env][a][0 .. 11].  [0 .. 7] the root's eight sums (samples = M, ret_sum, ret_min, ret_max, lives_sum, lost, ended,
 *   safe_frames_sum), 64-bit integers converted to binary64 once at the store.  Then the principal variation: from the root, while
 *   the node has a child, move to the child with the largest n, ties to the larger v_sum, then to the smaller k; [8] the final
 *   node's code, [9] its depth, [10] its n, [11] its v_sum.
 *   It follows that
 *     (i)   with depth 1 columns 0 .. 7 are the row of TBX_QUERY_LOOKAHEAD_SAMPLES {frames, hold, M, salt, rest, seed, t,
 *           env_offset} and [8 .. 10] = a, 1, M;
 *     (ii)  with depth >= 2 and M <= L simulation m plays code a + m * L at depth 2 on future m;
 *     (iii) with depth >= 2 the n of the root's children sum to M, and [9] >= 2;
 *     (iv)  env ranges (TBX_OPT_TREE_RANGES, capped by TBX_OPT_BEAM_RANGE_ENVS) and cuts of the simulations into several launches
 *           (TBX_OPT_TREE_LAUNCH_SIMULATIONS) change no output bit;
 *     (v)   two equal calls with no step between them give equal rows.
 *   The budget is per first action, not one root over the L actions: the row-per-first-action convention of every other planner
 *   holds, and callers pick the action with the order of the sampled planners on the root sums.
 *   The trees live in engine-owned scratch between the launches of one query, on the calling stream.  "Nothing in the engine
 *   changes" is the lookahead's sentence, verbatim.
 *   TBX_E_INVALID, nothing launched: a shared value out of the ranges above (frames, hold, depth, objective, rest, simulations,
 *   explore, salt), more than 12 arguments.  In per-env rows such an env's rows are 12 zeros per action -- field 0 = 0 -- and the
 *   other envs are answered. */
#define TBX_TREE_MAX_SIMULATIONS 1024
#define TBX_TREE_MAX_EXPLORE     1048576
#define TBX_QUERY_LOOKAHEAD_TREE 160  /* {frames, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, simulations, explore, salt} -> 12 * n_legal(game) */
/* Closed-loop tree search: search, pick, act and CARRY THE CHOSEN SUBTREE.  TBX_QUERY_LOOKAHEAD_ACT closes the loop for the planners
 * that answer a plan code; this query closes it for TBX_QUERY_LOOKAHEAD_TREE, whose memory is a tree: after a* is played, the subtree
 * under the root's children of tree a* is a search already done for the next state, and the next call may start from it.
 *   Arguments: {the twelve columns of TBX_QUERY_LOOKAHEAD_TREE in its order, reuse}.  Trailing columns may be left out with 160's
 *   defaults; reuse defaults to 0 and must be 0 or 1; at most 13 arguments.  SHARED ARGUMENTS ONLY: per_env = 1 answers TBX_E_INVALID
 *   with nothing launched.  Every shared value is checked exactly as TBX_QUERY_LOOKAHEAD_TREE checks it.
 *   Step 1, start trees, per env e and first action index a.  With reuse = 1 the tree starts as the carried tree (e, a) of the store
 *   (below) where one is LIVE: the store exists, its key (frames, hold, depth, objective, simulations) equals this call's, env e's
 *   drop flag is clear, and the carried tree is present (node count above 0).  Otherwise, and with reuse = 0 always, it starts as
 *   160's empty root.  The root's eight sums start at zero in every call: they cover this call's M futures only, so samples = M and
 *   rows stay comparable between actions and between calls.  Carried statistics steer the selection and nothing else.
 *   Step 2, M simulations: exactly 160's selection, play, backup and common random numbers, on the start trees.  A link that the
 *   carry dropped (below) is a missing child and is re-expanded as 160 expands.  Row columns 0 .. 7 are this call's sums; columns
 *   8 .. 11 are the principal variation of the whole tree, carried nodes included, so pv_visits may exceed M.
 *   Step 3, pick: one winner a* per env among the L rows, by the order of TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES on (ret_sum, lost,
 *   safe_frames_sum) for `objective`, then the smaller action index -- TBX_QUERY_LOOKAHEAD_ACT's pick of a sampled planner.
 *   Out, width 14 for every game: out[env] = {legal[a*], a*, the twelve columns of a*'s row}.  legal[a*] also goes to
 *   TBX_BUF_PLAN_ACTION int32[N], the buffer and pointer of TBX_QUERY_LOOKAHEAD_ACT (this query makes both of that query's buffers,
 *   zeroed, if they do not exist yet); TBX_BUF_PLAN_CARRY is left unchanged.
 *   Step 4, carry: for every k in 0 .. L-1 the new carried tree (e, k) is the subtree of the final tree a* under the root's child k,
 *   absent (node count 0) where the root has no such child; with depth 1 everything is absent.  Node ids in a tree always grow from
 *   parent to child (creation order; the carry preserves it), so the subtree's nodes are taken in ascending source id: the first
 *   `keep` of them are kept and renumbered 0, 1, 2, ... in that order -- the root's child comes first and becomes the new root.  A
 *   link to a node that was not kept becomes 0; a dropped node's descendants have larger ids and are dropped with it; the
 *   ancestors keep their n and v_sum.  keep = simulations + 1 (TBX_OPT_TREE_CARRY_KEEP lowers it), so a start tree plus M
 *   expansions never passes 2 * simulations + 1 nodes and the ids stay in 16 bits.  If the new root's n exceeds
 *   TBX_TREE_CARRY_MAX_VISITS (TBX_OPT_TREE_CARRY_MAX_VISITS lowers it), every kept node of that tree gets n = (n + 1) / 2 and
 *   v_sum = v_sum / 2, integer divisions: values are non-negative and every carried node has n >= 1, so no n becomes 0 and
 *   child n <= parent n survives.  No node's n ever passes TBX_TREE_CARRY_MAX_VISITS + TBX_TREE_MAX_SIMULATIONS = 5120: that, with
 *   the ranges of 160, is what keeps the selection's signed 64-bit arithmetic below 2^60 in this query (v_sum <= 5120 values of at
 *   most 2^31, times 256; explore * isqrt(5120 << 16) < 2^20 * 2^15).
 *   The store, TBX_BUF_PLAN_TREE, engine-owned: made by the first successful call of this query, TBX_E_INVALID until then.  N x L unit
 *   blocks in env-major order, block (e, k) at byte (e * L + k) * (64 + 32 * stride), stride = (simulations + 2) & ~1.  A block is one
 *   64-byte line whose first uint32 is the node count (0: absent) and whose other bytes are zero, then `stride` nodes of 32 bytes:
 *   int64 v_sum, uint32 n, uint16 child[6] (0: no child; child[L ..] zero), and 8 bytes of zero.  Nodes past the count are
 *   unspecified.  The store is rewritten for every env by each successful call, with either value of reuse, and left byte for byte
 *   unchanged by a refused one.  Its size follows `simulations`: a call with another `simulations` may move it (ask
 *   tbx_device_buffer again), and the key rule has made its content dead by then.  A failed allocation returns the HIP error and
 *   leaves the engine without a store.  The drop flags (uint8[N]) and the key live beside it.  All of it is ENGINE state, not env
 *   state: TBX_EDIT_COPY_ENV, the checkpoint edits, tbx_new_game and tbx_set_states leave it alone.  A caller who resets or rewrites
 *   envs says so with TBX_EDIT_TREE_DROP (no arguments, the usual mask in host or device form, NULL meaning all; TBX_E_INVALID before
 *   the store exists): it sets the drop flag of the masked envs, the next call of this query starts those envs' trees empty whatever
 *   reuse says, and every successful call clears all flags.  In the device form it is one small kernel on the given stream, so a
 *   device-side loop queues it behind every step with mask_dev = the step's own done buffer and forgets the trees of games that
 *   ended, with no host in it.  A stale tree is a heuristic gone wrong, not a wrong answer -- but statistics of a lost game must not
 *   steer a new one.
 *   "Nothing in the engine changes" holds for state, RNGs, step outputs, records, agent layer and checkpoint store: the action buffer,
 *   the store with its flags and key, and the scratch are the only writes.  On tbx_reduce_device everything runs on the caller's
 *   stream in order, with no host synchronisation in a call that allocates nothing.  The scratch: the working trees of one env range
 *   have 2 * simulations + 2 nodes and live in the planners' shared scratch under twice its usual budget (512 MiB instead of 256), so
 *   that the env ranges are never smaller than TBX_QUERY_LOOKAHEAD_TREE's; that scratch only grows, so an engine that has run this
 *   query keeps up to 512 MiB for its later planner queries, until tbx_destroy.
 *   It follows that
 *     (i)   with reuse = 0 columns 2 .. 13 are TBX_QUERY_LOOKAHEAD_TREE's row for a* bit for bit, and a* is the sampled planners'
 *           pick on 160's rows;
 *     (ii)  with reuse = 1 and no live tree the call equals reuse = 0: the first call, a changed key, dropped envs;
 *     (iii) column `samples` is M in every row;
 *     (iv)  env ranges (TBX_OPT_BEAM_RANGE_ENVS) and launch cuts (TBX_OPT_TREE_LAUNCH_SIMULATIONS) change no output bit and no byte of
 *           the store;
 *     (v)   the store after a call is step 4 applied to the final trees, node by node;
 *     (vi)  a refused call changes neither buffer nor store nor flags.
 *   TBX_E_INVALID, nothing launched: per_env = 1, more than 13 arguments, reuse other than 0 or 1, whatever
 *   TBX_QUERY_LOOKAHEAD_TREE refuses in a shared row. */
#define TBX_TREE_CARRY_MAX_VISITS 4096   /* 4 * TBX_TREE_MAX_SIMULATIONS */
#define TBX_QUERY_LOOKAHEAD_TREE_ACT 161  /* {the twelve columns of 160, reuse} -> 14 */
#define TBX_EDIT_TREE_DROP 44             /* {} : the masked envs' carried trees are dead for the next TBX_QUERY_LOOKAHEAD_TREE_ACT */
/* ids of tbx_device_buffer that exist only once their query has run */
enum {
    TBX_BUF_PLAN_ACTION = 17,    /* int32[N]  the ALE action every env's winner of the last TBX_QUERY_LOOKAHEAD_ACT / _TREE_ACT plays first */
    TBX_BUF_PLAN_CARRY = 18,     /* uint32[N] that winner's plan code shifted by one period: the next call's init = -2 */
    TBX_BUF_PLAN_TREE = 19       /* the carried trees of the last TBX_QUERY_LOOKAHEAD_TREE_ACT, N x n_legal unit blocks (layout above) */
};
int tbx_reduce_width(int game, int query);   /* doubles per env, or TBX_E_INVALID */
int tbx_edit(tbx_engine* engine, int op, const double* args_host, int n_args, int per_env, const uint8_t* mask_host);
int tbx_edit_device(tbx_engine* engine, int op, const double* args, int n_args, int per_env, const uint8_t* mask_dev, void* stream);
int tbx_reduce(tbx_engine* engine, int query, const double* args_host, int n_args, int per_env, double* out_host);
int tbx_reduce_device(tbx_engine* engine, int query, const double* args, int n_args, int per_env, double* out_dev, void* stream);

/* ------------------------------------------------------------------ agent-side preprocessing (SURVEY.md 8f rank 1 + 2)
 * The per-env wrapper stack that the reference's vendored baselines put between the env and the learner, fused on the
 * device so that only the small stacked observation ever leaves the chip.  The composition is the reference's, class by
 * class, with each class's state kept per env (baselines/baselines/common/...):
 *   NoopResetEnv(noop_max) atari_wrappers.py:108-135  1..noop_max no-op frames after a real reset (a game that ends inside them
 *                          is started again); the observation of such a reset is the raw frame after the last no-op
 *   MaxAndSkipEnv(skip)    atari_wrappers.py:193-219  repeat the action `skip` frames until the game ends, sum the rewards;
 *                          observation = per-pixel max of a PERSISTENT two-frame buffer that frame skip-2 and frame skip-1
 *                          write (zero frames at construction, never cleared by a reset: a step cut short by the end of
 *                          the game leaves the slots it did not reach as they were)
 *   bench.Monitor          bench/monitor.py:45-76     episode return (unclipped) and length in agent steps
 *   EpisodicLifeEnv        atari_wrappers.py:157-191  a lost life ends the agent's episode; its reset() is a real reset only
 *                          after a real game over, otherwise ONE no-op agent step whose `done` is ignored (:186-187)
 *   FireResetEnv           atari_wrappers.py:137-155  reset(), then agent steps with action #1 and action #2 of the action
 *                          set, each followed by a reset() if it reports done; the observation is the one of the second step
 *   WarpFrame              atari_wrappers.py:230-244  gray frame (Toybox frames are already gray, :241-242) resized to
 *                          out_w x out_h by area averaging (exact rational weights, round half up)
 *   ClipRewardEnv          atari_wrappers.py:221-227  sign(reward)
 *   DummyVecEnv            vec_env/dummy_vec_env.py:45-60  an env that reports done is reset and its observation is reset()'s
 *   VecFrameStack(stack)   vec_env/vec_frame_stack.py:17-30  roll the channel axis, zero the stack of envs that are done,
 *                          write the new frame last -- or, with stack_fill = 1, FrameStack(k) inside every env
 *                          (atari_wrappers.py:246-275): the same roll, but a reset fills the whole stack with its observation
 * obs = uint8[N][out_h][out_w][stack], reward float32[N], done uint8[N].
 * Not the Python's: NoopResetEnv draws its count from numpy's RandomState; here it is counter-based (below) unless counts
 * are injected with tbx_agent_set_noops.  bench.Monitor raises when an env is stepped after its game ended inside
 * EpisodicLifeEnv's ignored no-op step; here that is TBX_E_NEEDS_RESET and the stack carries on as it does without a Monitor.
 * Accepted output geometries, for an H x W frame (tbx_frame_dims): 1 <= out_h <= H, 1 <= out_w <= W, out_w <= 128 and
 * out_h * out_w <= 7056 (else TBX_E_INVALID), and at most 8 source pixels per output pixel on each axis,
 * ceil(H / out_h) + 1 <= 8 and ceil(W / out_w) + 1 <= 8 (else TBX_E_UNSUPPORTED).  Per game, out_w and out_h range over:
 *   Breakout       160 x 240  out_w 35..128, out_h 23..min(160, 7056 / out_w)  (out_h = 160 for out_w <= 44)
 *   SpaceInvaders  210 x 320  out_w 46..128, out_h 30..min(210, 7056 / out_w)  (out_h = 210 never: at most 153)
 *   Amidar         250 x 160  out_w 23..128, out_h 36..min(250, 7056 / out_w)  (out_h = 250 for out_w <= 28)
 *   GridWorld      128 x 160  out_w 23..128, out_h 19..min(128, 7056 / out_w)  (out_h = 128 for out_w <= 55) */
typedef struct tbx_agent_config {
    int32_t skip;          /* >= 1 (4) */
    int32_t out_h, out_w;  /* 84, 84 */
    int32_t stack;         /* 1..4 (4) */
    int32_t clip_reward;   /* 0 / 1 */
    int32_t episodic_life; /* EpisodicLifeEnv on / off */
    int32_t fire_reset;    /* FireResetEnv on / off */
    int32_t noop_max;      /* NoopResetEnv: 1..noop_max no-op frames after a real reset; 0 = off */
    uint64_t noop_seed;    /* count = 1 + splitmix64(noop_seed ^ (global env << 32) ^ episode index) % noop_max */
    uint64_t env_offset;   /* global index of env 0 of this engine (sharded batches) */
    int32_t stack_fill;    /* what a reset leaves in the OLDER stack slots: 0 = zeros (VecFrameStack, vec_frame_stack.py:22-33),
                            * 1 = the reset observation itself (the per-env FrameStack of wrap_deepmind(frame_stack=True),
                            * atari_wrappers.py:246-275: reset() appends the observation k times) */
    int32_t new_plane;     /* 1: the observation kernels also write the NEWEST plane alone, dense, into TBX_BUF_AGENT_PLANE
                            * (uint8[N][out_h][out_w]) -- what a host-side VecFrameStack receives per step (one new frame per
                            * env, vec_frame_stack.py:19-27), a quarter of the bytes of the whole stacks.
                            * 2: the plane INSTEAD of the stack -- the reference's own data flow, where a worker produces one
                            * frame per step and the stack exists only at the receiver (vec_frame_stack.py:17-30; LazyFrames
                            * shares the frames between observations, atari_wrappers.py:288-317).  The device keeps a ring of
                            * the last `stack` planes, TBX_BUF_AGENT_RING = uint8[stack][N][out_h][out_w]; every reset / agent
                            * step writes slot head = (head + 1) % stack (tbx_agent_ring_head; TBX_BUF_AGENT_PLANE is that slot's
                            * address and moves with it), so the stack of env i, oldest first, is ring[(head + 1 + c) % stack][i],
                            * c = 0 .. stack - 1 -- the same bytes as TBX_BUF_AGENT_OBS[i][y][x][c] of the other modes.  An env
                            * whose stack starts afresh (reset; done under VecFrameStack) gets its other slots rewritten (zeros,
                            * or the observation with stack_fill = 1).  7 KB written per env and step instead of the roll's 21 KB
                            * read + 28 KB written.  There is no TBX_BUF_AGENT_OBS and no obs output in this mode (TBX_E_INVALID). */
} tbx_agent_config_t;

int tbx_agent_init(tbx_engine* engine, const tbx_agent_config_t* cfg);
/* tbx_agent_init constructs the stack (zero frame buffers, EpisodicLifeEnv.was_real_done = True, Monitor idle).  A call that fails
 * once it has begun to replace the stack leaves the engine WITHOUT an agent layer: later agent calls answer "tbx_agent_init has
 * not been called" until one succeeds. */
/* NoopResetEnv.override_num_noops (atari_wrappers.py:115-123) per env: counts_host[i] > 0 replaces the drawn count in env i,
 * 0 keeps the default rule; NULL removes the override. */
int tbx_agent_set_noops(tbx_engine* engine, const int32_t* counts_host);
/* venv.reset(): reset() of every env's stack (so with EpisodicLifeEnv on, a SECOND call in the middle of an episode only
 * advances one no-op agent step, as in the reference); stack = zeros with the warped observation last (VecFrameStack.reset).
 * obs_host may be NULL. */
int tbx_agent_reset(tbx_engine* engine, uint8_t* obs_host);
/* one agent step with host pointers (synchronous); any output pointer may be NULL */
int tbx_agent_step(tbx_engine* engine, const int32_t* ale_actions_host, float* reward_host, uint8_t* done_host, uint8_t* obs_host);
/* device-resident forms: actions in HBM, or generated on the device like tbx_step_synthetic with t = agent step index
 * (every sub-frame of an agent step repeats the same action); results in TBX_BUF_AGENT_*.  Both return before the step has
 * run: their return code speaks of the call alone (TBX_E_INVALID before tbx_agent_init or for a NULL action pointer), and what the
 * synchronous tbx_agent_step returns about the step itself -- TBX_E_ACTION, TBX_E_NEEDS_RESET -- arrives with the next tbx_sync,
 * once for all steps queued since the last one (see there for which code wins). */
int tbx_agent_step_device(tbx_engine* engine, const int32_t* ale_actions_dev, void* stream);
int tbx_agent_step_synthetic(tbx_engine* engine, uint64_t action_seed, uint64_t t, uint64_t env_offset, void* stream);

#define TBX_BUF_AGENT_OBS    6   /* uint8[N][out_h][out_w][stack] */
#define TBX_BUF_AGENT_REWARD 7   /* float32[N] */
#define TBX_BUF_AGENT_DONE   8   /* uint8[N] */
/* episode monitor (bench.Monitor / VecMonitor: baselines/bench/monitor.py:51-76, common/vec_env/vec_monitor.py:21-37) */
#define TBX_BUF_AGENT_EP_DONE   9    /* uint8[N]   a real episode (game over) ended during the last agent step */
#define TBX_BUF_AGENT_EP_RETURN 10   /* float32[N] its unclipped return 'r' (valid where EP_DONE) */
#define TBX_BUF_AGENT_EP_LENGTH 11   /* int32[N]   its length 'l' in agent steps (valid where EP_DONE) */
/* host copy of the three episode-monitor arrays of the last agent step (any pointer may be NULL) */
int tbx_agent_episodes(tbx_engine* engine, uint8_t* ep_done_host, float* ep_return_host, int32_t* ep_length_host);
#define TBX_BUF_AGENT_PLANE    13   /* uint8[N][out_h][out_w] the newest plane of every stack (tbx_agent_config_t::new_plane) */
#define TBX_BUF_AGENT_RING     14   /* uint8[stack][N][out_h][out_w] the last `stack` planes (new_plane = 2), newest in slot head */
/* the ring slot that holds the newest plane (new_plane = 2; 0 .. stack - 1, advanced by every tbx_agent_reset / agent step) */
int tbx_agent_ring_head(tbx_engine* engine, int32_t* out_head);

/* ------------------------------------------------------------------ host delivery: step_async / step_wait
 * The reference's consumers sit on the HOST side of the boundary: VecEnv.step_async(actions) sends the actions to the workers,
 * step_wait() receives (obs, rews, dones, infos) (baselines/baselines/common/vec_env/__init__.py:26-131,
 * subproc_vec_env.py:63-74), and what a worker sends per step is ONE new frame per env -- VecFrameStack rolls its stack on the
 * receiving side (vec_frame_stack.py:17-30).  The "_begin" calls queue the whole step on the engine's stream -- actions host ->
 * device, the step (the agent step with all its wrappers), and the copies of every requested output into the caller's host
 * buffers -- and return at once; the "_end" call blocks until they have arrived and reports what the synchronous form reports
 * (TBX_E_ACTION, TBX_E_NEEDS_RESET).  Between the two the caller's thread is free (the learner's update of the previous
 * rollout step overlaps with the device step and the PCIe copy).  Every pointer of the out-struct may be NULL; the buffers must stay valid
 * until the "_end" call returns and should be page-locked (tbx_host_alloc): a copy into pageable memory is staged by the runtime and blocks the
 * "_begin" call.  The actions are copied out of the caller's array before "_begin" returns.  Any other call on the handle
 * between "_begin" and "_end" ends the step first (program order holds as everywhere). */
int tbx_host_alloc(void** out_ptr, size_t bytes);   /* page-locked host memory (hipHostMalloc), any device */
int tbx_host_free(void* ptr);
typedef struct tbx_agent_host_out {
    float*   reward;      /* float32[N] */
    uint8_t* done;        /* uint8[N] */
    uint8_t* obs;         /* uint8[N][out_h][out_w][stack]: the whole stacks (TBX_BUF_AGENT_OBS; not with new_plane = 2) */
    uint8_t* plane;       /* uint8[N][out_h][out_w]: the newest plane only (TBX_BUF_AGENT_PLANE; needs new_plane = 1 or 2) */
    uint8_t* ep_done;     /* uint8[N], float32[N], int32[N]: the episode monitor (tbx_agent_episodes) */
    float*   ep_return;
    int32_t* ep_length;
} tbx_agent_host_out_t;
int tbx_agent_step_begin(tbx_engine* engine, const int32_t* ale_actions_host, const tbx_agent_host_out_t* out);
int tbx_agent_step_end(tbx_engine* engine);
/* the current contents of the same buffers (after tbx_agent_reset or a step), synchronous: what venv.reset() hands out when
 * the host keeps the stacks (tbx_agent_reset(NULL), then the plane) */
int tbx_agent_fetch(tbx_engine* engine, const tbx_agent_host_out_t* out);
/* The plain env step in the same shape: ToyboxBaseEnv.step for every env (envs/atari/base.py:115-149 under
 * dummy_vec_env.py:45-54) = tbx_step + the frames of the states it leaves (channels 1, 3 or 4; frame may be NULL). */
typedef struct tbx_step_host_out {
    int32_t* reward;      /* int32[N] */
    uint8_t* done;        /* uint8[N] */
    int32_t* lives;       /* int32[N] */
    int32_t* score;       /* int32[N] */
    uint8_t* frame;       /* uint8[N][H][W][channels] */
    int32_t  channels;
    int32_t  _pad;
} tbx_step_host_out_t;
int tbx_step_begin(tbx_engine* engine, const int32_t* ale_actions_host, uint32_t flags, const tbx_step_host_out_t* out);
int tbx_step_end(tbx_engine* engine);
/* The receiving side's frame stack as host code: VecFrameStack.step_wait (vec_frame_stack.py:17-27) over channel-last stacks
 * uint8[n][px][stack] -- dst = src with every pixel's channels rolled by one and `plane` (uint8[n][px], what tbx_agent_host_out_t::
 * plane received) as the newest channel; the stack of an env whose `done` byte is set starts anew: zeros in the older channels
 * (fill = 0, VecFrameStack :21-23) or the new plane in every channel (fill = 1, FrameStack.reset inside the env,
 * atari_wrappers.py:257-261).  done == NULL: no env is done; reset != 0: every env is (VecFrameStack.reset :29-33).  dst may
 * be src.  Plain host loops on `threads` threads (<= 0: the usable cores, at most 16); no engine, no device. */
int tbx_host_stack_push(uint8_t* dst, const uint8_t* src, const uint8_t* plane, const uint8_t* done, int reset,
                        int n, int px, int stack, int fill, int threads);

/* ------------------------------------------------------------------ multi-GPU record gather
 * One process per GPU, one engine per process = one contiguous shard of the env batch; envs never interact, so the only
 * exchange is one all-gather per step of the packed TBX_BUF_PACKED records (8 B/env: reward i32, done u8, lives u8) over
 * RCCL / xGMI.  replaces the pipes of pickled (ob, rew, done, info) tuples between the reference's worker processes and
 * the learner (baselines/baselines/common/vec_env/subproc_vec_env.py:63-74); frames stay on their GPU.
 * librccl is resolved with dlopen inside these calls (no link-time dependency, no PyTorch); without it they return
 * TBX_E_UNSUPPORTED and a caller may fall back to gathering the records on the host. */
#define TBX_GATHER_ID_BYTES 128
/* rank 0: a fresh communicator id (ncclGetUniqueId) to hand to every rank out of band (file, env var, pipe).
 * Errors are reported through tbx_last_error(NULL). */
int tbx_gather_unique_id(void* id_out, size_t id_bytes);
/* Collective over all ranks (ncclCommInitRank).  records_per_rank >= this engine's env count is the per-rank slot width of
 * the gathered layout [nranks][records_per_rank] (ranks may hold unequal shards; unused slots read 0). */
int tbx_gather_init(tbx_engine* engine, int nranks, int rank, int records_per_rank, const void* id, size_t id_bytes);
/* What the communicator itself reports (ncclCommCount; == nranks after a successful tbx_gather_init) and the path of the
 * librccl that was loaded -- so that a benchmark line can say which collective really ran over how many ranks. */
int tbx_gather_nranks(tbx_engine* engine);
const char* tbx_gather_library(tbx_engine* engine);
/* K of the record ring this communicator was initialised with (TBX_OPT_GATHER_EVERY at tbx_gather_init; 1 = a collective per
 * step), and how many steps' records sit in the ring waiting for the next collective (0 right after one went out). */
int tbx_gather_every(tbx_engine* engine);
int tbx_gather_fill(tbx_engine* engine);
/* Queue the all-gather of the last step's records into out_dev (NULL: the engine-owned TBX_BUF_GATHERED) -- with a K-step ring
 * (TBX_OPT_GATHER_EVERY) only every K-th call queues anything, then for the last K steps at once.  Asynchronous: it
 * is ordered after everything queued through this handle so far, runs on an engine-owned communication stream, and the next
 * step that rewrites those records is ordered after it -- what the caller queues in between (the rasteriser) overlaps with it.  `stream` is not used to run it; make a
 * stream wait for the result with tbx_gather_wait.
 * With the fused call (tbx_render_step_synthetic) in stream order and one collective PER STEP there is nothing in between: the
 * collective waits for the whole launch (the step rides in it) and the next launch rewrites the same records, so it waits for
 * the collective -- no overlap in that combination; the K-step ring (TBX_OPT_GATHER_EVERY > 1), the two-launch loop or
 * overlapped fused launches (TBX_OPT_FUSED_OVERLAP: two output sets) overlap it. */
int tbx_gather(tbx_engine* engine, uint64_t* out_dev, void* stream);
/* Make `stream` wait for the last queued gather (device-side consumers of the gathered records). */
int tbx_gather_wait(tbx_engine* engine, void* stream);
/* Block until the last queued gather has finished and copy TBX_BUF_GATHERED to the host: uint64[nranks * K * records_per_rank]
 * (K = tbx_gather_every, 1 by default). */
int tbx_gather_host(tbx_engine* engine, uint64_t* out_host);
/* Blocking max-reduction of one double over all ranks (barrier + "slowest rank" timing of bench.py). */
int tbx_gather_reduce_max(tbx_engine* engine, double* inout_host);
#define TBX_BUF_GATHERED 12   /* uint64[nranks][K][records_per_rank] result of tbx_gather(out_dev = NULL) */

/* Address of an engine-owned device buffer (TBX_BUF_*).  In pipelined mode (TBX_OPT_PIPELINE) the step outputs and the
 * engine-owned frame buffer each alternate between two addresses: ask again after every step / render. */
int tbx_device_buffer(tbx_engine* engine, int which, void** out_ptr, size_t* out_bytes);

/* ------------------------------------------------------------------ engine options
 * Launch-time choices that used to be environment variables.  Every non-default path they select has a parity test against
 * the oracle (tests/test_gpu_paths.py, tests/test_preproc.py).  Unknown options / values: TBX_E_INVALID.
 *
 * TBX_OPT_PIPELINE -- random-rollout loops (tbx_step_synthetic + tbx_render_device) only; 0 = off (default).
 *   A step whose actions are generated on the device depends on nothing the previous frame's rasteriser produces, and a
 *   rasteriser that reads step-written render records (Breakout, SpaceInvaders) disturbs nothing the next step touches.  With the option
 *   on, such engines keep TWO sets of render records, of step outputs (TBX_BUF_REWARD / DONE / LIVES / SCORE / PACKED) and
 *   -- for tbx_render_device(out_dev = NULL) -- of TBX_BUF_FRAME, and run the calls on internal streams:
 *     value 2: tbx_step_synthetic N+1 runs beside the rasteriser of frame N;
 *     value 3: additionally consecutive rasteriser launches alternate between two internal streams and the two frame
 *              buffers, so that launch N+1 fills the ramp-down of launch N (small batches: BASELINE configs 2-4, the
 *              per-GPU share of a strong-scaled batch);
 *     value 1: the engine's choice: value 3 for Breakout from 4 096 to 16 383 envs and for SpaceInvaders below 16 384 envs while
 *              no per-step gather is initialised (BASELINE configs 2-4: 0.0985 -> 0.0868 ms and 0.162 -> 0.150 ms per step at
 *              4 096 envs), 0 otherwise.  (Rounds 2-3 chose 2 for large batches, 1-15 % faster "depending on the box": what it
 *              bought was a rasteriser launch that does not start against an idle memory system, and the rasterisers now see to
 *              that themselves -- csrc/raster.hpp, tbx_stagger_first_waves; scripts/pipeline_sweep.py, 16 384 .. 65 536 envs:
 *              stream order 0.5-3 % ahead of value 2.  Value 3 loses with a gather: 0.230 against 0.175 ms at 8 192 envs.)
 *   Contract in this mode: the stream a call names still waits for the call's work, so anything queued on it afterwards sees
 *   the result; the result of step N (render N) stays valid for readers queued on that stream BEFORE step N+1 (render N+1)
 *   is issued -- the same rule as without the option -- but it lives at the address tbx_device_buffer reports after the
 *   call, which alternates.  Every other call on the handle first joins the pipeline.  Engines whose rasteriser reads live
 *   state (Amidar, GridWorld, Breakout with intervention-written bricks, SpaceInvaders with intervention-written enemy
 *   positions) ignore the option.  (Round 3 let Amidar take part through a record kernel behind its step: slower than stream
 *   order at every size -- its step, a chain of dependent loads, runs ten times longer beside a rasteriser -- and removed.) */
#define TBX_OPT_PIPELINE      0
/* batch step kernel form of Breakout and Amidar: 0 = the engine's choice (by batch size), 1 = one thread per env, 2 = one
 * wavefront per env */
#define TBX_OPT_STEP_FORM     1
/* waves per frame of the rasteriser launches: 0 = the engine's choice (by game, channels and batch size) */
#define TBX_OPT_RENDER_SPLIT  2
/* 1: the agent observation goes through two full-resolution gray renders and the generic warp kernel instead of the per-game
 * fused kernels (the cross-check path); read by tbx_agent_init */
#define TBX_OPT_AGENT_GENERIC 3
/* 1 (default): tbx_step1 on a one-env engine talks to the resident step kernel; 0: single-env launch + read-back */
#define TBX_OPT_RESIDENT_STEP 4
/* K-step record ring of the multi-GPU gather, 1..64 (default 1 = one collective per step).  Read by tbx_gather_init (like
 * TBX_OPT_AGENT_GENERIC by tbx_agent_init; a later change takes effect at the next tbx_gather_init).  SURVEY.md 8e: "one
 * ncclAllGather per step (or per K steps)" -- and what the reference's learners consume is a K-step rollout anyway: the A2C
 * runner collects nsteps = 5 steps of (obs, rewards, dones) per update, PPO2 128 (baselines/baselines/a2c/runner.py:16,
 * a2c/a2c.py:87, ppo2/ppo2.py:103).  With K > 1 the step kernels write their 8-byte records straight into slot j of a ring
 * [K][records_per_rank] (j = steps since the last collective; TBX_BUF_PACKED names the slot of the most recent step), tbx_gather
 * only counts -- no stream operation at all -- and every K-th call sends the whole ring with ONE ncclAllGather of
 * K * records_per_rank records; the following K steps fill a second ring meanwhile.  Gathered layout
 * [nranks][K][records_per_rank] (TBX_BUF_GATHERED, tbx_gather_host).  The pipelined mode is off while a ring is in force. */
#define TBX_OPT_GATHER_EVERY  5
/* how the record gather travels, read by tbx_gather_init: 0 (default) = RCCL (ncclAllGather over xGMI); 1 = host-staged over a
 * POSIX shared-memory segment named after the id -- the ranks of ONE node, no librccl needed ("a host-staged
 * gather is the fallback if RCCL is missing").  Same calls, same gathered layout, same ordering rules; but every collective
 * blocks the calling thread until the step that wrote the records has finished and all ranks have exchanged them.  It also lets
 * several ranks share ONE device (RCCL refuses two ranks of a communicator on one GPU): `bench.py --gather host --one-device`
 * walks the whole N-process flow on a one-GPU box.  tbx_gather_library() names the transport in use. */
#define TBX_OPT_GATHER_TRANSPORT 6
/* Consecutive tbx_render_step_synthetic(out_dev = NULL) calls of an engine whose call is ONE launch (TBX_OPT_RENDER_STEP_FUSED):
 * 0 (default) = the engine's choice by batch size, 1 = overlap them, 2 = stream order.
 *   Launch N+1 needs only what the STEP BLOCKS of launch N write (state, render records, outputs) -- the first few blocks of a
 *   launch that otherwise paints for 70 .. 1 200 us.  Overlapped, consecutive launches alternate between two internal streams,
 *   the two sets of step outputs and two engine-owned frame buffers (as in the pipelined mode), over THREE buffers of render
 *   records, and launch N+1 is ordered behind a device counter that the step blocks of launch N bump once their stores are
 *   visible device-wide: a one-wave kernel in front of launch N+1 waits for it (bounded; a time-out is reported by tbx_sync as
 *   TBX_E_NO_DEVICE), the launch itself never spins.  So launch N+1 ramps up in the ramp-down of launch N -- what N worker
 *   processes stepping independently of each other give the reference (baselines/baselines/common/vec_env/subproc_vec_env.py:49-74),
 *   and what the per-GPU share of a strong-scaled batch (8 192 envs) loses between launches in stream order.  It works with the
 *   record gather in both forms (one collective per step: the collective of step N then runs beside launch N+1; K-step ring).
 *   Contract: TBX_BUF_FRAME / TBX_BUF_REWARD ... alternate between two addresses -- ask tbx_device_buffer after every call whose
 *   results are to be read -- and it is THAT call which makes the stream the step call named wait for the launch that wrote
 *   them (the stream joins lazily: a loop that only rolls, or whose only consumer is the record gather, queues nothing on the
 *   caller's stream -- with a gather on the device a wait and a fence per call there cost more than the overlap gains).  The
 *   results of call N stay valid for readers queued on that stream after tbx_device_buffer and before call N+1.  A call with
 *   out_dev != NULL, or any other call on the handle, first joins everything (program order holds as everywhere). */
#define TBX_OPT_FUSED_OVERLAP 7
/* How early an overlapped launch is released, in blocks of the launch before it: launch N+1 starts once the step blocks of
 * launch N are through AND the block `lead` blocks before the end of launch N's grid has STARTED (blocks start in index order:
 * from there on launch N only drains).  0 = the engine's choice; 1 .. 2^20 blocks; a value beyond the grid releases launch N+1
 * as soon as the step blocks are through (both launches then run side by side for most of their length -- measured slower,
 * profiles/r06_experiments.txt). */
#define TBX_OPT_FUSED_OVERLAP_LEAD 8
/* tbx_rollout_synthetic as ONE step launch + the chunk's rasteriser launches on internal streams (see there): 0 (default) = the
 * engine's choice by batch size, 1 = wherever the engine can (the rasteriser form its choice), 2 = never (the k single calls in
 * stream order); 3 / 4 = as 1 with the rasteriser form named -- 3 a launch per frame on two streams, 4 one launch per chunk on one
 * (games without that form: as 3) */
#define TBX_OPT_ROLLOUT_CHUNKS 9
#define TBX_OPT_COUNT         10
/* read-only (tbx_get_option): what TBX_OPT_PIPELINE resolves to on this engine right now -- 0, 2 or 3 */
#define TBX_OPT_PIPELINE_ACTIVE 100
/* read-only: 1 while the rasteriser reads step-written render records (Breakout with the canonical wall, SpaceInvaders with
 * the canonical formation), 0 once an intervention has switched the engine to the state-reading rasteriser, or for games
 * without records */
#define TBX_OPT_RECORDS_ACTIVE  101
/* read-only: 1 if tbx_render_step_synthetic(channels = 3) is ONE launch on this engine right now (the rasteriser reads
 * step-written records and the game has a fused kernel), 0 if it is the two launches in stream order */
#define TBX_OPT_RENDER_STEP_FUSED 102
/* read-only: 1 if tbx_render_step_synthetic(out_dev = NULL, channels = 3) would be an overlapped launch right now
 * (TBX_OPT_FUSED_OVERLAP resolved), 0 if it runs in stream order */
#define TBX_OPT_FUSED_OVERLAP_ACTIVE 103
/* read-only: 1 if tbx_rollout_synthetic(channels = 3) would run as overlapped chunks right now, 0 if as single calls */
#define TBX_OPT_ROLLOUT_CHUNKS_ACTIVE 104
/* read-only: into how many chunks the last TBX_QUERY_LOOKAHEAD_SEARCH cut every (env, first action) group of plans (0: none yet) */
#define TBX_OPT_SEARCH_CHUNKS 105
/* read-only: into how many chunks the last TBX_QUERY_LOOKAHEAD_SAMPLES cut the samples of every (env, first action) group (0: none yet) */
#define TBX_OPT_SAMPLE_CHUNKS 106
/* read-only: into how many chunks the last TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES cut the suffix codes of every (env, first action)
 * group, and into how many launches over env ranges it was cut (0: none yet) */
#define TBX_OPT_SEARCH_SAMPLES_CHUNKS 107
#define TBX_OPT_SEARCH_SAMPLES_LAUNCHES 108
/* read-only: into how many env ranges the last TBX_QUERY_LOOKAHEAD_BEAM was cut (0: none yet; a refused query leaves it standing) */
#define TBX_OPT_BEAM_RANGES 109
/* at most this many envs per range of a TBX_QUERY_LOOKAHEAD_BEAM, on top of the engine's budgets; 0 (default): the engine's choice.
 * It changes no output bit.  It caps the ranges of a TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES too. */
#define TBX_OPT_BEAM_RANGE_ENVS 110
/* read-only: into how many env ranges the last TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES was cut, and the largest number of sample chunks
 * any of its levels used (0: none yet; a refused query leaves both standing) */
#define TBX_OPT_BEAM_SAMPLES_RANGES 111
#define TBX_OPT_BEAM_SAMPLES_CHUNKS 112
/* at most this many sample chunks per level of a TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES; 0 (default): the engine's choice, 1: never cut.
 * It changes no output bit. */
#define TBX_OPT_BEAM_SAMPLES_MAX_CHUNKS 113
/* read-only: into how many env ranges the last TBX_QUERY_LOOKAHEAD_EVOLVE was cut (0: none yet; a refused query leaves it standing) */
#define TBX_OPT_EVOLVE_RANGES 114
/* read-only: into how many env ranges the last TBX_QUERY_LOOKAHEAD_TREE was cut (0: none yet; a refused query leaves it standing) */
#define TBX_OPT_TREE_RANGES 115
/* at most this many simulations per launch of a TBX_QUERY_LOOKAHEAD_TREE (0 .. TBX_TREE_MAX_SIMULATIONS), on top of the engine's
 * budget; 0 (default): the engine's choice.  It changes no output bit. */
#define TBX_OPT_TREE_LAUNCH_SIMULATIONS 116
/* for tests of the carry of TBX_QUERY_LOOKAHEAD_TREE_ACT; neither changes anything at its default.
 * at most this many nodes of a subtree are carried: 0 (default) means simulations + 1.  The option is set before a call names its
 * `simulations`, so tbx_set_option accepts 1 .. TBX_TREE_MAX_SIMULATIONS + 1 and a call carries min(value, simulations + 1). */
#define TBX_OPT_TREE_CARRY_KEEP 117
/* the halving threshold of the carry: 0 (default) means TBX_TREE_CARRY_MAX_VISITS, otherwise 1 .. TBX_TREE_CARRY_MAX_VISITS */
#define TBX_OPT_TREE_CARRY_MAX_VISITS 118
int tbx_set_option(tbx_engine* engine, int option, int value);
int tbx_get_option(tbx_engine* engine, int option, int* value_out);
/* Block until all work queued by this engine has finished, and report what the asynchronous calls since the last report could
 * not return themselves: the device keeps ONE error word for all of them, read and cleared here (and by the synchronous forms,
 * which report it as their own return code).  In order of precedence, one code per call:
 *   TBX_E_NO_DEVICE    an overlapped fused launch timed out waiting for the launch before it (TBX_OPT_FUSED_OVERLAP);
 *   TBX_E_NEEDS_RESET  an agent step ran on an env that needed a reset (tbx_agent_step_device / _synthetic);
 *   TBX_E_ACTION       an illegal ALE action id was seen (any "_dev" step) and played as NOOP.
 * So when the steps since the last report had both an illegal id and an env that needed a reset, TBX_E_NEEDS_RESET is what
 * comes back, and the illegal id is not reported again later.  Every step has been carried out either way. */
int tbx_sync(tbx_engine* engine);

#ifdef __cplusplus
}
#endif
#endif /* TOYBOX_AMD_H */
