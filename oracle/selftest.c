/* selftest.c -- drives the CPU restatement through the C-ABI under AddressSanitizer + UBSan (`make -C oracle sanitize`).
 * TEST INFRASTRUCTURE ONLY.  GPU sanitizers are unavailable on this pool, so the checker itself is what gets sanitized:
 * rollouts of every game with auto-reset, all frame formats, state round trips, the agent layer with every wrapper on, and the
 * written states of tests/test_gpu_rule_edges.py whose values sit where a conversion or an index could leave its range. */
#include "oracle.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #x, rc_, tbx_last_error(e)); return 1; } } while (0)

static int run_game(int game, int n, int steps)
{
    tbx_engine* e = NULL;
    if (tbx_create(game, n, 0, NULL, 0, &e)) { fprintf(stderr, "create failed for game %d\n", game); return 1; }
    int h, w;
    CHECK(tbx_frame_dims(game, &h, &w));
    CHECK(tbx_seed(e, -1, 1234));
    CHECK(tbx_new_game(e, NULL));
    int32_t* actions = (int32_t*)malloc((size_t)n * 4);
    int32_t* reward = (int32_t*)malloc((size_t)n * 4);
    uint8_t* done = (uint8_t*)malloc((size_t)n);
    uint8_t* frame = (uint8_t*)malloc((size_t)n * h * w * 4);
    const size_t ssz = tbx_state_size(game);
    char* st = (char*)malloc(ssz * (size_t)n);
    long dones = 0;
    for (int t = 0; t < steps; t++) {
        for (int i = 0; i < n; i++) actions[i] = orc_synthetic_action(game, 1337, (uint64_t)i, (uint64_t)t);
        CHECK(tbx_step(e, actions, TBX_STEP_AUTO_RESET, reward, done, NULL, NULL));
        for (int i = 0; i < n; i++) dones += done[i];
        if (t % 97 == 0) {
            for (int c = 1; c <= 4; c += (c == 1 ? 2 : 1)) CHECK(tbx_render(e, frame, c));
            CHECK(orc_render_envs(e, n / 3, n - n / 3, frame, 4));
            CHECK(tbx_get_states(e, 0, n, st, ssz));
            CHECK(tbx_set_states(e, 0, n, st, ssz));
        }
    }
    /* the agent layer with every wrapper on */
    tbx_agent_config_t ac;
    memset(&ac, 0, sizeof ac);
    ac.skip = 4; ac.out_h = 84; ac.out_w = 84; ac.stack = 4; ac.clip_reward = 1;
    ac.episodic_life = 1; ac.fire_reset = 1; ac.noop_max = 30; ac.noop_seed = 7; ac.env_offset = 11;
    CHECK(tbx_agent_init(e, &ac));
    uint8_t* obs = (uint8_t*)malloc((size_t)n * 84 * 84 * 4);
    float* ar = (float*)malloc((size_t)n * 4);
    CHECK(tbx_agent_reset(e, obs));
    for (int t = 0; t < steps / 4; t++) {
        for (int i = 0; i < n; i++) actions[i] = orc_synthetic_action(game, 99, (uint64_t)i, (uint64_t)t);
        CHECK(tbx_agent_step(e, actions, ar, done, obs));
        CHECK(tbx_agent_episodes(e, done, ar, reward));
    }
    printf("game %d: %d envs x %d frames ok (%ld episode ends)\n", game, n, steps, dones);
    free(actions); free(reward); free(done); free(frame); free(st); free(obs); free(ar);
    tbx_destroy(e);
    return 0;
}

/* Breakout states a caller may write (tbx_set_state takes any binary64): env i of 16 gets one of
 *   0 paddle_width 0 with the ball coming down exactly onto paddle_x  -- (x - left) / width is 0 / 0, segment 0 by SPEC.md
 *   1 radius 0 and -1 with a launched ball
 *   2 paddle, ball and brick rectangles at +-1e6 +- 1, +-1e300, +-inf, and inf - inf for the paddle's left edge
 *   3 an indestructible brick in the ball's way
 * then every frame format, four frames of every action, the frames again. */
static int breakout_written_states(void)
{
    enum { N = 16 };
    static const double X[10] = {1e6 - 1, 1e6, 1e6 + 1, -1e6 + 1, -1e6, -1e6 - 1, 1e300, -1e300, INFINITY, -INFINITY};
    static const int32_t ACT[4] = {0, 1, 3, 4};
    tbx_engine* e = NULL;
    if (tbx_create(TBX_GAME_BREAKOUT, N, 0, NULL, 0, &e)) { fprintf(stderr, "create failed for the written Breakout states\n"); return 1; }
    CHECK(tbx_seed(e, -1, 5));
    CHECK(tbx_new_game(e, NULL));
    tbx_breakout_state_t* s = (tbx_breakout_state_t*)malloc(sizeof *s);
    for (int i = 0; i < N; i++) {
        CHECK(tbx_get_state(e, i, s, sizeof *s));
        s->is_dead = s->reset = 0;
        s->n_balls = 1;
        s->ball_x[0] = 60.0 + i; s->ball_y[0] = 100.0; s->ball_vx[0] = 0.5; s->ball_vy[0] = 1.0;
        switch (i % 4) {
        case 0:
            s->paddle_width = 0.0; s->paddle_speed = 0.0; s->paddle_x = 20.0 + 9.5 * i;
            s->ball_x[0] = s->paddle_x; s->ball_y[0] = s->paddle_y - 3.0; s->ball_vx[0] = 0.0; s->ball_vy[0] = 1.0 + 0.25 * (i / 4);
            break;
        case 1:
            s->ball_radius = (i & 4) ? 0.0 : -1.0;
            s->ball_x[0] = 18.0 + 12.0 * i; s->ball_y[0] = 68.5; s->ball_vx[0] = 0.5; s->ball_vy[0] = -3.0;
            break;
        case 2:
            s->paddle_x = X[i % 10]; s->paddle_width = (i & 8) ? INFINITY : X[(3 * i + 1) % 10];
            if (i & 8) s->paddle_x = INFINITY;
            s->n_balls = 2;
            s->ball_x[0] = X[(7 * i + 2) % 10];
            s->ball_x[1] = 100.0; s->ball_y[1] = X[(i + 5) % 10]; s->ball_vx[1] = -0.75; s->ball_vy[1] = -1.0;
            s->ball_radius = X[(i / 4 + 6) % 10];
            s->bricks[0].x = X[(i + 3) % 10]; s->bricks[0].w = X[(3 * i + 4) % 10];
            s->bricks[1].y = X[(i + 6) % 10]; s->bricks[1].h = X[(7 * i) % 10];
            s->bricks[2].x = -1e6 - 1; s->bricks[2].w = 1e6 + 40;
            break;
        default:
            s->bricks[6 * i + 5].destructible = 0;
            s->ball_x[0] = s->bricks[6 * i + 5].x + 6.0; s->ball_y[0] = s->bricks[6 * i + 5].y + 6.5; s->ball_vx[0] = 0.25; s->ball_vy[0] = -2.0;
        }
        CHECK(tbx_set_state(e, i, s, sizeof *s));
    }
    int h, w;
    CHECK(tbx_frame_dims(TBX_GAME_BREAKOUT, &h, &w));
    uint8_t* frame = (uint8_t*)malloc((size_t)N * h * w * 4);
    int32_t actions[N], reward[N];
    uint8_t done[N];
    for (int t = 0; t <= 4; t++) {
        for (int c = 1; c <= 4; c += (c == 1 ? 2 : 1)) CHECK(tbx_render(e, frame, c));
        for (int i = 0; i < N; i++) actions[i] = ACT[(i / 4 + t) % 4];
        CHECK(tbx_step(e, actions, TBX_STEP_AUTO_RESET, reward, done, NULL, NULL));
    }
    printf("breakout: %d written states x 5 frames ok\n", N);
    free(frame); free(s);
    tbx_destroy(e);
    return 0;
}

/* SpaceInvaders states of the same module: env i of 12 gets one of
 *   0 enemy lasers and the ship's laser flying LEFT and RIGHT off their sides    1 the ship's laser at the ground line
 *   2 a full laser table when the enemies' shot comes due                         3 no enemy at all (n_enemies 0)
 *   4 a ship neither alive nor exploding                                          5 ufo_appearance_counter -1 */
static int si_written_states(void)
{
    enum { N = 12 };
    static const int32_t ACT[6] = {0, 1, 3, 4, 11, 12};
    tbx_engine* e = NULL;
    if (tbx_create(TBX_GAME_SPACE_INVADERS, N, 0, NULL, 0, &e)) { fprintf(stderr, "create failed for the written SpaceInvaders states\n"); return 1; }
    CHECK(tbx_seed(e, -1, 5));
    CHECK(tbx_new_game(e, NULL));
    tbx_si_state_t* s = (tbx_si_state_t*)malloc(sizeof *s);
    for (int i = 0; i < N; i++) {
        CHECK(tbx_get_state(e, i, s, sizeof *s));
        s->life_display_timer = 0; s->ship_alive = 1; s->ship_death_counter = -1;
        s->enemy_shot_delay = 40; s->move_counter = 20;
        const int far = i >= 6;
        switch (i % 6) {
        case 0:
            s->n_enemy_lasers = TBX_SI_MAX_LASERS;
            for (int k = 0; k < TBX_SI_MAX_LASERS; k++) {
                tbx_si_laser_t* l = &s->enemy_lasers[k];
                l->movement = (k & 1) ? TBX_DIR_RIGHT : TBX_DIR_LEFT;
                l->x = (k & 1) ? TBX_SI_W - 1 - k : k - 1; l->y = 40 + 9 * k; l->w = 2; l->h = 8; l->speed = 1 + k % 3;
            }
            s->has_ship_laser = 1;
            s->ship_laser.movement = far ? TBX_DIR_RIGHT : TBX_DIR_LEFT; s->ship_laser.x = far ? TBX_SI_W - 2 : 1;
            s->ship_laser.y = 20; s->ship_laser.w = 2; s->ship_laser.h = 8; s->ship_laser.speed = 2;
            break;
        case 1:
            s->has_ship_laser = 1;
            s->ship_laser.movement = far ? TBX_DIR_DOWN : TBX_DIR_UP; s->ship_laser.x = 100; s->ship_laser.y = far ? 190 : 203;
            s->ship_laser.w = 2; s->ship_laser.h = 8; s->ship_laser.speed = 6;
            break;
        case 2:
            s->n_enemy_lasers = TBX_SI_MAX_LASERS;
            for (int k = 0; k < TBX_SI_MAX_LASERS; k++) {
                tbx_si_laser_t* l = &s->enemy_lasers[k];
                l->movement = TBX_DIR_DOWN; l->x = 2 + 3 * k; l->y = 30 + 5 * k; l->w = 2; l->h = 8; l->speed = 1;
            }
            s->enemy_shot_delay = 1 + far;
            break;
        case 3:
            s->n_enemies = 0; s->move_counter = 1; s->enemy_shot_delay = 1;
            break;
        case 4:
            s->ship_alive = 0;
            break;
        default:
            s->ufo_appearance_counter = -1; s->ufo_x = far ? 400 : -30;
        }
        CHECK(tbx_set_state(e, i, s, sizeof *s));
    }
    int h, w;
    CHECK(tbx_frame_dims(TBX_GAME_SPACE_INVADERS, &h, &w));
    uint8_t* frame = (uint8_t*)malloc((size_t)N * h * w * 4);
    int32_t actions[N], reward[N];
    uint8_t done[N];
    for (int t = 0; t <= 4; t++) {
        for (int c = 1; c <= 4; c += (c == 1 ? 2 : 1)) CHECK(tbx_render(e, frame, c));
        for (int i = 0; i < N; i++) actions[i] = ACT[(i + t) % 6];
        CHECK(tbx_step(e, actions, TBX_STEP_AUTO_RESET, reward, done, NULL, NULL));
    }
    printf("space_invaders: %d written states x 5 frames ok\n", N);
    free(frame); free(s);
    tbx_destroy(e);
    return 0;
}

/* Amidar states of the same module: env i of 12 gets one of
 *   0 route index 99 / -1, ai.next 99 / -1, a caught enemy of route 99 put back when the chase ends   1 speed -3, ai.kind 7, movers off their corner
 *   2 movers at negative world coordinates, one on the corner of tile (-1, 0)                          3 the player arriving with a history of -5 / 5000 / nothing
 *   4 the player walking onto a tile that is no track                                                   5 enemies of every protocol alone on their tile */
static int amidar_written_states(void)
{
    enum { N = 12 };
    tbx_engine* e = NULL;
    if (tbx_create(TBX_GAME_AMIDAR, N, 0, NULL, 0, &e)) { fprintf(stderr, "create failed for the written Amidar states\n"); return 1; }
    CHECK(tbx_seed(e, -1, 5));
    CHECK(tbx_new_game(e, NULL));
    tbx_amidar_state_t* s = (tbx_amidar_state_t*)malloc(sizeof *s);
    for (int i = 0; i < N; i++) {
        CHECK(tbx_get_state(e, i, s, sizeof *s));
        const int far = i >= 6;
        tbx_amidar_mover_t* m = s->enemies;
        switch (i % 6) {
        case 0:
            m[0].ai.default_route_index = far ? -1 : 99;
            m[1].ai.next = far ? -1 : 99;
            m[2].ai.default_route_index = 99; m[2].caught = 1; m[2].x = 64 * 9; m[2].y = 80 * 12;
            s->chase_timer = 1 + far;
            break;
        case 1:
            m[0].speed = -3;
            m[1].ai.kind = far ? -1 : 7;
            m[2].x = 64 * 5 + 5; m[2].y = 80 * 6; m[2].step_tx = m[2].step_ty = -1;
            m[3].x = 64 * 5; m[3].y = 80 * 12 + 7; m[3].step_tx = m[3].step_ty = -1;
            s->player.x += 5;
            break;
        case 2:
            m[0].x = -21; m[1].y = -19; m[2].x = -1; m[2].y = -33;
            m[3].x = far ? -128 : -64; m[3].y = 0;
            for (int k = 0; k < 4; k++) m[k].step_tx = m[k].step_ty = -1;
            if (far) { s->player.x = -200; s->player.y = -100; s->player.step_tx = s->player.step_ty = -1; }
            break;
        case 3:
            s->player.x = 64 * 4 - 8; s->player.y = 80 * 12; s->player.step_tx = 4; s->player.step_ty = 12;
            s->player.n_history = far ? 0 : 1; s->player.history[0] = far ? 5000 : -5;
            break;
        case 4:
            s->player.x = 64 * 4; s->player.y = 80 * 13 - 8; s->player.step_tx = 4; s->player.step_ty = 13;
            break;
        default:
            s->tiles[12][6] = s->tiles[12][8] = s->tiles[6][6] = s->tiles[6][8] = s->tiles[24][8] = s->tiles[24][10] = TBX_TILE_EMPTY;
            for (int k = 0; k < 4; k++) {
                memset(&m[k].ai, 0, sizeof m[k].ai);
                m[k].ai.kind = TBX_AI_PERIMETER + k; m[k].ai.dir = TBX_DIR_RIGHT; m[k].ai.horiz = TBX_DIR_RIGHT;
                m[k].step_tx = m[k].step_ty = -1; m[k].n_history = 0;
            }
            m[0].x = 64 * 31; m[0].y = 80 * 30; m[1].x = 64 * 7; m[1].y = 80 * 12; m[2].x = 64 * 7; m[2].y = 80 * 6; m[3].x = 64 * 9; m[3].y = 80 * 24;
            s->tiles[30][30] = s->tiles[29][31] = far ? TBX_TILE_EMPTY : TBX_TILE_UNPAINTED;
        }
        CHECK(tbx_set_state(e, i, s, sizeof *s));
    }
    int h, w;
    CHECK(tbx_frame_dims(TBX_GAME_AMIDAR, &h, &w));
    uint8_t* frame = (uint8_t*)malloc((size_t)N * h * w * 4);
    int32_t actions[N], reward[N];
    uint8_t done[N];
    for (int t = 0; t <= 4; t++) {
        for (int c = 1; c <= 4; c += (c == 1 ? 2 : 1)) CHECK(tbx_render(e, frame, c));
        for (int i = 0; i < N; i++) actions[i] = (i + t) % 6;
        CHECK(tbx_step(e, actions, TBX_STEP_AUTO_RESET, reward, done, NULL, NULL));
    }
    printf("amidar: %d written states x 5 frames ok\n", N);
    free(frame); free(s);
    tbx_destroy(e);
    return 0;
}

/* GridWorld states of the same module: cells whose number names no tile (7 and 200 with four tiles), a border of floor, a board cut
 * to 5 x 4 with the player outside it, a player one cell off every side, a game already over */
static int gridworld_written_states(void)
{
    enum { N = 12 };
    static const int32_t ACT[5] = {0, 2, 3, 4, 5};
    tbx_engine* e = NULL;
    if (tbx_create(TBX_GAME_GRIDWORLD, N, 0, NULL, 0, &e)) { fprintf(stderr, "create failed for the written GridWorld states\n"); return 1; }
    CHECK(tbx_new_game(e, NULL));
    tbx_gridworld_state_t* s = (tbx_gridworld_state_t*)malloc(sizeof *s);
    for (int i = 0; i < N; i++) {
        CHECK(tbx_get_state(e, i, s, sizeof *s));
        for (int y = 0; y < 7; y++)
            for (int x = 0; x < 9; x++) {
                const int r = (x * 7 + y * 3 + i) % 10;
                s->grid[y * TBX_GW_MAX_DIM + x] = (uint8_t)(r < 4 ? 0 : r == 4 ? 1 : r < 7 ? 3 : r == 7 ? 2 : r == 8 ? 7 : 200);
            }
        if (i % 4 == 3) { s->width = 5; s->height = 4; }
        s->player_x = (i % 3 == 0) ? -1 : (i % 3 == 1) ? 9 : i % 9;
        s->player_y = (i % 5 == 0) ? -1 : (i % 5 == 1) ? 7 : i % 7;
        s->game_over = i == 5;
        s->reward_becomes = i % 2;
        CHECK(tbx_set_state(e, i, s, sizeof *s));
    }
    int h, w;
    CHECK(tbx_frame_dims(TBX_GAME_GRIDWORLD, &h, &w));
    uint8_t* frame = (uint8_t*)malloc((size_t)N * h * w * 4);
    int32_t actions[N], reward[N];
    uint8_t done[N];
    for (int t = 0; t <= 4; t++) {
        for (int c = 1; c <= 4; c += (c == 1 ? 2 : 1)) CHECK(tbx_render(e, frame, c));
        for (int i = 0; i < N; i++) actions[i] = ACT[(i + t) % 5];
        CHECK(tbx_step(e, actions, TBX_STEP_AUTO_RESET, reward, done, NULL, NULL));
    }
    printf("gridworld: %d written states x 5 frames ok\n", N);
    free(frame); free(s);
    tbx_destroy(e);
    return 0;
}

int main(void)
{
    int rc = 0;
    rc |= breakout_written_states();
    rc |= si_written_states();
    rc |= amidar_written_states();
    rc |= gridworld_written_states();
    rc |= run_game(TBX_GAME_BREAKOUT, 12, 2000);
    rc |= run_game(TBX_GAME_SPACE_INVADERS, 6, 2000);
    rc |= run_game(TBX_GAME_AMIDAR, 6, 2000);
    rc |= run_game(TBX_GAME_GRIDWORLD, 16, 1000);
    return rc;
}
