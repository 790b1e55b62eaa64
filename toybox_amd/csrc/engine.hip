// engine.hip -- the C-ABI of include/toybox_amd.h over the per-game gfx950 kernels.
// No CPU fallback: every entry point that computes needs a visible gfx950 device.

#include "engine_host.hpp"
#include "envcopy.hpp"
#include "pipeline.hpp"
#include <emmintrin.h>   // host side only: tbx_host_stack_push

#include <sched.h>
#include <thread>
#include <vector>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

int tbx_agent_buffer(tbx_engine* e, int which, void** out_ptr, size_t* out_bytes);

namespace {

thread_local std::string g_create_error;

}  // namespace

void tbx_set_create_error(const std::string& msg) { g_create_error = msg; }

void tbx_set_out_parity(tbx_engine* e, int p)
{
    e->out_par = p;
    e->reward = e->outs[p].reward;
    e->done = e->outs[p].done;
    e->lives_out = e->outs[p].lives;
    e->score_out = e->outs[p].score;
    e->packed = e->outs[p].packed;
    if (e->ops) e->ops->rebind_outputs(e);
}

// TBX_BUF_PACKED leaves a chunk's record array (tbx_use_stream): the records it names are copied into the current output set on s,
// which the caller has ordered behind the chunk's step launch, and the step kernels write there again.  TBX_BUF_ROLLOUT_PACKED keeps
// all k rows of the chunk.
hipError_t tbx_packed_leaves_chunk(tbx_engine* e, hipStream_t s)
{
    uint64_t* own = e->outs[e->out_par].packed;
    hipError_t r = hipMemcpyAsync(own, e->packed, sizeof(uint64_t) * (size_t)e->n, hipMemcpyDeviceToDevice, s);
    if (r != hipSuccess) return r;
    e->packed = own;
    if (e->ops) e->ops->rebind_outputs(e);
    return hipSuccess;
}

int ensure_frame(tbx_engine* e, size_t bytes)
{
    EHIP(e->frame_own.reserve(bytes));
    e->frame = e->frame_own.p;
    e->frame_bytes = bytes;                                    // TBX_BUF_FRAME: the size of the frame it names, not of the allocation
    return TBX_OK;
}

// the buffers of chunk parity q of tbx_rollout_synthetic: k frames and, unless a ring of the gather takes them, k rows of step records
int chunk_buffers(tbx_engine* e, int q, int k, size_t frame_bytes, bool want_packed, hipStream_t sync_a, hipStream_t sync_b)
{
    EHIP(e->rollout.frames[q].reserve((size_t)k * frame_bytes, sync_a, sync_b));
    if (want_packed) EHIP(e->rollout.packed[q].reserve(sizeof(uint64_t) * (size_t)k * (size_t)e->n, sync_a, sync_b));
    return TBX_OK;
}

namespace {

void breakout_default_config(tbx_breakout_config_t* c)
{
    memset(c, 0, sizeof *c);
    tbx_seed_state(13, c->rand[0], c->rand[1]);
    c->start_lives = 5;
    c->n_rows = 6;
    const int scores[6] = {7, 7, 4, 4, 1, 1};
    const uint8_t cols[6][3] = {{200, 72, 72}, {198, 108, 58}, {180, 122, 48}, {162, 162, 42}, {72, 160, 72}, {66, 72, 200}};
    for (int i = 0; i < 6; i++) {
        c->row_scores[i] = scores[i];
        c->row_colors[i] = tbx_color_t{cols[i][0], cols[i][1], cols[i][2], 255};
    }
    c->ball_speed_row_depth = 3;
    c->ball_speed_slow = 2.0;
    c->ball_speed_fast = 4.0;
    c->n_starts = 4;
    const double sx[4] = {24.0, 120.0, 120.0, 216.0}, sa[4] = {30.0, 30.0, 150.0, 150.0};
    for (int i = 0; i < 4; i++) {
        c->start_x[i] = sx[i]; c->start_y[i] = 80.0; c->start_angle_deg[i] = sa[i];
        const double rad = sa[i] * (M_PI / 180.0);
        c->start_dir_x[i] = std::cos(rad);   // host libm: the device never evaluates trig
        c->start_dir_y[i] = std::sin(rad);
    }
    c->paddle_discrete_segments = 5;
    for (int i = 0; i < 5; i++) {
        const double rad = (150.0 - (double)i * (120.0 / 4.0)) * (M_PI / 180.0);
        c->paddle_dir_x[i] = std::cos(rad);
        c->paddle_dir_y[i] = -std::sin(rad);
    }
    c->bg_color = tbx_color_t{0, 0, 0, 255};
    c->frame_color = tbx_color_t{144, 144, 144, 255};
    c->paddle_color = tbx_color_t{200, 72, 72, 255};
    c->ball_color = tbx_color_t{200, 72, 72, 255};
}

void si_default_config(tbx_si_config_t* c)
{
    memset(c, 0, sizeof *c);
    tbx_seed_state(17, c->rand[0], c->rand[1]);
    c->jitter = 0.5;
    c->start_lives = 3;
    c->n_rows = 6;
    c->n_shields = 3;
    c->enemy_protocol = 0;
    const int sc[6] = {30, 30, 20, 20, 10, 10}, sx[3] = {84, 148, 212};
    for (int i = 0; i < 6; i++) c->row_scores[i] = sc[i];
    for (int i = 0; i < 3; i++) { c->shield_x[i] = sx[i]; c->shield_y[i] = 157; }
}

// toybox/interventions/defaults/gridworld_config_default.json (tiles in the order of the dump's keys)
void gridworld_default_config(tbx_gridworld_config_t* c)
{
    static const char* const rows[7] = {"111111111", "1000R0001", "101111101", "100010001", "10001R111", "1000100G1", "111111111"};
    memset(c, 0, sizeof *c);
    c->width = 9; c->height = 7; c->n_tiles = 4;
    c->player_start_x = 2; c->player_start_y = 4;
    c->reward_becomes = 0;
    c->player_color = tbx_color_t{255, 0, 0, 255};
    const char keys[4] = {'0', '1', 'G', 'R'};
    const tbx_color_t colors[4] = {{255, 255, 255, 255}, {0, 0, 0, 255}, {0, 255, 0, 255}, {255, 255, 0, 255}};
    const int rewards[4] = {0, 0, 10, 1};
    for (int i = 0; i < 4; i++) {
        c->tile_keys[i] = (uint8_t)keys[i];
        c->tiles[i].color = colors[i];
        c->tiles[i].reward = rewards[i];
        c->tiles[i].goal = keys[i] == 'G';
        c->tiles[i].walkable = keys[i] != '1';
    }
    for (int y = 0; y < 7; y++)
        for (int x = 0; x < 9; x++)
            for (int i = 0; i < 4; i++)
                if (keys[i] == rows[y][x]) c->grid[y * TBX_GW_MAX_DIM + x] = (uint8_t)i;
}

void amidar_default_config(tbx_amidar_config_t* c)
{
    static const char* board[TBX_AMI_BOARD_H] = {
        "c========================c======", "=     =   =   =  =   =   =     =", "=     =   =   =  =   =   =     =",
        "=     =   =   =  =   =   =     =", "=     =   =   =  =   =   =     =", "=     =   =   =  =   =   =     =",
        "================================", "=   =    =  =      =  =    =   =", "=   =    =  =      =  =    =   =",
        "=   =    =  =      =  =    =   =", "=   =    =  =      =  =    =   =", "=   =    =  =      =  =    =   =",
        "================================", "=  =       =        =       =  p", "=  =       =        =       =  p",
        "=  =       =        =       =  p", "=  =       =        =       =  p", "=  =       =        =       =  p",
        "===============================p", "=    =        =  =        =    =", "=    =        =  =        =    =",
        "=    =        =  =        =    =", "=    =        =  =        =    =", "=    =        =  =        =    =",
        "c========================c======", "=     =     =      =     =     =", "=     =     =      =     =     =",
        "=     =     =      =     =     =", "=     =     =      =     =     =", "=     =     =      =     =     =",
        "================================"};
    memset(c, 0, sizeof *c);
    tbx_seed_state(13, c->rand[0], c->rand[1]);
    c->start_lives = 3; c->start_jumps = 4; c->jump_time = 75; c->chase_time = 300;
    c->box_bonus = 50; c->chase_score_bonus = 100;
    c->player_start_tx = 31; c->player_start_ty = 15;
    c->n_enemies = 5;
    c->render_images = 1; c->default_board_bugs = 1;
    for (int i = 0; i < 5; i++) {
        c->enemies[i].kind = TBX_AI_LOOKUP; c->enemies[i].default_route_index = i;
        c->enemies[i].seen_tx = c->enemies[i].seen_ty = -1;
    }
    c->bg_color = tbx_color_t{0, 0, 0, 255}; c->player_color = tbx_color_t{255, 255, 153, 255};
    c->unpainted_color = tbx_color_t{148, 0, 211, 255}; c->painted_color = tbx_color_t{255, 255, 30, 255};
    c->enemy_color = tbx_color_t{255, 50, 100, 255}; c->inner_painted_color = tbx_color_t{255, 255, 0, 255};
    for (int y = 0; y < TBX_AMI_BOARD_H; y++)
        for (int x = 0; x < TBX_AMI_BOARD_W; x++) {
            const char ch = board[y][x];
            c->board[y][x] = ch == '=' ? TBX_TILE_UNPAINTED : ch == 'p' ? TBX_TILE_PAINTED : ch == 'c' ? TBX_TILE_CHASE_MARKER : TBX_TILE_EMPTY;
        }
}

__global__ void seed_kernel(uint64_t* sim_rng, int n, int env, uint32_t seed)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (env >= 0 && i != env) return;
    uint64_t s0, s1;
    tbx_seed_state(env >= 0 ? seed : seed + (uint32_t)i, s0, s1);
    sim_rng[i] = s0;
    sim_rng[(size_t)n + i] = s1;
}

__global__ void seed_array_kernel(uint64_t* sim_rng, int n, const uint32_t* seeds)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t s0, s1;
    tbx_seed_state(seeds[i], s0, s1);
    sim_rng[i] = s0;
    sim_rng[(size_t)n + i] = s1;
}

// step outputs into one block for the host: [reward N | lives N | score N | err 1 | done N bytes]
__global__ void gather_outputs_kernel(const int32_t* reward, const int32_t* lives, const int32_t* score, const uint8_t* done,
                                      uint32_t* err_flag, int32_t* out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { out[3 * (size_t)n] = (int32_t)*err_flag; *err_flag = 0u; }
    if (i >= n) return;
    out[i] = reward[i]; out[(size_t)n + i] = lives[i]; out[2 * (size_t)n + i] = score[i];
    reinterpret_cast<uint8_t*>(out + 3 * (size_t)n + 1)[i] = done[i];
}

__global__ void fill_rng_kernel(uint64_t* sim_rng, int n, uint64_t s0, uint64_t s1)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sim_rng[i] = s0;
    sim_rng[(size_t)n + i] = s1;
}

int check_err_flag(tbx_engine* e)
{
    uint32_t f = 0;
    EHIP(hipMemcpyAsync(&f, e->err_flag, sizeof f, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    if (f) {
        EHIP(hipMemsetAsync(e->err_flag, 0, sizeof f, e->stream));
        if (f & 4u)
            return e->fail(TBX_E_NO_DEVICE, "an overlapped fused launch waited 3 s for the step blocks of the launch before it (TBX_OPT_FUSED_OVERLAP): results are not valid");
        if (f & 2u)
            return e->fail(TBX_E_NEEDS_RESET, "an env was stepped after its game ended inside EpisodicLifeEnv's no-op step (bench.Monitor raises here)");
        return e->fail(TBX_E_ACTION, "an illegal ALE action id was passed (treated as NOOP)");
    }
    return TBX_OK;
}

}  // namespace

extern "C" {

int tbx_abi_version(void) { return TBX_ABI_VERSION; }

const char* tbx_last_error(const tbx_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int tbx_frame_dims(int game, int* h, int* w)
{
    if (!h || !w) return TBX_E_INVALID;
    switch (game) {
    case TBX_GAME_BREAKOUT: *h = TBX_BRK_H; *w = TBX_BRK_W; return TBX_OK;
    case TBX_GAME_SPACE_INVADERS: *h = TBX_SI_H; *w = TBX_SI_W; return TBX_OK;
    case TBX_GAME_AMIDAR: *h = TBX_AMI_H; *w = TBX_AMI_W; return TBX_OK;
    case TBX_GAME_GRIDWORLD: *h = TBX_GW_H; *w = TBX_GW_W; return TBX_OK;
    default: return TBX_E_INVALID;
    }
}

int tbx_legal_actions(int game, int32_t* out, int cap)
{
    if (game < 0 || game >= TBX_NUM_GAMES) return TBX_E_INVALID;
    const int n = tbx_legal_count(game);
    for (int i = 0; i < n && i < cap; i++) out[i] = tbx_legal_action(game, i);
    return n;
}

int tbx_ale_action_to_buttons(int a)
{
    const uint32_t b = tbx_ale_buttons(a);
    return b == 0xFFu ? TBX_E_INVALID : (int)b;
}

size_t tbx_state_size(int game)
{
    switch (game) {
    case TBX_GAME_BREAKOUT: return sizeof(tbx_breakout_state_t);
    case TBX_GAME_SPACE_INVADERS: return sizeof(tbx_si_state_t);
    case TBX_GAME_AMIDAR: return sizeof(tbx_amidar_state_t);
    case TBX_GAME_GRIDWORLD: return sizeof(tbx_gridworld_state_t);
    default: return 0;
    }
}

size_t tbx_config_size(int game)
{
    switch (game) {
    case TBX_GAME_BREAKOUT: return sizeof(tbx_breakout_config_t);
    case TBX_GAME_SPACE_INVADERS: return sizeof(tbx_si_config_t);
    case TBX_GAME_AMIDAR: return sizeof(tbx_amidar_config_t);
    case TBX_GAME_GRIDWORLD: return sizeof(tbx_gridworld_config_t);
    default: return 0;
    }
}

int tbx_destroy(tbx_engine* e)
{
    if (!e) return TBX_OK;
    hipSetDevice(e->device);
    tbx_serve_stop(e);
    if (e->serve_stream) hipStreamDestroy(e->serve_stream);
    if (e->serve_ctl) hipHostFree(e->serve_ctl);
    if (e->serve_frame) hipHostFree(e->serve_frame);
    if (e->stream) hipStreamSynchronize(e->stream);
    pipe_drain(e);
    tbx_gather_free(e);
    tbx_agent_free(e);
    if (e->ops) { e->ops->destroy(e); delete e->ops; }
    hipFree(e->sim_rng); hipFree(e->prev_score);
    for (int k = 0; k < 2; k++) {
        hipFree(e->outs[k].reward); hipFree(e->outs[k].done); hipFree(e->outs[k].lives); hipFree(e->outs[k].score); hipFree(e->outs[k].packed);
        e->rollout.frames[k].release(); e->rollout.packed[k].release();
    }
    pipe_free(e);
    hipFree(e->actions);
    hipFree(e->plan_action); hipFree(e->plan_carry); e->act_scratch.release();
    hipFree(e->plan_tree); hipFree(e->plan_tree_drop);
    e->edit_args.release(); e->reduce_out.release(); e->search_parts.release(); e->sample_parts.release(); e->search_samples_parts.release(); e->beam_scratch.release(); envcopy_free(e); e->frame_own.release(); e->staging.release();
    hipFree(e->mask); hipFree(e->err_flag); hipFree(e->scal); hipFree(e->one_frame); hipFree(e->io_dev);
    if (e->io_host) hipHostFree(e->io_host);
    if (e->scal_host) hipHostFree(e->scal_host);
    if (e->order_ev) hipEventDestroy(e->order_ev);
    if (e->stream) hipStreamDestroy(e->stream);
    delete e;
    return TBX_OK;
}

int tbx_device_identity(tbx_engine* e, tbx_device_identity_t* out)
{
    CHECK_ENGINE(e);
    if (!out) return e->fail(TBX_E_INVALID, "out is NULL");
    hipDeviceProp_t prop;
    EHIP(hipGetDeviceProperties(&prop, e->device));
    memset(out, 0, sizeof *out);
    out->ordinal = e->device;
    out->pci_domain = prop.pciDomainID; out->pci_bus = prop.pciBusID; out->pci_device = prop.pciDeviceID;
    out->total_memory = (uint64_t)prop.totalGlobalMem;
    out->compute_units = prop.multiProcessorCount;
    snprintf(out->arch, sizeof out->arch, "%s", prop.gcnArchName);
    snprintf(out->name, sizeof out->name, "%s", prop.name);
    return TBX_OK;
}

int tbx_create(int game, int n_envs, int device, const void* config_pod, size_t config_size, tbx_engine** out)
{
    if (!out) return TBX_E_INVALID;
    *out = nullptr;
    if (n_envs < 1) { g_create_error = "n_envs must be >= 1"; return TBX_E_INVALID; }
    int ndev = 0;
    hipError_t he = hipGetDeviceCount(&ndev);
    if (he != hipSuccess || ndev < 1) {
        g_create_error = std::string("no HIP device visible (the engine has no CPU fallback): ") + hipGetErrorString(he);
        return TBX_E_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) { g_create_error = "device index out of range"; return TBX_E_INVALID; }
    hipDeviceProp_t prop;
    he = hipGetDeviceProperties(&prop, device);
    if (he != hipSuccess) { g_create_error = hipGetErrorString(he); return TBX_E_NO_DEVICE; }
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        g_create_error = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
        return TBX_E_NO_DEVICE;
    }
    tbx_engine* e = new (std::nothrow) tbx_engine();
    if (!e) { g_create_error = "out of host memory"; return TBX_E_NOMEM; }
    e->game = game;
    e->n = n_envs;
    e->device = device;
    int rc = TBX_OK;
    auto bail = [&](int code) {
        g_create_error = e->err;
        tbx_destroy(e);
        return code;
    };
    switch (game) {
    case TBX_GAME_BREAKOUT: e->ops = tbx_make_breakout_ops(); break;
    case TBX_GAME_SPACE_INVADERS: e->ops = tbx_make_si_ops(); break;
    case TBX_GAME_AMIDAR: e->ops = tbx_make_amidar_ops(); break;
    case TBX_GAME_GRIDWORLD: e->ops = tbx_make_gridworld_ops(); break;
    default: e->err = "unknown game id"; return bail(TBX_E_INVALID);
    }
    const size_t N = (size_t)n_envs;
#define CHIP(call)                                                                 \
    do {                                                                           \
        hipError_t _e = (call);                                                    \
        if (_e != hipSuccess) { hip_fail(e, #call, _e); return bail(_e == hipErrorOutOfMemory ? TBX_E_NOMEM : TBX_E_NO_DEVICE); } \
    } while (0)
    CHIP(hipSetDevice(device));
    CHIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    CHIP(hipMalloc((void**)&e->sim_rng, 2 * N * sizeof(uint64_t)));
    CHIP(hipMalloc((void**)&e->prev_score, N * sizeof(int32_t)));
    CHIP(hipMalloc((void**)&e->outs[0].reward, N * sizeof(int32_t)));
    CHIP(hipMalloc((void**)&e->outs[0].done, N));
    CHIP(hipMalloc((void**)&e->outs[0].lives, N * sizeof(int32_t)));
    CHIP(hipMalloc((void**)&e->outs[0].score, N * sizeof(int32_t)));
    CHIP(hipMalloc((void**)&e->outs[0].packed, N * sizeof(uint64_t)));
    tbx_set_out_parity(e, 0);
    CHIP(hipMalloc((void**)&e->actions, N * sizeof(int32_t)));
    CHIP(hipMalloc((void**)&e->mask, N));
    CHIP(hipMalloc((void**)&e->err_flag, sizeof(uint32_t)));
    CHIP(hipMalloc((void**)&e->scal, 3 * N * sizeof(int32_t)));
    CHIP(hipMemsetAsync(e->err_flag, 0, sizeof(uint32_t), e->stream));
    CHIP(hipMemsetAsync(e->reward, 0, N * sizeof(int32_t), e->stream));
    CHIP(hipMemsetAsync(e->done, 0, N, e->stream));
    CHIP(hipMemsetAsync(e->packed, 0, N * sizeof(uint64_t), e->stream));
    CHIP(e->staging.reserve(e->ops->state_size()));

    // config: NULL -> game defaults
    std::vector<uint8_t> cfg(e->ops->config_size());
    if (config_pod) {
        if (config_size != cfg.size()) { e->err = "config size mismatch"; return bail(TBX_E_INVALID); }
        memcpy(cfg.data(), config_pod, cfg.size());
    } else {
        switch (game) {
        case TBX_GAME_BREAKOUT: breakout_default_config((tbx_breakout_config_t*)cfg.data()); break;
        case TBX_GAME_SPACE_INVADERS: si_default_config((tbx_si_config_t*)cfg.data()); break;
        case TBX_GAME_AMIDAR: amidar_default_config((tbx_amidar_config_t*)cfg.data()); break;
        case TBX_GAME_GRIDWORLD: gridworld_default_config((tbx_gridworld_config_t*)cfg.data()); break;
        }
    }
    rc = e->ops->init(e, cfg.data(), cfg.size());
    if (rc) return bail(rc);
    // every env's simulator RNG starts at config.rand (first 16 bytes of every config record)
    uint64_t r[2];
    memcpy(r, cfg.data(), sizeof r);
    hipLaunchKernelGGL(fill_rng_kernel, dim3((n_envs + 255) / 256), dim3(256), 0, e->stream, e->sim_rng, n_envs, r[0], r[1]);
    CHIP(hipGetLastError());
    rc = e->ops->new_game(e, nullptr, e->stream);
    if (rc) return bail(rc);
    CHIP(hipStreamSynchronize(e->stream));
#undef CHIP
    *out = e;
    return TBX_OK;
}

int tbx_num_envs(const tbx_engine* e) { return e ? e->n : TBX_E_INVALID; }
int tbx_game(const tbx_engine* e) { return e ? e->game : TBX_E_INVALID; }

int tbx_seed(tbx_engine* e, int env, uint32_t seed)
{
    CHECK_ENGINE(e);
    if (env < -1 || env >= e->n) return e->fail(TBX_E_INVALID, "env index out of range");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    hipLaunchKernelGGL(seed_kernel, dim3((e->n + 255) / 256), dim3(256), 0, e->stream, e->sim_rng, e->n, env, seed);
    EHIP(hipGetLastError());
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int tbx_seed_array(tbx_engine* e, const uint32_t* seeds_host)
{
    CHECK_ENGINE(e);
    if (!seeds_host) return e->fail(TBX_E_INVALID, "seeds pointer is NULL");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    // e->actions is the engine's N-dword upload staging
    EHIP(hipMemcpyAsync(e->actions, seeds_host, (size_t)e->n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(seed_array_kernel, dim3((e->n + 255) / 256), dim3(256), 0, e->stream, e->sim_rng, e->n,
                       reinterpret_cast<const uint32_t*>(e->actions));
    EHIP(hipGetLastError());
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int tbx_get_sim_rng(tbx_engine* e, int env, uint64_t out[2])
{
    CHECK_ENGINE(e);
    if (env < 0 || env >= e->n || !out) return e->fail(TBX_E_INVALID, "env index out of range");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    EHIP(hipMemcpyAsync(&out[0], e->sim_rng + env, 8, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipMemcpyAsync(&out[1], e->sim_rng + (size_t)e->n + env, 8, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int tbx_set_sim_rng(tbx_engine* e, int env, const uint64_t st[2])
{
    CHECK_ENGINE(e);
    if (env < -1 || env >= e->n || !st) return e->fail(TBX_E_INVALID, "env index out of range");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    if (env == -1) {
        hipLaunchKernelGGL(fill_rng_kernel, dim3((e->n + 255) / 256), dim3(256), 0, e->stream, e->sim_rng, e->n, st[0], st[1]);
        EHIP(hipGetLastError());
    } else {
        EHIP(hipMemcpyAsync(e->sim_rng + env, &st[0], 8, hipMemcpyHostToDevice, e->stream));
        EHIP(hipMemcpyAsync(e->sim_rng + (size_t)e->n + env, &st[1], 8, hipMemcpyHostToDevice, e->stream));
    }
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int tbx_new_game(tbx_engine* e, const uint8_t* mask_host)
{
    CHECK_ENGINE(e);
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    const uint8_t* m = nullptr;
    if (mask_host) {
        EHIP(hipMemcpyAsync(e->mask, mask_host, (size_t)e->n, hipMemcpyHostToDevice, e->stream));
        m = e->mask;
    }
    int rc = e->ops->new_game(e, m, e->stream);
    if (rc) return rc;
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int tbx_step_device(tbx_engine* e, const int32_t* actions_dev, uint32_t flags, void* stream)
{
    CHECK_ENGINE(e);
    if (!actions_dev) return e->fail(TBX_E_INVALID, "actions pointer is NULL");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, (hipStream_t)stream));
    EHIP(tbx_gather_before_step(e, (hipStream_t)stream));
    ActionSource src{};
    src.actions = actions_dev;
    src.single_env = -1;
    return e->ops->step(e, src, flags, (hipStream_t)stream);
}

int tbx_step_synthetic(tbx_engine* e, uint64_t action_seed, uint64_t t, uint64_t env_offset, uint32_t flags, void* stream)
{
    CHECK_ENGINE(e);
    EHIP(hipSetDevice(e->device));
    ActionSource src{};
    src.actions = nullptr;
    src.seed = action_seed;
    src.t = t;
    src.env_offset = env_offset;
    src.single_env = -1;
    if (const int mode = pipe_mode(e)) return pipe_step(e, src, flags, (hipStream_t)stream, mode);
    EHIP(tbx_use_stream(e, (hipStream_t)stream));
    EHIP(tbx_gather_before_step(e, (hipStream_t)stream));
    return e->ops->step(e, src, flags, (hipStream_t)stream);
}

// ---- host delivery (toybox_amd.h: step_async / step_wait).  tbx_step is begin + end without a frame.

int tbx_host_alloc(void** out_ptr, size_t bytes)
{
    if (!out_ptr) { tbx_set_create_error("tbx_host_alloc: out_ptr is NULL"); return TBX_E_INVALID; }
    *out_ptr = nullptr;
    hipError_t r = hipHostMalloc(out_ptr, bytes ? bytes : 1, hipHostMallocDefault);
    if (r != hipSuccess) { tbx_set_create_error(std::string("hipHostMalloc: ") + hipGetErrorString(r)); return r == hipErrorOutOfMemory ? TBX_E_NOMEM : TBX_E_NO_DEVICE; }
    return TBX_OK;
}

int tbx_host_free(void* ptr)
{
    if (!ptr) return TBX_OK;
    hipError_t r = hipHostFree(ptr);
    if (r != hipSuccess) { tbx_set_create_error(std::string("hipHostFree: ") + hipGetErrorString(r)); return TBX_E_INVALID; }
    return TBX_OK;
}

// rows [first, last) of the host-side frame stack (see toybox_amd.h)
static void host_stack_rows(uint8_t* dst, const uint8_t* src, const uint8_t* plane, const uint8_t* done, int reset, int first, int last,
                            int px, int stack, int fill)
{
    for (int i = first; i < last; i++) {
        uint8_t* d = dst + (size_t)i * px * stack;
        const uint8_t* s = src + (size_t)i * px * stack;
        const uint8_t* p = plane + (size_t)i * px;
        const bool fresh = reset || (done && done[i]);
        if (stack == 4) {                                    // one dword per pixel: shift the older three down, the new byte on top
            uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
            if (d != s && (px & 15) == 0 && ((((uintptr_t)d | (uintptr_t)s | (uintptr_t)p)) & 15u) == 0) {
                // 16 pixels per turn with streaming stores: the destination (another array of the pool) is written without being
                // read first -- 8 bytes of host memory traffic per pixel instead of 12 (the roll is bound by exactly that)
                const __m128i zero = _mm_setzero_si128();
                for (int k = 0; k < px; k += 16) {
                    const __m128i pb = _mm_load_si128(reinterpret_cast<const __m128i*>(p + k));
                    const __m128i lo16 = _mm_unpacklo_epi8(zero, pb), hi16 = _mm_unpackhi_epi8(zero, pb);   // byte -> high half of a word
                    const __m128i top[4] = {_mm_unpacklo_epi16(zero, lo16), _mm_unpackhi_epi16(zero, lo16),   // ... -> top byte of a dword
                                            _mm_unpacklo_epi16(zero, hi16), _mm_unpackhi_epi16(zero, hi16)};
                    for (int q = 0; q < 4; q++) {
                        __m128i v;
                        if (!fresh) v = _mm_or_si128(_mm_srli_epi32(_mm_load_si128(reinterpret_cast<const __m128i*>(s4 + k + 4 * q)), 8), top[q]);
                        else if (fill) { const __m128i b = _mm_srli_epi32(top[q], 24); v = _mm_or_si128(_mm_or_si128(b, _mm_slli_epi32(b, 8)), _mm_or_si128(_mm_slli_epi32(b, 16), top[q])); }
                        else v = top[q];
                        _mm_stream_si128(reinterpret_cast<__m128i*>(d4 + k + 4 * q), v);
                    }
                }
                continue;
            }
            if (!fresh) for (int k = 0; k < px; k++) d4[k] = (s4[k] >> 8) | ((uint32_t)p[k] << 24);
            else if (fill) for (int k = 0; k < px; k++) d4[k] = (uint32_t)p[k] * 0x01010101u;
            else for (int k = 0; k < px; k++) d4[k] = (uint32_t)p[k] << 24;
            continue;
        }
        for (int k = 0; k < px; k++) {
            uint8_t* dk = d + (size_t)k * stack;
            const uint8_t* sk = s + (size_t)k * stack;
            for (int c = 0; c + 1 < stack; c++) dk[c] = fresh ? (fill ? p[k] : (uint8_t)0) : sk[c + 1];
            dk[stack - 1] = p[k];
        }
    }
    _mm_sfence();                                            // the streaming stores above are globally visible before the thread is joined
}

int tbx_host_stack_push(uint8_t* dst, const uint8_t* src, const uint8_t* plane, const uint8_t* done, int reset, int n, int px, int stack,
                        int fill, int threads)
{
    if (!dst || !src || !plane || n < 0 || px < 1 || stack < 1 || stack > 16 || fill < 0 || fill > 1) {
        tbx_set_create_error("tbx_host_stack_push: bad argument");
        return TBX_E_INVALID;
    }
    if (stack == 4 && ((((uintptr_t)dst | (uintptr_t)src) & 3u) != 0)) { tbx_set_create_error("tbx_host_stack_push: stacks of depth 4 must be 4-byte aligned"); return TBX_E_INVALID; }
    int T = threads;
    if (T <= 0) {
        cpu_set_t set;
        T = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : 1;
        if (T > 16) T = 16;
    }
    const long work = (long)n * px;
    if ((long)T > work >> 19) T = (int)(work >> 19);         // half a million pixels per thread at least: starting a thread costs ~20 us
                                                             // (64 envs: 0.54 ms with sixteen threads, 0.07 with one)
    if (T > n) T = n > 0 ? n : 1;
    if (T <= 1) { host_stack_rows(dst, src, plane, done, reset, 0, n, px, stack, fill); return TBX_OK; }
    std::vector<std::thread> pool;
    pool.reserve((size_t)T);
    for (int t = 0; t < T; t++) {
        const int first = (int)((long)n * t / T), last = (int)((long)n * (t + 1) / T);
        pool.emplace_back(host_stack_rows, dst, src, plane, done, reset, first, last, px, stack, fill);
    }
    for (auto& th : pool) th.join();
    return TBX_OK;
}

// the waiting half of tbx_step_end: the queued step has finished, its outputs are in the caller's buffers
static int step_deliver(tbx_engine* e)
{
    EHIP(hipSetDevice(e->device));
    EHIP(hipStreamSynchronize(e->stream));
    e->host_pending = false;
    e->pending_kind = 0;
    const size_t N = (size_t)e->n;
    const int32_t* host_out = e->io_host + N;
    const tbx_step_host_out_t& o = e->host_out;
    if (o.reward) memcpy(o.reward, host_out, N * sizeof(int32_t));
    if (o.lives) memcpy(o.lives, host_out + N, N * sizeof(int32_t));
    if (o.score) memcpy(o.score, host_out + 2 * N, N * sizeof(int32_t));
    if (o.done) memcpy(o.done, host_out + 3 * N + 1, N);
    if (host_out[3 * N] & 2) return e->fail(TBX_E_NEEDS_RESET, "an env was stepped after its game ended inside EpisodicLifeEnv's no-op step (bench.Monitor raises here)");
    if (host_out[3 * N]) return e->fail(TBX_E_ACTION, "an illegal ALE action id was passed (treated as NOOP)");
    return TBX_OK;
}

// Another entry point was called between "_begin" and "_end" (every one that queues work comes through tbx_use_stream or
// pipe_enter): the step is ended here -- the stream drained, the outputs delivered to the caller's buffers -- and what its "_end"
// call would have returned is kept for that call (the header promised this, and a later "_end" delivered stale data).
}  // extern "C"

hipError_t tbx_finish_pending(tbx_engine* e)
{
    const int kind = e->pending_kind;
    if (!kind) return hipSuccess;
    const int rc = kind == 1 ? step_deliver(e) : tbx_agent_deliver(e);
    e->pending_kind = 0;
    e->ended_early_kind = kind;
    e->ended_early_rc = rc;
    e->ended_early_msg = rc ? e->err : std::string();
    return rc == TBX_E_NO_DEVICE ? hipErrorUnknown : hipSuccess;
}

extern "C" {

int tbx_step_begin(tbx_engine* e, const int32_t* actions_host, uint32_t flags, const tbx_step_host_out_t* out)
{
    CHECK_ENGINE(e);
    if (!actions_host || !out) return e->fail(TBX_E_INVALID, "actions / output descriptor is NULL");
    if (e->pending_kind) return e->fail(TBX_E_INVALID, "tbx_step_begin: the previous step has not been ended (tbx_step_end / tbx_agent_step_end)");
    e->ended_early_kind = 0;                   // (an "_end" that was never called for a step another call ended)
    if (out->frame && out->channels != 1 && out->channels != 3 && out->channels != 4) return e->fail(TBX_E_INVALID, "channels must be 1, 3 or 4");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    EHIP(tbx_gather_before_step(e, e->stream));
    const size_t N = (size_t)e->n;
    const size_t out_bytes = (3 * N + 1) * sizeof(int32_t) + N;
    if (!e->io_dev) {
        EHIP(hipMalloc((void**)&e->io_dev, out_bytes));
        EHIP(hipHostMalloc((void**)&e->io_host, N * sizeof(int32_t) + out_bytes, hipHostMallocDefault));
    }
    int32_t* host_actions = e->io_host;
    int32_t* host_out = e->io_host + N;
    memcpy(host_actions, actions_host, N * sizeof(int32_t));
    EHIP(hipMemcpyAsync(e->actions, host_actions, N * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    ActionSource src{};
    src.actions = e->actions;
    src.single_env = -1;
    int rc = e->ops->step(e, src, flags, e->stream);
    if (rc) return rc;
    hipLaunchKernelGGL(gather_outputs_kernel, dim3((e->n + 255) / 256), dim3(256), 0, e->stream, e->reward, e->lives_out, e->score_out,
                       e->done, e->err_flag, e->io_dev, e->n);
    EHIP(hipGetLastError());
    EHIP(hipMemcpyAsync(host_out, e->io_dev, out_bytes, hipMemcpyDeviceToHost, e->stream));
    if (out->frame) {
        const size_t bytes = N * e->ops->height() * e->ops->width() * out->channels;
        rc = ensure_frame(e, bytes);
        if (rc) return rc;
        rc = e->ops->render(e, e->frame_own.p, out->channels, 0, e->n, e->stream);
        if (rc) return rc;
        EHIP(hipMemcpyAsync(out->frame, e->frame_own.p, bytes, hipMemcpyDeviceToHost, e->stream));
    }
    e->host_out = *out;
    e->host_pending = true;
    e->pending_kind = 1;
    return TBX_OK;
}

int tbx_step_end(tbx_engine* e)
{
    CHECK_ENGINE(e);
    if (!e->host_pending) {
        if (e->ended_early_kind == 1) {        // another call on the handle ended the step: its outputs have been delivered
            e->ended_early_kind = 0;
            return e->ended_early_rc ? e->fail(e->ended_early_rc, e->ended_early_msg) : TBX_OK;
        }
        return e->fail(TBX_E_INVALID, "tbx_step_end without tbx_step_begin");
    }
    return step_deliver(e);
}

int tbx_step(tbx_engine* e, const int32_t* actions_host, uint32_t flags, int32_t* reward, uint8_t* done,
             int32_t* lives, int32_t* score)
{
    CHECK_ENGINE(e);
    if (e->pending_kind) return e->fail(TBX_E_INVALID, "tbx_step: a step is between its begin and end calls (tbx_step_end / tbx_agent_step_end)");
    tbx_step_host_out_t out{};
    out.reward = reward; out.done = done; out.lives = lives; out.score = score;
    int rc = tbx_step_begin(e, actions_host, flags, &out);
    if (rc) return rc;
    return tbx_step_end(e);
}

// ---- resident single-env step (TbxServeCtl, tbx_common.hpp)

// the pinned, device-mapped frame buffer of the single-env path (tbx_step1_frame): the resident kernel rasterises into it
static int ensure_serve_frame(tbx_engine* e)
{
    if (e->serve_frame) return TBX_OK;
    const size_t bytes = (size_t)e->ops->height() * e->ops->width() * 4;
    EHIP(hipHostMalloc((void**)&e->serve_frame, bytes, hipHostMallocMapped));
    memset(e->serve_frame, 0, bytes);
    EHIP(hipHostGetDevicePointer((void**)&e->serve_frame_dev, e->serve_frame, 0));
    return TBX_OK;
}

static int serve_start(tbx_engine* e)
{
    if (!e->serve_ctl) {
        EHIP(hipHostMalloc((void**)&e->serve_ctl, sizeof(TbxServeCtl), hipHostMallocMapped | hipHostMallocCoherent));
        memset(e->serve_ctl, 0, sizeof(TbxServeCtl));
        EHIP(hipHostGetDevicePointer((void**)&e->serve_ctl_dev, e->serve_ctl, 0));
        EHIP(hipStreamCreateWithFlags(&e->serve_stream, hipStreamNonBlocking));
    }
    if (!e->serve_frame) {
        int rc = ensure_serve_frame(e);
        if (rc) return rc;
    }
    TbxServeCtl* c = e->serve_ctl;
    c->exited = 0;
    c->frame_dev = (uint64_t)(uintptr_t)e->serve_frame_dev;
    c->ack_seq = e->serve_seq;
    c->req = (uint64_t)e->serve_seq;
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    // ordered after everything queued through the handle so far
    EHIP(tbx_use_stream(e, e->serve_stream));
    int rc = e->ops->serve(e, e->serve_ctl_dev, e->serve_stream);
    if (rc) return rc;
    e->serve_running = true;
    return TBX_OK;
}

}  // extern "C"

hipError_t tbx_serve_stop(tbx_engine* e)
{
    if (!e->serve_running) return hipSuccess;
    __atomic_store_n(&e->serve_ctl->req, (uint64_t)e->serve_seq | TBX_SERVE_STOP, __ATOMIC_RELEASE);
    hipError_t r = hipStreamSynchronize(e->serve_stream);     // the wave leaves at its next poll
    e->serve_running = false;
    return r;
}

extern "C" {

// one frame of one env, optionally with its picture (channels 0 / 1 / 3 / 4) in e->serve_frame
static int step1_impl(tbx_engine* e, int env, int32_t ale_action, uint32_t flags, int channels, int32_t out[4])
{
    CHECK_ENGINE(e);
    if (env < 0 || env >= e->n) return e->fail(TBX_E_INVALID, "env index out of range");
    if (channels != 0 && channels != 1 && channels != 3 && channels != 4) return e->fail(TBX_E_INVALID, "channels must be 1, 3 or 4");
    EHIP(hipSetDevice(e->device));
    bool painted = false;
    if (e->n == 1 && e->opt[TBX_OPT_RESIDENT_STEP] && !e->gather) {
        // the resident kernel: post the request, spin on the acknowledgement (no launch, no copy, no synchronisation)
        TbxServeCtl* c = e->serve_ctl;
        if (!e->serve_running || __atomic_load_n(&c->exited, __ATOMIC_ACQUIRE)) {
            if (e->serve_running) { EHIP(hipStreamSynchronize(e->serve_stream)); e->serve_running = false; }
            int rc = serve_start(e);
            if (rc == TBX_E_UNSUPPORTED) goto slow;
            if (rc) return rc;
            c = e->serve_ctl;
        }
        {
            const uint32_t want = (channels && e->ops->serve_paints()) ? (channels == 1 ? 1u : channels == 3 ? 2u : 3u) : 0u;
            const uint32_t seq = ++e->serve_seq;
            const uint64_t word = tbx_serve_word(seq, ale_action, (flags & 0x0Fu) | (want << TBX_SERVE_FRAME_SHIFT));
            __atomic_store_n(&c->req, word, __ATOMIC_RELEASE);
            unsigned long spins = 0;
            while (__atomic_load_n(&c->ack_seq, __ATOMIC_ACQUIRE) != seq) {
                if ((++spins & 0xFFFul) == 0) {
                    if (__atomic_load_n(&c->exited, __ATOMIC_ACQUIRE) && __atomic_load_n(&c->ack_seq, __ATOMIC_ACQUIRE) != seq) {
                        // the wave went idle and left just as the request arrived: start another, it serves the pending request
                        EHIP(hipStreamSynchronize(e->serve_stream));
                        e->serve_running = false;
                        e->serve_seq = seq - 1;
                        int rc = serve_start(e);
                        if (rc) return rc;
                        e->serve_seq = seq;
                        __atomic_store_n(&c->req, word, __ATOMIC_RELEASE);
                    }
                    if (spins > (1ul << 33)) return e->fail(TBX_E_NO_DEVICE, "the resident step kernel does not answer");
                }
                __builtin_ia32_pause();
            }
            const uint32_t de = c->done_err;
            if (out) { out[0] = c->reward; out[1] = (int32_t)(de & 1u); out[2] = c->lives; out[3] = c->score; }
            painted = want != 0 && !(de & 4u);
            if (channels && !painted) {                      // this game's resident kernel does not paint: the launched rasteriser
                int rc = ensure_serve_frame(e);
                if (rc) return rc;
                rc = tbx_render_env(e, env, e->serve_frame, channels);
                if (rc) return rc;
            }
            if (de & 2u) return e->fail(TBX_E_ACTION, "an illegal ALE action id was passed (treated as NOOP)");
            return TBX_OK;
        }
    }
slow:
    {
        // any env of a batch engine: the single-env launch of tbx_apply_input, then its outputs
        const uint32_t b = tbx_ale_buttons(ale_action);
        const int action_rc = b == 0xFFu ? TBX_E_ACTION : TBX_OK;
        int rc = tbx_apply_input(e, env, b == 0xFFu ? 0u : b);
        if (rc) return rc;
        bool reset = false;
        int32_t o[4] = {0, 0, 0, 0};
        uint8_t dn = 0;
        EHIP(hipMemcpy(&o[0], e->reward + env, 4, hipMemcpyDeviceToHost));
        EHIP(hipMemcpy(&dn, e->done + env, 1, hipMemcpyDeviceToHost));
        EHIP(hipMemcpy(&o[2], e->lives_out + env, 4, hipMemcpyDeviceToHost));
        EHIP(hipMemcpy(&o[3], e->score_out + env, 4, hipMemcpyDeviceToHost));
        o[1] = dn;
        if ((flags & TBX_STEP_AUTO_RESET) && o[2] <= 0) {
            // (rare on this path) a finished game starts over, as in tbx_step
            std::vector<uint8_t> mask((size_t)e->n, 0);
            mask[(size_t)env] = 1;
            rc = tbx_new_game(e, mask.data());
            if (rc) return rc;
            o[1] = 1;
            reset = true;
        }
        (void)reset;
        if (out) memcpy(out, o, sizeof o);
        if (channels) {
            rc = ensure_serve_frame(e);
            if (rc) return rc;
            rc = tbx_render_env(e, env, e->serve_frame, channels);
            if (rc) return rc;
        }
        return action_rc ? e->fail(TBX_E_ACTION, "an illegal ALE action id was passed (treated as NOOP)") : TBX_OK;
    }
}

int tbx_step1(tbx_engine* e, int env, int32_t ale_action, uint32_t flags, int32_t out[4])
{
    return step1_impl(e, env, ale_action, flags, 0, out);
}

int tbx_step1_frame(tbx_engine* e, int env, int32_t ale_action, uint32_t flags, int channels, int32_t out[4], const uint8_t** frame_host)
{
    if (e && channels == 0) return e->fail(TBX_E_INVALID, "channels must be 1, 3 or 4");
    int rc = step1_impl(e, env, ale_action, flags, channels, out);
    if (frame_host && e) *frame_host = (rc == TBX_OK || rc == TBX_E_ACTION) ? e->serve_frame : nullptr;
    return rc;
}

int tbx_apply_input(tbx_engine* e, int env, uint32_t buttons)
{
    CHECK_ENGINE(e);
    if (env < 0 || env >= e->n) return e->fail(TBX_E_INVALID, "env index out of range");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    EHIP(tbx_gather_before_step(e, e->stream));
    ActionSource src{};
    src.single_env = env;
    src.single_buttons = buttons & 0x3Fu;
    int rc = e->ops->step(e, src, 0, e->stream);
    if (rc) return rc;
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int tbx_get_scalars(tbx_engine* e, int32_t* score, int32_t* lives, int32_t* level, uint8_t* game_over)
{
    CHECK_ENGINE(e);
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    const size_t N = (size_t)e->n;
    int32_t* tmp = e->scal;
    int rc = e->ops->scalars(e, tmp, tmp + N, tmp + 2 * N, e->stream);
    if (rc) return rc;
    if (!e->scal_host) EHIP(hipHostMalloc((void**)&e->scal_host, 3 * N * sizeof(int32_t), hipHostMallocDefault));
    const int32_t* host = e->scal_host;
    EHIP(hipMemcpyAsync(e->scal_host, tmp, 3 * N * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < N; i++) {
        if (score) score[i] = host[i];
        if (lives) lives[i] = host[N + i];
        if (level) level[i] = host[2 * N + i];
        if (game_over) game_over[i] = host[N + i] <= 0;
    }
    return TBX_OK;
}

int tbx_render_device(tbx_engine* e, uint8_t* out_dev, int channels, void* stream)
{
    CHECK_ENGINE(e);
    if (channels != 1 && channels != 3 && channels != 4) return e->fail(TBX_E_INVALID, "channels must be 1, 3 or 4");
    EHIP(hipSetDevice(e->device));
    if (const int mode = pipe_mode(e)) return pipe_render(e, out_dev, channels, (hipStream_t)stream, mode);
    EHIP(tbx_use_stream(e, (hipStream_t)stream));
    if (!out_dev) {
        const size_t bytes = (size_t)e->n * e->ops->height() * e->ops->width() * channels;
        int rc = ensure_frame(e, bytes);
        if (rc) return rc;
        out_dev = e->frame;
    }
    if (((uintptr_t)out_dev & 15u) != 0) return e->fail(TBX_E_INVALID, "frame buffer must be 16-byte aligned");
    return e->ops->render(e, out_dev, channels, 0, e->n, (hipStream_t)stream);
}

int tbx_render_step_synthetic(tbx_engine* e, uint8_t* out_dev, int channels, uint64_t action_seed, uint64_t t, uint64_t env_offset,
                              uint32_t flags, void* stream)
{
    CHECK_ENGINE(e);
    if (channels != 1 && channels != 3 && channels != 4) return e->fail(TBX_E_INVALID, "channels must be 1, 3 or 4");
    EHIP(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    ActionSource src{};
    src.actions = nullptr;
    src.seed = action_seed;
    src.t = t;
    src.env_offset = env_offset;
    src.single_env = -1;
    if (fused_overlap_on(e, out_dev, channels)) return fused_overlapped(e, channels, src, flags, s);
    EHIP(tbx_use_stream(e, s));                                 // (everything on the caller's stream: leaves a pipelined mode first)
    if (!out_dev) {
        const size_t bytes = (size_t)e->n * e->ops->height() * e->ops->width() * channels;
        int rc = ensure_frame(e, bytes);
        if (rc) return rc;
        out_dev = e->frame;                                     // (ensure_frame: TBX_BUF_FRAME is the engine's own buffer again)
    }
    if (((uintptr_t)out_dev & 15u) != 0) return e->fail(TBX_E_INVALID, "frame buffer must be 16-byte aligned");
    if (e->ops->render_step_fused(channels)) {
        EHIP(tbx_gather_before_step(e, s));
        return e->ops->render_step(e, out_dev, channels, src, flags, s);
    }
    // engines whose rasteriser reads live state (or gray frames): the same two things as two launches in stream order
    int rc = e->ops->render(e, out_dev, channels, 0, e->n, s);
    if (rc) return rc;
    EHIP(tbx_gather_before_step(e, s));
    return e->ops->step(e, src, flags, s);
}

int tbx_rollout_synthetic(tbx_engine* e, int channels, uint64_t action_seed, uint64_t t0, int k, uint64_t env_offset, uint32_t flags, void* stream)
{
    CHECK_ENGINE(e);
    if (channels != 1 && channels != 3 && channels != 4) return e->fail(TBX_E_INVALID, "channels must be 1, 3 or 4");
    if (k < 1 || k > 64) return e->fail(TBX_E_INVALID, "tbx_rollout_synthetic: k must be in 1 .. 64");
    EHIP(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (e->gather_ring && e->gather_ring_every != k)
        return e->fail(TBX_E_INVALID, "tbx_rollout_synthetic: the chunk must be as long as the gather's record ring (TBX_OPT_GATHER_EVERY)");
    if (e->gather_ring && tbx_gather_fill(e) != 0)
        return e->fail(TBX_E_INVALID, "tbx_rollout_synthetic: the record ring is partly filled (finish it with single steps + tbx_gather)");
    ActionSource src{};
    src.actions = nullptr;
    src.seed = action_seed;
    src.t = t0;
    src.env_offset = env_offset;
    src.single_env = -1;
    if (rollout_chunks_on(e, channels)) return rollout_chunked(e, channels, src, flags, k, s);
    // everywhere else: the k single calls in stream order, frames into chunk buffer 0, the step records into the ring (K-step ring:
    // tbx_gather after every step, the k-th one sends it) or copied out of TBX_BUF_PACKED after every step
    EHIP(tbx_use_stream(e, s));
    TbxRolloutResult& p = e->rollout;
    const size_t fb = (size_t)e->n * e->ops->height() * e->ops->width() * channels;
    int rc = chunk_buffers(e, 0, k, fb, !e->gather_ring, s, nullptr);
    if (rc) return rc;
    uint64_t* ring_base = nullptr;
    for (int j = 0; j < k; j++) {
        rc = tbx_render_step_synthetic(e, p.frames[0].p + (size_t)j * fb, channels, action_seed, t0 + (uint64_t)j, env_offset, flags, s);
        if (rc) return rc;
        if (e->gather_ring) {
            if (j == 0) ring_base = e->packed;                  // slot 0 of the ring this chunk fills
            rc = tbx_gather(e, nullptr, s);
            if (rc) return rc;
        } else if (e->gather) {
            rc = tbx_gather(e, nullptr, s);                     // one collective per step
            if (rc) return rc;
            EHIP(hipMemcpyAsync(p.packed[0].p + (size_t)j * e->n, e->packed, sizeof(uint64_t) * (size_t)e->n, hipMemcpyDeviceToDevice, s));
        } else
            EHIP(hipMemcpyAsync(p.packed[0].p + (size_t)j * e->n, e->packed, sizeof(uint64_t) * (size_t)e->n, hipMemcpyDeviceToDevice, s));
    }
    p.cur = 0; p.k = k; p.channels = channels;
    p.packed_base = e->gather_ring ? ring_base : p.packed[0].p;
    p.packed_stride = e->gather_ring ? (size_t)e->gather_ring_width : (size_t)e->n;
    e->frame = p.frames[0].p + (size_t)(k - 1) * fb;        // TBX_BUF_FRAME: the chunk's last frame, as in rollout_chunked
    e->frame_bytes = fb;
    return TBX_OK;
}

int tbx_render(tbx_engine* e, uint8_t* out_host, int channels)
{
    CHECK_ENGINE(e);
    if (!out_host) return e->fail(TBX_E_INVALID, "output pointer is NULL");
    int rc = tbx_render_device(e, nullptr, channels, e->stream);
    if (rc) return rc;
    const size_t bytes = (size_t)e->n * e->ops->height() * e->ops->width() * channels;
    EHIP(hipMemcpyAsync(out_host, e->frame, bytes, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int tbx_render_env(tbx_engine* e, int env, uint8_t* out_host, int channels)
{
    CHECK_ENGINE(e);
    if (env < 0 || env >= e->n || !out_host) return e->fail(TBX_E_INVALID, "env index out of range");
    if (channels != 1 && channels != 3 && channels != 4) return e->fail(TBX_E_INVALID, "channels must be 1, 3 or 4");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    const size_t bytes = (size_t)e->ops->height() * e->ops->width() * channels;
    if (!e->one_frame) EHIP(hipMalloc((void**)&e->one_frame, (size_t)e->ops->height() * e->ops->width() * 4));
    int rc = e->ops->render(e, e->one_frame, channels, env, 1, e->stream);
    if (rc) return rc;
    EHIP(hipMemcpyAsync(out_host, e->one_frame, bytes, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int tbx_get_states(tbx_engine* e, int first_env, int count, void* pods, size_t record_size)
{
    CHECK_ENGINE(e);
    if (first_env < 0 || count < 1 || first_env + count > e->n || !pods) return e->fail(TBX_E_INVALID, "env range out of bounds");
    if (record_size != e->ops->state_size()) return e->fail(TBX_E_INVALID, "state record size mismatch");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    EHIP(e->staging.reserve(record_size * (size_t)count, e->stream));
    int rc = e->ops->pack_state(e, first_env, count, e->stream);
    if (rc) return rc;
    EHIP(hipMemcpyAsync(pods, e->staging.p, record_size * (size_t)count, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int tbx_set_states(tbx_engine* e, int first_env, int count, const void* pods, size_t record_size)
{
    CHECK_ENGINE(e);
    if (first_env < 0 || count < 1 || first_env + count > e->n || !pods) return e->fail(TBX_E_INVALID, "env range out of bounds");
    if (record_size != e->ops->state_size()) return e->fail(TBX_E_INVALID, "state record size mismatch");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    EHIP(e->staging.reserve(record_size * (size_t)count, e->stream));
    int rc = e->ops->unpack_state(e, first_env, count, pods, e->stream);
    if (rc) return rc;
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int tbx_get_state(tbx_engine* e, int env, void* pod, size_t size)
{
    CHECK_ENGINE(e);
    if (env < 0 || env >= e->n || !pod) return e->fail(TBX_E_INVALID, "env index out of range");
    return tbx_get_states(e, env, 1, pod, size);
}

int tbx_set_state(tbx_engine* e, int env, const void* pod, size_t size)
{
    CHECK_ENGINE(e);
    if (env < 0 || env >= e->n || !pod) return e->fail(TBX_E_INVALID, "env index out of range");
    return tbx_set_states(e, env, 1, pod, size);
}

int tbx_get_config(tbx_engine* e, void* pod, size_t size)
{
    CHECK_ENGINE(e);
    if (!pod || size != e->ops->config_size()) return e->fail(TBX_E_INVALID, "config record size mismatch");
    int rc = e->ops->get_config(e, pod);
    if (rc) return rc;
    uint64_t r[2];
    rc = tbx_get_sim_rng(e, 0, r);
    if (rc) return rc;
    memcpy(pod, r, sizeof r);
    return TBX_OK;
}

int tbx_set_config(tbx_engine* e, const void* pod, size_t size)
{
    CHECK_ENGINE(e);
    if (!pod || size != e->ops->config_size()) return e->fail(TBX_E_INVALID, "config record size mismatch");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    int rc = e->ops->set_config(e, pod);
    if (rc) return rc;
    // `rand` as tbx_get_config reported it (env 0's words) means "not edited": the per-env simulator RNGs stay as they are,
    // so a config edit does not collapse a seeded batch onto one stream.  Any other value is written to every env.
    uint64_t r[2], cur[2];
    memcpy(r, pod, sizeof r);
    rc = tbx_get_sim_rng(e, 0, cur);
    if (rc) return rc;
    if (r[0] == cur[0] && r[1] == cur[1]) return TBX_OK;
    return tbx_set_sim_rng(e, -1, r);
}

// ---- batched interventions (include/toybox_amd.h): field writes and per-env features over the state in HBM

int tbx_reduce_width(int game, int query)
{
    const bool every_game = game >= TBX_GAME_BREAKOUT && game <= TBX_GAME_GRIDWORLD;
    switch (query) {
    case TBX_QUERY_BRK_BRICKS_REMAINING: case TBX_QUERY_BRK_NUM_BRICKS: case TBX_QUERY_BRK_IS_CHANNEL: case TBX_QUERY_BRK_CHANNEL_COUNT:
    case TBX_QUERY_BRK_FIND_CHANNEL: return game == TBX_GAME_BREAKOUT ? 1 : TBX_E_INVALID;
    case TBX_QUERY_BRK_COLUMN: case TBX_QUERY_BRK_ROW: return game == TBX_GAME_BREAKOUT ? 32 : TBX_E_INVALID;
    case TBX_QUERY_BRK_PADDLE: return game == TBX_GAME_BREAKOUT ? 4 : TBX_E_INVALID;
    case TBX_QUERY_BRK_BALLS: return game == TBX_GAME_BREAKOUT ? 1 + 4 * TBX_BRK_MAX_BALLS : TBX_E_INVALID;
    case TBX_QUERY_AMI_MODE: return game == TBX_GAME_AMIDAR ? 2 : TBX_E_INVALID;
    case TBX_QUERY_AMI_ANY_CAUGHT: case TBX_QUERY_AMI_TILE: case TBX_QUERY_AMI_COUNT_TILES: case TBX_QUERY_AMI_PLAYER_ON_PAINTED:
    case TBX_QUERY_AMI_PLAYER_NEAR_UNPAINTED: return game == TBX_GAME_AMIDAR ? 1 : TBX_E_INVALID;
    case TBX_QUERY_AMI_ADJACENT: return game == TBX_GAME_AMIDAR ? 4 : TBX_E_INVALID;
    case TBX_QUERY_AMI_ENEMY_DISTANCES: case TBX_QUERY_AMI_PLAYER_ENEMY_DISTANCES: return game == TBX_GAME_AMIDAR ? TBX_AMI_MAX_ENEMIES : TBX_E_INVALID;
    case TBX_QUERY_AMI_PLAYER_TILE: return game == TBX_GAME_AMIDAR ? 3 : TBX_E_INVALID;
    case TBX_QUERY_SI_SHIP: return game == TBX_GAME_SPACE_INVADERS ? 8 : TBX_E_INVALID;
    case TBX_QUERY_BRK_FIND_BRICK: return game == TBX_GAME_BREAKOUT ? 1 : TBX_E_INVALID;
    case TBX_QUERY_AMI_TILES_MASK: return game == TBX_GAME_AMIDAR ? 32 : TBX_E_INVALID;
    case TBX_QUERY_AMI_RANDOM_TILE: return game == TBX_GAME_AMIDAR ? 4 : TBX_E_INVALID;
    case TBX_QUERY_AMI_RANDOM_DIR: return game == TBX_GAME_AMIDAR ? 2 : TBX_E_INVALID;
    // the engine's own queries: every game has them
    case TBX_QUERY_CHECKPOINT_VALID: return every_game ? 1 : TBX_E_INVALID;
    case TBX_QUERY_LOOKAHEAD: case TBX_QUERY_LOOKAHEAD_PLAN: return every_game ? 5 : TBX_E_INVALID;
    case TBX_QUERY_LOOKAHEAD_ALL: return every_game ? 5 * tbx_legal_count(game) : TBX_E_INVALID;
    case TBX_QUERY_LOOKAHEAD_SEARCH: case TBX_QUERY_LOOKAHEAD_BEAM: case TBX_QUERY_LOOKAHEAD_EVOLVE: return every_game ? 6 * tbx_legal_count(game) : TBX_E_INVALID;
    case TBX_QUERY_LOOKAHEAD_ACT: return every_game ? 11 : TBX_E_INVALID;
    case TBX_QUERY_LOOKAHEAD_TREE_ACT: return every_game ? 14 : TBX_E_INVALID;
    case TBX_QUERY_LOOKAHEAD_SAMPLES: return every_game ? 8 * tbx_legal_count(game) : TBX_E_INVALID;
    case TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES: case TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES: return every_game ? 9 * tbx_legal_count(game) : TBX_E_INVALID;
    case TBX_QUERY_LOOKAHEAD_TREE: return every_game ? 12 * tbx_legal_count(game) : TBX_E_INVALID;
    default: return TBX_E_INVALID;
    }
}

static int edit_args(tbx_engine* e, const double* args, int n_args, int per_env, bool args_on_host, hipStream_t s, TbxEditArgs& a)
{
    if (n_args < 0 || n_args > TBX_EDIT_MAX_ARGS || (n_args > 0 && !args)) return e->fail(TBX_E_INVALID, "bad intervention arguments");
    memset(&a, 0, sizeof a);
    a.n = n_args;
    a.per_env = nullptr;
    if (!per_env || n_args == 0) {
        for (int i = 0; i < n_args; i++) a.v[i] = args[i];                  // (a host pointer in every form)
        return TBX_OK;
    }
    if (!args_on_host) { a.per_env = args; return TBX_OK; }
    const size_t bytes = sizeof(double) * (size_t)e->n * (size_t)n_args;
    EHIP(e->edit_args.reserve(bytes, e->stream));
    EHIP(hipMemcpyAsync(e->edit_args.p, args, bytes, hipMemcpyHostToDevice, s));
    a.per_env = e->edit_args.p;
    return TBX_OK;
}

// ---- The shared row of a lookahead query is refused on the host, before anything is launched (per-env rows are met by the kernels).
// These are the only copies of the checks.  Every query calls them top to bottom in its own order -- the first fault of a row
// decides the message -- with its own word in front of the colon.
static bool playable(int game, double v)
{
    if (v == -1.0) return true;
    for (int i = 0; i < tbx_legal_count(game); i++)
        if (v == (double)tbx_legal_action(game, i)) return true;
    return false;
}
// columns 0 and 1
static int shared_frames_hold(tbx_engine* e, const TbxEditArgs& a)
{
    if (!(a.v[0] >= 1.0 && a.v[0] <= (double)TBX_LOOKAHEAD_MAX_FRAMES)) return e->fail(TBX_E_INVALID, "lookahead: frames must be 1 .. TBX_LOOKAHEAD_MAX_FRAMES");
    if (a.n > 1 && !(a.v[1] >= 1.0)) return e->fail(TBX_E_INVALID, "lookahead: hold must be at least 1");
    return TBX_OK;
}
// column `col`, where the row has it: `name` ("first", "rest") is -1 or an action the game plays
static int shared_action(tbx_engine* e, const TbxEditArgs& a, int col, const char* name)
{
    if (a.n > col && !playable(e->game, a.v[col])) return e->fail(TBX_E_INVALID, std::string("lookahead: ") + name + " is neither -1 nor a legal action of this game");
    return TBX_OK;
}
// columns 2 and 3 of the planners that rank plans (a search checks its plan count between the two)
static int shared_depth(tbx_engine* e, const char* word, double depth, int least)
{
    if (!(depth >= (double)least && depth <= (double)tbx_plan_max_depth(e->game)))
        return e->fail(TBX_E_INVALID, std::string(word) + ": depth must be " + std::to_string(least) + " .. TBX_PLAN_MAX_DEPTH(game)");
    return TBX_OK;
}
static int shared_objective(tbx_engine* e, const char* word, const TbxEditArgs& a)
{
    if (a.n > 3 && !(a.v[3] == 0.0 || a.v[3] == 1.0)) return e->fail(TBX_E_INVALID, std::string(word) + ": objective must be 0 (return) or 1 (survival)");
    return TBX_OK;
}
static int shared_width(tbx_engine* e, const char* word, double width)
{
    if (!(width >= 1.0 && width <= (double)TBX_BEAM_MAX_WIDTH)) return e->fail(TBX_E_INVALID, std::string(word) + ": width must be 1 .. TBX_BEAM_MAX_WIDTH");
    return TBX_OK;
}
static int shared_samples(tbx_engine* e, const char* word, double count)
{
    if (!(count >= 1.0 && count <= (double)TBX_LOOKAHEAD_MAX_SAMPLES)) return e->fail(TBX_E_INVALID, std::string(word) + ": samples must be 1 .. TBX_LOOKAHEAD_MAX_SAMPLES");
    return TBX_OK;
}
// the salt of `samples` futures (the count is checked): sample s draws with salt + s, in 32 bits
static int shared_salt(tbx_engine* e, const char* word, double salt, long long samples)
{
    if (!(salt >= 0.0 && salt < 4294967296.0)) return e->fail(TBX_E_INVALID, std::string(word) + ": salt must be 0 .. 2^32 - 1");
    if ((uint64_t)salt != 0 && (uint64_t)salt + (uint64_t)samples - 1 >= (1ull << 32)) return e->fail(TBX_E_INVALID, std::string(word) + ": salt + samples - 1 must stay below 2^32");
    return TBX_OK;
}
// The most arguments each lookahead query takes: its own "takes {...}" refusal, tbx_reduce's scan of host rows and TBX_QUERY_LOOKAHEAD_ACT
// read it here (150 / 151, 152, 153, 154, 155, 156, 157, 158, 160)
static constexpr int MAX_ARGS_LOOKAHEAD = 8, MAX_ARGS_PLAN = 9, MAX_ARGS_SEARCH = 9, MAX_ARGS_SAMPLES = 9, MAX_ARGS_SEARCH_SAMPLES = 11, MAX_ARGS_BEAM = 10,
                     MAX_ARGS_BEAM_SAMPLES = 12, MAX_ARGS_EVOLVE = 15, MAX_ARGS_TREE = 12;

// chunks > 1: the winner among the partial rows parts[group][chunks][6] of every (env, first action) group of envs from
// first_env on, by the order of the search kernel; a group without a leaf (a refused row) answers zeros
__global__ __launch_bounds__(256) void tbx_search_pick_kernel(const double* __restrict__ parts, TbxEditArgs a, int legal, int chunks, long long first_group, int count,
                                                              double* __restrict__ out)
{
    const int rel = blockIdx.x * 256 + threadIdx.x;
    if (rel >= count) return;
    const long long group = first_group + rel;
    const int env = (int)(group / legal);
    const int objective = a.n > 3 ? a.geti(env, 3) : 0;
    const double* p = parts + group * chunks * 6;
    TbxLookFields best{0, 0, 0, 0, 0};
    uint32_t best_code = 0;
    bool none = true;
    for (int c = 0; c < chunks; c++, p += 6) {
        if (p[5] < 0.0) continue;
        const TbxLookFields f{(long long)p[0], (int)p[1], (int)p[2], (int)p[3], (int)p[4]};
        const uint32_t code = (uint32_t)p[5];
        if (none || tbx_search_better(objective, f, code, best, best_code)) { best = f; best_code = code; none = false; }
    }
    tbx_search_store(out + group * 6, best, best_code, none, false);
}

// TBX_QUERY_LOOKAHEAD_PLAN / _SEARCH: shared values are refused here, before anything is launched; per-env rows are met by the
// kernels.  The search is cut into chunks (tbx_search_chunks) and into launches over env ranges (tbx_range_step).
static int lookahead_plans(tbx_engine* e, int query, const TbxEditArgs& a, double* out_dev, hipStream_t s)
{
    const bool search = query == TBX_QUERY_LOOKAHEAD_SEARCH;
    const int L = tbx_legal_count(e->game);
    if (a.n < 1 || a.n > (search ? MAX_ARGS_SEARCH : MAX_ARGS_PLAN))
        return e->fail(TBX_E_INVALID, search ? "search takes {frames[, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset]}" : "plan takes {frames[, hold, depth, code, rest, seed_lo, seed_hi, t, env_offset]}");
    long long plans = TBX_LOOKAHEAD_MAX_PLANS, frames = TBX_LOOKAHEAD_MAX_FRAMES;      // per-env rows: the most a valid row can ask for
    if (!a.per_env) {
        if (int rc = shared_frames_hold(e, a)) return rc;
        const double depth = a.n > 2 ? a.v[2] : search ? 1.0 : 0.0;
        if (!(depth >= (search ? 1.0 : 0.0) && depth <= (double)tbx_plan_max_depth(e->game))) return e->fail(TBX_E_INVALID, "lookahead: depth must be 0 (search: 1) .. TBX_PLAN_MAX_DEPTH(game)");
        const uint64_t count = tbx_plan_count(e->game, TbxEditArgs::to_int(depth));
        if (search && count > (uint64_t)TBX_LOOKAHEAD_MAX_PLANS) return e->fail(TBX_E_INVALID, "search: n_legal^depth must not exceed TBX_LOOKAHEAD_MAX_PLANS");
        if (search)
            if (int rc = shared_objective(e, "search", a)) return rc;
        if (!search && a.n > 3 && !(a.v[3] >= 0.0 && a.v[3] < (double)count)) return e->fail(TBX_E_INVALID, "plan: code must be 0 .. n_legal^depth - 1");
        if (int rc = shared_action(e, a, 4, "rest")) return rc;
        plans = (long long)count;
        frames = TbxEditArgs::to_int(a.v[0]);
    }
    TbxPlanLaunch l{};
    l.query = query;
    l.envs = e->n;
    l.rows = out_dev;
    if (!search) return e->ops->lookahead_play(e, a, l, s);
    const int chunks = tbx_search_chunks(e->n, L, plans / L, e->ops->search_lanes());
    double* rows = out_dev;
    if (chunks > 1) {
        EHIP(e->search_parts.reserve(sizeof(double) * 6 * (size_t)e->n * (size_t)L * (size_t)chunks, e->stream, s));
        rows = e->search_parts.p;
    }
    e->search_chunks = chunks;
    l.chunks = chunks;
    l.rows = rows;
    int rc = TBX_OK;
    tbx_each_range(e->n, tbx_range_step(e->n, TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH, plans * frames, (long long)L * chunks), [&](int env0, int envs) {
        if (rc) return;
        l.first_env = env0;
        l.envs = envs;
        rc = e->ops->lookahead_play(e, a, l, s);
        if (rc || chunks == 1) return;
        const int groups = envs * L;
        hipLaunchKernelGGL(tbx_search_pick_kernel, dim3((groups + 255) / 256), dim3(256), 0, s, rows, a, L, chunks, (long long)env0 * L, groups, out_dev);
    });
    if (rc) return rc;
    EHIP(hipGetLastError());
    return TBX_OK;
}

// TBX_QUERY_LOOKAHEAD_BEAM, between two levels: one wave per (env, first action) group of envs from first_env on.  It stages the
// group's candidates of `level` (at most TBX_BEAM_MAX_WIDTH * 6 = 384) in LDS, ranks each by COUNTING the candidates that beat it
// under tbx_search_better -- codes within a level are distinct, so the ranks are a permutation and a pure function of the
// candidate set: no atomics, no sort network, nothing that depends on the launch shape -- and writes the candidate of rank
// r < width to slot r of the next beam; on the env's last level rank 0 goes to the output row.  A refused env's rows are zeros,
// written at level 1; an env whose depth is below `level` idles.
constexpr int TBX_BEAM_MAX_CANDS = TBX_BEAM_MAX_WIDTH * 6;
__global__ __launch_bounds__(64) void tbx_beam_select_kernel(TbxEditArgs a, int game, int level, int first_env, TbxBeamScratch sc, double* __restrict__ out)
{
    __shared__ TbxBeamCand lds[TBX_BEAM_MAX_CANDS];
    const int L = tbx_legal_count(game);
    const int group = blockIdx.x, lane = threadIdx.x;
    const int env = first_env + group / L;
    double* const o = out + ((size_t)first_env * L + group) * 6;
    int depth, objective, width;
    if (!tbx_beam_row(game, a, env, depth, objective, width)) {
        if (level == 1 && lane < 6) o[lane] = 0.0;
        return;
    }
    if (level > depth) return;
    const int n = level == 1 ? 1 : tbx_beam_kept(L, width, level - 1) * L;       // at most width * L
    const TbxBeamCand* const c = sc.cands + (size_t)group * sc.stride * L;
    for (int i = lane; i < n; i += 64) lds[i] = c[i];
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const TbxBeamCand x = lds[i];
        int rank = 0;
        for (int j = 0; j < n; j++) rank += j != i && tbx_search_better(objective, lds[j].f, lds[j].code, x.f, x.code) ? 1 : 0;
        if (level < depth && rank < width) sc.beam_out[(size_t)group * sc.stride + rank] = x.code;
        if (level == depth && rank == 0) tbx_search_store(o, x.f, x.code, false, false);
    }
}

// TBX_QUERY_LOOKAHEAD_BEAM: shared values are refused here, before anything is launched; per-env rows are met by the kernels.
// Env ranges keep a launch under TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH leaf-frames and TBX_LOOKAHEAD_PAIRS_PER_LAUNCH units and the
// scratch under TBX_BEAM_SCRATCH_BYTES (per-env rows: budgeted as the largest valid row, and every level up to
// TBX_PLAN_MAX_DEPTH runs -- the device form cannot see the rows; a shallower env writes its row at its own last level and idles
// afterwards).  Within a range, per level: play, select -- all on `s`, in stream order, no host synchronisation.
static int lookahead_beam(tbx_engine* e, const TbxEditArgs& a, double* out_dev, hipStream_t s)
{
    const int L = tbx_legal_count(e->game);
    if (a.n < 1 || a.n > MAX_ARGS_BEAM) return e->fail(TBX_E_INVALID, "beam takes {frames[, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, width]}");
    long long frames = TBX_LOOKAHEAD_MAX_FRAMES;      // per-env rows: the most a valid row can ask for
    int depth = tbx_plan_max_depth(e->game), width = TBX_BEAM_MAX_WIDTH;
    if (!a.per_env) {
        const double dp = a.n > 2 ? a.v[2] : 1.0, w = a.n > 9 ? a.v[9] : 1.0;
        if (int rc = shared_frames_hold(e, a)) return rc;
        if (int rc = shared_depth(e, "beam", dp, 1)) return rc;
        if (int rc = shared_objective(e, "beam", a)) return rc;
        if (int rc = shared_action(e, a, 4, "rest")) return rc;
        if (int rc = shared_width(e, "beam", w)) return rc;
        frames = TbxEditArgs::to_int(a.v[0]);
        depth = TbxEditArgs::to_int(dp);
        width = TbxEditArgs::to_int(w);
    }
    // per env: L groups of at most width * L candidates, and two beams of width codes per group
    const long long units_per_env = (long long)L * width * L;
    const size_t bytes_per_env = (size_t)units_per_env * sizeof(TbxBeamCand) + 2 * (size_t)L * width * sizeof(uint32_t);
    const long long step = tbx_range_step(e->n, TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH, units_per_env * frames, units_per_env, bytes_per_env, e->beam_range_envs);
    EHIP(e->beam_scratch.reserve(bytes_per_env * (size_t)step, e->stream, s));
    TbxBeamScratch sc;
    sc.stride = width;
    sc.cands = reinterpret_cast<TbxBeamCand*>(e->beam_scratch.p);
    sc.beam_in = reinterpret_cast<uint32_t*>(e->beam_scratch.p + (size_t)units_per_env * sizeof(TbxBeamCand) * (size_t)step);
    sc.beam_out = sc.beam_in + (size_t)L * width * (size_t)step;
    TbxPlanLaunch l{};
    l.query = TBX_QUERY_LOOKAHEAD_BEAM;
    int rc = TBX_OK;
    const int ranges = tbx_each_range(e->n, step, [&](int env0, int envs) {
        l.first_env = env0;
        l.envs = envs;
        for (int level = 1; !rc && level <= depth; level++) {
            l.level = level;
            l.slots = tbx_beam_kept(L, width, level - 1);
            l.beam = sc;
            rc = e->ops->lookahead_play(e, a, l, s);
            if (rc) return;
            hipLaunchKernelGGL(tbx_beam_select_kernel, dim3((unsigned)(envs * L)), dim3(64), 0, s, a, e->game, level, env0, sc, out_dev);
            uint32_t* const t = sc.beam_in; sc.beam_in = sc.beam_out; sc.beam_out = t;
        }
    });
    if (rc) return rc;
    e->beam_ranges = ranges;
    EHIP(hipGetLastError());
    return TBX_OK;
}

// TBX_QUERY_LOOKAHEAD_EVOLVE, after the play of generation `gen`: one wave per (env, first action) group of envs from first_env on.
// It stages the group's population (at most TBX_EVOLVE_MAX_POPULATION records, 8 KiB) in LDS and ranks each individual by COUNTING
// those that beat it, as tbx_beam_select_kernel does -- two individuals of one code are one plan with one record, and the smaller
// index goes first, so the ranks are a permutation and a pure function of the population.  In the env's last generation rank 0
// goes to the output row.  Earlier it writes the next generation: the record and code of rank r < elite into slot r (nobody
// replays them), and per child a lane that draws its parent among the elites and mutates the parent's digits, in 32-bit
// arithmetic (a Breakout code reaches 2^32 - 1).  A refused env's rows are zeros, written at generation 0; an env whose
// generations are below `gen` idles.
__global__ __launch_bounds__(64) void tbx_evolve_select_kernel(TbxEditArgs a, int game, int gen, int first_env, TbxEvolveScratch sc, double* __restrict__ out)
{
    __shared__ TbxBeamCand lds[TBX_EVOLVE_MAX_POPULATION];
    __shared__ uint16_t by_rank[TBX_EVOLVE_MAX_POPULATION];
    const uint32_t L = (uint32_t)tbx_legal_count(game);
    const int group = blockIdx.x, lane = threadIdx.x;
    const int env = first_env + group / (int)L, cand = group % (int)L;
    double* const o = out + ((size_t)first_env * L + group) * 6;
    TbxEvolveRow r;
    if (!tbx_evolve_row(game, a, env, r)) {
        if (gen == 0 && lane < 6) o[lane] = 0.0;
        return;
    }
    if (gen > r.generations) return;
    const int n = r.population;
    TbxBeamCand* const recs = sc.recs + (size_t)group * sc.stride;
    uint32_t* const codes = sc.codes + (size_t)group * sc.stride;
    for (int i = lane; i < n; i += 64) lds[i] = recs[i];
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const TbxBeamCand x = lds[i];
        int rank = 0;
        for (int j = 0; j < n; j++) rank += tbx_search_better(r.objective, lds[j].f, lds[j].code, x.f, x.code) || (j < i && lds[j].code == x.code) ? 1 : 0;
        by_rank[rank] = (uint16_t)i;
        if (gen == r.generations && rank == 0) tbx_search_store(o, x.f, x.code, false, false);
    }
    if (gen == r.generations) return;
    __syncthreads();
    for (int k = lane; k < r.elite; k += 64) {
        const TbxBeamCand x = lds[by_rank[k]];
        recs[k] = x;
        codes[k] = x.code;
    }
    const uint64_t base = tbx_evolve_base(r.plan_seed, cand, (uint64_t)a.getu(env, 8) + (uint64_t)env);
    for (int i = r.elite + lane; i < n; i += 64) {
        uint32_t c = lds[by_rank[(uint32_t)(tbx_evolve_word(base, gen + 1, i, 0) >> 32) % (uint32_t)r.elite]].code;
        uint32_t code = c % L, pow = L;                                            // digit 0: the first action, every parent's
        c /= L;
        for (int p = 1; p < r.depth; p++, pow *= L, c /= L) {
            const uint64_t x = tbx_evolve_word(base, gen + 1, i, p);
            const uint32_t digit = (int)(x & 0xff) < r.mutation ? (uint32_t)(x >> 32) % L : c % L;
            code += digit * pow;
        }
        codes[i] = code;
    }
}

// What a TBX_QUERY_LOOKAHEAD_EVOLVE is budgeted for: the largest frames, population and generations of a valid row and the
// smallest elite (nobody's unit after generation 0)
struct TbxEvolveBounds {
    long long frames;
    int population, generations, elite;
};
// tbx_reduce has per-env rows on the host: the bounds of the rows that tbx_evolve_values accepts (none: the smallest query)
static TbxEvolveBounds evolve_scan(const tbx_engine* e, const double* rows, int n)
{
    TbxEvolveBounds b{1, 1, 0, 1};
    bool any = false;
    for (int env = 0; env < e->n; env++) {
        const double* const r = rows + (size_t)env * n;
        auto geti = [&](int i, int otherwise) { return i < n ? TbxEditArgs::to_int(r[i]) : otherwise; };
        const int frames = geti(0, 0), population = geti(9, 1), generations = geti(10, 0), elite = geti(11, 1);
        if (!tbx_evolve_values(e->game, frames, geti(1, 1), geti(2, 1), geti(3, 0), geti(4, -1), population, generations, elite, n > 12 ? r[12] : 0.0, geti(13, 64),
                               n > 14 ? r[14] : -1.0))
            continue;
        if (frames > b.frames) b.frames = frames;
        if (population > b.population) b.population = population;
        if (generations > b.generations) b.generations = generations;
        if (!any || elite < b.elite) b.elite = elite;
        any = true;
    }
    return b;
}

// the shared row of a TBX_QUERY_LOOKAHEAD_EVOLVE: refused here, before anything is launched, else its budget in `b`
static int evolve_shared_check(tbx_engine* e, const TbxEditArgs& a, TbxEvolveBounds& b)
{
    const double dp = a.n > 2 ? a.v[2] : 1.0, pop = a.n > 9 ? a.v[9] : 1.0, gens = a.n > 10 ? a.v[10] : 0.0, elite = a.n > 11 ? a.v[11] : 1.0;
    const double plan_seed = a.n > 12 ? a.v[12] : 0.0, mutation = a.n > 13 ? a.v[13] : 64.0, init = a.n > 14 ? a.v[14] : -1.0;
    if (int rc = shared_frames_hold(e, a)) return rc;
    if (int rc = shared_depth(e, "evolve", dp, 1)) return rc;
    if (int rc = shared_objective(e, "evolve", a)) return rc;
    if (int rc = shared_action(e, a, 4, "rest")) return rc;
    if (!(pop >= 1.0 && pop <= (double)TBX_EVOLVE_MAX_POPULATION)) return e->fail(TBX_E_INVALID, "evolve: population must be 1 .. TBX_EVOLVE_MAX_POPULATION");
    if (!(gens >= 0.0 && gens <= (double)TBX_EVOLVE_MAX_GENERATIONS)) return e->fail(TBX_E_INVALID, "evolve: generations must be 0 .. TBX_EVOLVE_MAX_GENERATIONS");
    b.frames = TbxEditArgs::to_int(a.v[0]);
    b.population = TbxEditArgs::to_int(pop);
    b.generations = TbxEditArgs::to_int(gens);
    if (!(elite >= 1.0 && elite <= (double)b.population)) return e->fail(TBX_E_INVALID, "evolve: elite must be 1 .. population");
    b.elite = TbxEditArgs::to_int(elite);
    if (!(plan_seed >= 0.0 && plan_seed < 4294967296.0)) return e->fail(TBX_E_INVALID, "evolve: plan_seed must be 0 .. 2^32 - 1");
    if (!(mutation >= 0.0 && mutation <= 256.0)) return e->fail(TBX_E_INVALID, "evolve: mutation must be 0 .. 256");
    if (!(init == -1.0 || (init >= 0.0 && init < (double)tbx_plan_count(e->game, TbxEditArgs::to_int(dp))))) return e->fail(TBX_E_INVALID, "evolve: init must be -1 or 0 .. n_legal^depth - 1");
    return TBX_OK;
}

// TBX_QUERY_LOOKAHEAD_EVOLVE: shared values are refused here, before anything is launched; per-env rows are met by the kernels.
// Env ranges come from the beam's three budgets -- a launch under TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH leaf-frames and
// TBX_LOOKAHEAD_PAIRS_PER_LAUNCH units, the scratch under TBX_BEAM_SCRATCH_BYTES (starting values here as there: profiles/beam.md,
// profiles/evolve.md) -- and TBX_OPT_BEAM_RANGE_ENVS cuts them as it cuts the beam's.  Per env the scratch is L * population records
// and as many codes; beam_scratch is shared with the beam queries: all run in stream order.  Per-env rows are budgeted by `rows`
// where the host form has scanned them, else as the largest valid row with TBX_EVOLVE_MAX_GENERATIONS + 1 rounds run -- the device
// form cannot see the rows; an env writes its row at its own last generation and idles afterwards.  Within a range, per
// generation: play, select -- all on `s`, in stream order, no host synchronisation.
static int lookahead_evolve(tbx_engine* e, const TbxEditArgs& a, const TbxEvolveBounds* rows, double* out_dev, hipStream_t s)
{
    const int L = tbx_legal_count(e->game);
    if (a.n < 1 || a.n > MAX_ARGS_EVOLVE)
        return e->fail(TBX_E_INVALID, "evolve takes {frames[, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, population, generations, elite, plan_seed, mutation, init]}");
    // per-env rows the host has not seen: the most a valid row can ask for
    TbxEvolveBounds b{TBX_LOOKAHEAD_MAX_FRAMES, TBX_EVOLVE_MAX_POPULATION, TBX_EVOLVE_MAX_GENERATIONS, 1};
    if (!a.per_env) {
        const int rc = evolve_shared_check(e, a, b);
        if (rc) return rc;
    } else if (rows) b = *rows;
    // per env: L groups of `population` individuals -- a record and a code each
    const long long units_per_env = (long long)L * b.population;
    const size_t bytes_per_env = (size_t)units_per_env * (sizeof(TbxBeamCand) + sizeof(uint32_t));
    const long long step = tbx_range_step(e->n, TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH, units_per_env * b.frames, units_per_env, bytes_per_env, e->beam_range_envs);
    EHIP(e->beam_scratch.reserve(bytes_per_env * (size_t)step, e->stream, s));
    TbxEvolveScratch sc;
    sc.stride = b.population;
    sc.recs = reinterpret_cast<TbxBeamCand*>(e->beam_scratch.p);
    sc.codes = reinterpret_cast<uint32_t*>(e->beam_scratch.p + (size_t)units_per_env * sizeof(TbxBeamCand) * (size_t)step);
    TbxPlanLaunch l{};
    l.query = TBX_QUERY_LOOKAHEAD_EVOLVE;
    l.evolve = sc;
    int rc = TBX_OK;
    const int ranges = tbx_each_range(e->n, step, [&](int env0, int envs) {
        l.first_env = env0;
        l.envs = envs;
        for (int gen = 0; !rc && gen <= b.generations; gen++) {
            l.level = gen;
            l.first_slot = gen == 0 ? 0 : b.elite;
            l.slots = b.population - l.first_slot;
            if (l.slots > 0) {                                   // (elite = population: every later generation is carried whole)
                rc = e->ops->lookahead_play(e, a, l, s);
                if (rc) return;
            }
            hipLaunchKernelGGL(tbx_evolve_select_kernel, dim3((unsigned)(envs * L)), dim3(64), 0, s, a, e->game, gen, env0, sc, out_dev);
        }
    });
    if (rc) return rc;
    e->evolve_ranges = ranges;
    EHIP(hipGetLastError());
    return TBX_OK;
}

// What a TBX_QUERY_LOOKAHEAD_TREE is budgeted for: the largest frames and simulations of a valid row
struct TbxTreeBounds {
    long long frames;
    int simulations;
};
// tbx_reduce has per-env rows on the host: the bounds of the rows that tbx_tree_values accepts (none: the smallest query)
static TbxTreeBounds tree_scan(const tbx_engine* e, const double* rows, int n)
{
    TbxTreeBounds b{1, 1};
    for (int env = 0; env < e->n; env++) {
        const double* const r = rows + (size_t)env * n;
        auto geti = [&](int i, int otherwise) { return i < n ? TbxEditArgs::to_int(r[i]) : otherwise; };
        const int frames = geti(0, 0), simulations = geti(9, 1);
        if (!tbx_tree_values(e->game, frames, geti(1, 1), geti(2, 1), geti(3, 0), geti(4, -1), simulations, geti(10, 0), n > 11 ? r[11] : 0.0)) continue;
        if (frames > b.frames) b.frames = frames;
        if (simulations > b.simulations) b.simulations = simulations;
    }
    return b;
}

// ---- TBX_QUERY_LOOKAHEAD_TREE_ACT (include/toybox_amd.h): the tree query on start trees, then pick and carry per env range.

// What lookahead_tree does on top of query 160 when it runs for query 161: where the working trees start from, where the L rows
// of an env go before the pick, and what the carry writes.  The store's blocks have TbxTreeScratch's layout at store_stride.
struct TbxTreeAct {
    uint8_t* store;            // TBX_BUF_PLAN_TREE
    uint8_t* drop;             // [N] drop flags
    int32_t* action;           // TBX_BUF_PLAN_ACTION
    double* rows;              // [N][L][12] the tree's rows (act_scratch)
    int store_stride, live, keep, max_visits, objective;
};

// Step 1 for the units of one env range: one wave per unit.  A live carried tree is copied into the unit's working block, 16 bytes
// a lane and coalesced, with the node count put where the tree kernel keeps it (the root's `nodes`); any other unit gets 160's
// empty root.  The drop flags are read here and cleared by tbx_tree_carry_kernel, which runs behind every launch that reads them.
__global__ __launch_bounds__(64) void tbx_tree_load_kernel(TbxTreeAct t, int legal, int first_env, TbxTreeScratch sc)
{
    const int rel = blockIdx.x, lane = threadIdx.x;
    const int env = first_env + rel / legal;
    const uint8_t* const block = t.store + ((size_t)env * legal + rel % legal) * TbxTreeScratch::unit_bytes(t.store_stride);
    uint32_t count = t.live && !t.drop[env] ? *reinterpret_cast<const uint32_t*>(block) : 0u;
    if (count > (uint32_t)t.store_stride) count = 0;                                   // (never: the carry keeps at most simulations + 1)
    uint4* const dst = reinterpret_cast<uint4*>(sc.nodes(rel));
    if (count == 0) {
        if (lane < 2) dst[lane] = uint4{0u, 0u, lane == 1 ? 1u : 0u, 0u};              // bytes 24 .. 27 of node 0: nodes = 1
        return;
    }
    const uint4* const src = reinterpret_cast<const uint4*>(block + 64);
    for (uint32_t i = lane; i < 2 * count; i += 64) {
        uint4 v = src[i];
        if (i == 1) v.z = count;
        dst[i] = v;
    }
}

// Steps 3 and 4 for the envs of one range, one thread per env.  Pick: tbx_act_pick_kernel's sampled order on the L rows.  Carry: ONE
// ascending pass over the working tree a*.  A node of a kept subtree carries a tag in its `pad` word (free below the root; the
// working copy is dead after this kernel): the destination tree k, the parent's new id, the digit under it, and whether the
// tree is being halved.  The root tags its children as new roots; a tagged node that still fits under `keep` takes the next id of
// its tree -- the count in the block's first word is the counter -- writes itself with empty links, patches its parent's link and
// tags its own children.  Ids grow from parent to child, so every tag is in place before its node is met, a node past `keep` tags
// nobody, and its descendants fall with it.  Reads come from the range's working scratch and writes go to the store: tree a*'s own
// slot is written like any other.  Nothing here coalesces: profiles/tree_act.md.
__global__ __launch_bounds__(64) void tbx_tree_carry_kernel(TbxTreeAct t, int game, int first_env, int envs, TbxTreeScratch sc, double* __restrict__ out)
{
    constexpr uint32_t TAG = 1u << 31, NEW_ROOT = 1u << 30, HALVE = 1u << 29;
    const int rel = blockIdx.x * 64 + threadIdx.x;
    if (rel >= envs) return;
    const int env = first_env + rel, L = tbx_legal_count(game);
    const double* p = t.rows + (size_t)env * L * 12;
    TbxSearchSamplesKey bk{0, 0, 0};
    int best_a = 0;
    for (int a = 0; a < L; a++) {
        const TbxSearchSamplesKey k{(long long)p[a * 12 + 1], (int)p[a * 12 + 5], (int)p[a * 12 + 7]};
        if (a == 0 || tbx_search_samples_better(t.objective, k, (uint32_t)a, bk, (uint32_t)best_a)) { bk = k; best_a = a; }
    }
    const int ale = tbx_legal_action(game, best_a);
    double* const o = out + (size_t)env * 14;
    o[0] = (double)ale;
    o[1] = (double)best_a;
    for (int i = 0; i < 12; i++) o[2 + i] = p[best_a * 12 + i];
    t.action[env] = ale;
    t.drop[env] = 0;

    const size_t block_bytes = TbxTreeScratch::unit_bytes(t.store_stride);
    uint8_t* const blocks = t.store + (size_t)env * L * block_bytes;
    for (int k = 0; k < L; k++) {
        uint4* const line = reinterpret_cast<uint4*>(blocks + (size_t)k * block_bytes);
        for (int i = 0; i < 4; i++) line[i] = uint4{0u, 0u, 0u, 0u};
    }
    TbxTreeNode* const nd = sc.nodes(rel * L + best_a);
    const uint32_t count = nd[0].nodes;
    for (int k = 0; k < L; k++) {
        const uint32_t c = nd[0].child[k];
        if (c) nd[c].pad = TAG | NEW_ROOT | ((uint32_t)k << 20);
    }
    for (uint32_t id = 1; id < count; id++) {
        const TbxTreeNode src = nd[id];
        if (!(src.pad & TAG)) continue;
        const uint32_t k = (src.pad >> 20) & 7u;
        uint8_t* const block = blocks + (size_t)k * block_bytes;
        uint32_t* const counter = reinterpret_cast<uint32_t*>(block);
        TbxTreeNode* const dst = reinterpret_cast<TbxTreeNode*>(block + 64);
        const uint32_t id_new = *counter;
        if (id_new >= (uint32_t)t.keep) continue;
        *counter = id_new + 1;
        const bool halve = src.pad & NEW_ROOT ? src.n > (uint32_t)t.max_visits : (src.pad & HALVE) != 0;
        TbxTreeNode kept{};
        kept.v_sum = halve ? src.v_sum / 2 : src.v_sum;
        kept.n = halve ? (src.n + 1) / 2 : src.n;
        dst[id_new] = kept;
        if (!(src.pad & NEW_ROOT)) dst[src.pad & 0xffffu].child[(src.pad >> 16) & 7u] = (uint16_t)id_new;
        for (int j = 0; j < L; j++) {
            const uint32_t c = src.child[j];
            if (c) nd[c].pad = TAG | (halve ? HALVE : 0u) | (k << 20) | ((uint32_t)j << 16) | id_new;
        }
    }
}

// TBX_QUERY_LOOKAHEAD_TREE: shared values are refused here, before anything is launched; per-env rows are met by the kernel.  Env
// ranges come from the beam's three budgets -- a launch of ONE simulation per unit under TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH
// leaf-frames and TBX_LOOKAHEAD_PAIRS_PER_LAUNCH units, the scratch under TBX_BEAM_SCRATCH_BYTES -- and TBX_OPT_BEAM_RANGE_ENVS
// cuts them as it cuts the beam's.  Per env the scratch is L trees of simulations + 1 nodes (TbxTreeScratch); beam_scratch is shared
// with the beam queries and the evolution: all run in stream order, and the launch of simulation 0 makes its trees empty.  Within a
// range the simulations are cut into launches that stay under the leaf-frame budget (and under TBX_OPT_TREE_LAUNCH_SIMULATIONS);
// the trees persist in scratch between them.  Per-env rows are budgeted by `rows` where the host form has scanned them, else as
// the largest valid row -- the device form cannot see the rows; an env stores its row in the launch of its own last simulation and
// idles afterwards.  All on `s`, in stream order, no host synchronisation.
// tree_check holds the checks and answers the budget; tree_run cuts the ranges and launches.
// TBX_QUERY_LOOKAHEAD_TREE_ACT goes through both (`act`, lookahead_tree_act below): the same checks, and the same range cut -- its
// working trees have 2 * simulations + 1 nodes and its scratch budget is twice TBX_BEAM_SCRATCH_BYTES, so its env ranges are query
// 160's -- with the rows into act->rows, tbx_tree_load_kernel in front of a range's first launch and tbx_tree_carry_kernel behind its
// last, before the next range overwrites the scratch.
static int tree_check(tbx_engine* e, const TbxEditArgs& a, const TbxTreeBounds* rows, TbxTreeBounds& b)
{
    if (a.n < 1 || a.n > MAX_ARGS_TREE)
        return e->fail(TBX_E_INVALID, "tree takes {frames[, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, simulations, explore, salt]}");
    b = TbxTreeBounds{TBX_LOOKAHEAD_MAX_FRAMES, TBX_TREE_MAX_SIMULATIONS};      // per-env rows the host has not seen: the most a valid row can ask for
    if (!a.per_env) {
        const double dp = a.n > 2 ? a.v[2] : 1.0, sims = a.n > 9 ? a.v[9] : 1.0, explore = a.n > 10 ? a.v[10] : 0.0, salt = a.n > 11 ? a.v[11] : 0.0;
        if (int rc = shared_frames_hold(e, a)) return rc;
        if (int rc = shared_depth(e, "tree", dp, 1)) return rc;
        if (int rc = shared_objective(e, "tree", a)) return rc;
        if (int rc = shared_action(e, a, 4, "rest")) return rc;
        if (!(sims >= 1.0 && sims <= (double)TBX_TREE_MAX_SIMULATIONS)) return e->fail(TBX_E_INVALID, "tree: simulations must be 1 .. TBX_TREE_MAX_SIMULATIONS");
        if (!(explore >= 0.0 && explore <= (double)TBX_TREE_MAX_EXPLORE)) return e->fail(TBX_E_INVALID, "tree: explore must be 0 .. TBX_TREE_MAX_EXPLORE");
        b.frames = TbxEditArgs::to_int(a.v[0]);
        b.simulations = TbxEditArgs::to_int(sims);
        if (int rc = shared_salt(e, "tree", salt, b.simulations)) return rc;
    } else if (rows) b = *rows;
    return TBX_OK;
}

static int tree_run(tbx_engine* e, const TbxEditArgs& a, const TbxTreeBounds& b, double* out_dev, hipStream_t s, const TbxTreeAct* act)
{
    const int L = tbx_legal_count(e->game);
    const int stride = TbxTreeScratch::stride_for(act ? 2 * b.simulations : b.simulations);
    const size_t bytes_per_env = (size_t)L * TbxTreeScratch::unit_bytes(stride);
    const long long step = tbx_range_step(e->n, TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH, (long long)L * b.frames, L, bytes_per_env, e->beam_range_envs,
                                          act ? 2 * TBX_BEAM_SCRATCH_BYTES : TBX_BEAM_SCRATCH_BYTES);
    EHIP(e->beam_scratch.reserve(bytes_per_env * (size_t)step, e->stream, s));
    TbxPlanLaunch l{};
    l.query = TBX_QUERY_LOOKAHEAD_TREE;
    l.rows = act ? act->rows : out_dev;
    l.tree.base = e->beam_scratch.p;
    l.tree.stride = stride;
    l.tree.preloaded = act ? 1 : 0;
    int rc = TBX_OK;
    const int ranges = tbx_each_range(e->n, step, [&](int env0, int envs) {
        l.first_env = env0;
        l.envs = envs;
        long long per_launch = TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH / ((long long)envs * L * b.frames);
        if (e->tree_launch_simulations > 0 && per_launch > e->tree_launch_simulations) per_launch = e->tree_launch_simulations;
        if (per_launch > b.simulations) per_launch = b.simulations;
        if (per_launch < 1) per_launch = 1;
        if (act && !rc) {
            hipLaunchKernelGGL(tbx_tree_load_kernel, dim3((unsigned)(envs * L)), dim3(64), 0, s, *act, L, env0, l.tree);
            if (hipGetLastError() != hipSuccess) rc = e->fail(TBX_E_NO_DEVICE, "tree act: the start-tree launch failed");
        }
        for (int m0 = 0; !rc && m0 < b.simulations; m0 += (int)per_launch) {
            l.first_slot = m0;
            l.slots = (int)(b.simulations - m0 < per_launch ? b.simulations - m0 : per_launch);
            rc = e->ops->lookahead_play(e, a, l, s);
        }
        if (act && !rc) {
            hipLaunchKernelGGL(tbx_tree_carry_kernel, dim3((unsigned)((envs + 63) / 64)), dim3(64), 0, s, *act, e->game, env0, envs, l.tree, out_dev);
            if (hipGetLastError() != hipSuccess) rc = e->fail(TBX_E_NO_DEVICE, "tree act: the carry launch failed");
        }
    });
    if (rc) return rc;
    e->tree_ranges = ranges;
    EHIP(hipGetLastError());
    return TBX_OK;
}

static int lookahead_tree(tbx_engine* e, const TbxEditArgs& a, const TbxTreeBounds* rows, double* out_dev, hipStream_t s)
{
    TbxTreeBounds b;
    if (int rc = tree_check(e, a, rows, b)) return rc;
    return tree_run(e, a, b, out_dev, s, nullptr);
}

// chunks > 1: the sum of the partial rows parts[group][chunks][8] (64-bit integers; fields 2 / 3: the smallest / the largest) of
// every (env, first action) group of envs from first_env on; a group without a sample (a refused row) answers zeros
__global__ __launch_bounds__(256) void tbx_sample_sum_kernel(const long long* __restrict__ parts, int chunks, long long first_group, int count, double* __restrict__ out)
{
    const int rel = blockIdx.x * 256 + threadIdx.x;
    if (rel >= count) return;
    const long long group = first_group + rel;
    const long long* p = parts + group * chunks * 8;
    TbxSampleSums sum;
    for (int c = 0; c < chunks; c++, p += 8) sum.merge(p);
    sum.store(out + group * 8);
}

// TBX_QUERY_LOOKAHEAD_SAMPLES: shared values are refused here, before anything is launched; per-env rows are met by the kernel.
// Cut into chunks and launches as the search is, with the samples of a group where the search has its suffixes.
static int lookahead_samples(tbx_engine* e, const TbxEditArgs& a, double* out_dev, hipStream_t s)
{
    const int L = tbx_legal_count(e->game);
    if (a.n < 1 || a.n > MAX_ARGS_SAMPLES) return e->fail(TBX_E_INVALID, "samples takes {frames[, hold, samples, salt, rest, seed_lo, seed_hi, t, env_offset]}");
    long long samples = TBX_LOOKAHEAD_MAX_SAMPLES, frames = TBX_LOOKAHEAD_MAX_FRAMES;      // per-env rows: the most a valid row can ask for
    if (!a.per_env) {
        if (int rc = shared_frames_hold(e, a)) return rc;
        const double count = a.n > 2 ? a.v[2] : 1.0, salt = a.n > 3 ? a.v[3] : 0.0;
        if (int rc = shared_samples(e, "samples", count)) return rc;
        samples = TbxEditArgs::to_int(count);
        if (int rc = shared_salt(e, "samples", salt, samples)) return rc;
        if (int rc = shared_action(e, a, 4, "rest")) return rc;
        frames = TbxEditArgs::to_int(a.v[0]);
    }
    const int chunks = tbx_search_chunks(e->n, L, samples, e->ops->search_lanes());
    double* rows = out_dev;
    if (chunks > 1) {
        EHIP(e->sample_parts.reserve(sizeof(double) * 8 * (size_t)e->n * (size_t)L * (size_t)chunks, e->stream, s));
        rows = e->sample_parts.p;
    }
    e->sample_chunks = chunks;
    TbxPlanLaunch l{};
    l.query = TBX_QUERY_LOOKAHEAD_SAMPLES;
    l.chunks = chunks;
    l.rows = rows;
    int rc = TBX_OK;
    tbx_each_range(e->n, tbx_range_step(e->n, TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH, samples * frames, (long long)L * chunks), [&](int env0, int envs) {
        if (rc) return;
        l.first_env = env0;
        l.envs = envs;
        rc = e->ops->lookahead_play(e, a, l, s);
        if (rc || chunks == 1) return;
        const int groups = envs * L;
        hipLaunchKernelGGL(tbx_sample_sum_kernel, dim3((groups + 255) / 256), dim3(256), 0, s, reinterpret_cast<const long long*>(rows), chunks, (long long)env0 * L, groups, out_dev);
    });
    if (rc) return rc;
    EHIP(hipGetLastError());
    return TBX_OK;
}

// chunks > 1: the winner among the partial rows parts[group][chunks][9] (64-bit integers; word 8 the code, -1: no plan behind
// the row) of every (env, first action) group of envs from first_env on, by the order of the search-samples kernel; a group
// without a plan (a refused row) answers zeros
__global__ __launch_bounds__(256) void tbx_search_samples_pick_kernel(const long long* __restrict__ parts, TbxEditArgs a, int legal, int chunks, long long first_group, int count,
                                                                      double* __restrict__ out)
{
    const int rel = blockIdx.x * 256 + threadIdx.x;
    if (rel >= count) return;
    const long long group = first_group + rel;
    const int env = (int)(group / legal);
    const int objective = a.n > 3 ? a.geti(env, 3) : 0;
    const long long* const p0 = parts + group * chunks * 9;
    TbxSearchSamplesKey best{0, 0, 0};
    uint32_t best_code = 0;
    int best_chunk = -1;
    for (int c = 0; c < chunks; c++) {
        const long long* p = p0 + (size_t)c * 9;
        if (p[8] < 0) continue;
        const TbxSearchSamplesKey key{p[1], (int)p[5], (int)p[7]};
        const uint32_t code = (uint32_t)p[8];
        if (best_chunk < 0 || tbx_search_samples_better(objective, key, code, best, best_code)) { best = key; best_code = code; best_chunk = c; }
    }
    TbxSampleSums win;
    if (best_chunk >= 0) win.merge(p0 + (size_t)best_chunk * 9);
    tbx_search_samples_store(out + group * 9, win, best_code, best_chunk < 0, false);
}

// TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES: shared values are refused here, before anything is launched; per-env rows are met by the
// kernel.  Chunks over the suffix codes (tbx_search_chunks), launches over env ranges under the game's own leaf-frame budget
// (tbx_search_samples_budget); per-env rows are budgeted as the largest valid row, TBX_LOOKAHEAD_MAX_LEAVES x TBX_LOOKAHEAD_MAX_FRAMES.
static int lookahead_search_samples(tbx_engine* e, const TbxEditArgs& a, double* out_dev, hipStream_t s)
{
    const int L = tbx_legal_count(e->game);
    if (a.n < 1 || a.n > MAX_ARGS_SEARCH_SAMPLES) return e->fail(TBX_E_INVALID, "search over samples takes {frames[, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, samples, salt]}");
    long long suffixes = TBX_LOOKAHEAD_MAX_PLANS / L, leaves = TBX_LOOKAHEAD_MAX_LEAVES, frames = TBX_LOOKAHEAD_MAX_FRAMES;      // per-env rows: the most a valid row can ask for
    if (!a.per_env) {
        if (int rc = shared_frames_hold(e, a)) return rc;
        const double depth = a.n > 2 ? a.v[2] : 1.0;
        if (int rc = shared_depth(e, "search over samples", depth, 1)) return rc;
        const uint64_t plans = tbx_plan_count(e->game, TbxEditArgs::to_int(depth));
        if (plans > (uint64_t)TBX_LOOKAHEAD_MAX_PLANS) return e->fail(TBX_E_INVALID, "search over samples: n_legal^depth must not exceed TBX_LOOKAHEAD_MAX_PLANS");
        if (int rc = shared_objective(e, "search over samples", a)) return rc;
        if (int rc = shared_action(e, a, 4, "rest")) return rc;
        const double count = a.n > 9 ? a.v[9] : 1.0, salt = a.n > 10 ? a.v[10] : 0.0;
        if (int rc = shared_samples(e, "search over samples", count)) return rc;
        const long long samples = TbxEditArgs::to_int(count);
        if ((long long)plans * samples > (long long)TBX_LOOKAHEAD_MAX_LEAVES) return e->fail(TBX_E_INVALID, "search over samples: n_legal^depth * samples must not exceed TBX_LOOKAHEAD_MAX_LEAVES");
        if (int rc = shared_salt(e, "search over samples", salt, samples)) return rc;
        suffixes = (long long)plans / L;
        leaves = (long long)plans * samples;
        frames = TbxEditArgs::to_int(a.v[0]);
    }
    const int lanes = e->ops->search_lanes();
    const int chunks = tbx_search_chunks(e->n, L, suffixes, lanes);
    double* rows = out_dev;
    if (chunks > 1) {
        EHIP(e->search_samples_parts.reserve(sizeof(double) * 9 * (size_t)e->n * (size_t)L * (size_t)chunks, e->stream, s));
        rows = e->search_samples_parts.p;
    }
    e->search_samples_chunks = chunks;
    TbxPlanLaunch l{};
    l.query = TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES;
    l.chunks = chunks;
    l.rows = rows;
    int rc = TBX_OK;
    e->search_samples_launches = tbx_each_range(e->n, tbx_range_step(e->n, tbx_search_samples_budget(e->game, lanes), leaves * frames, (long long)L * chunks), [&](int env0, int envs) {
        if (rc) return;
        l.first_env = env0;
        l.envs = envs;
        rc = e->ops->lookahead_play(e, a, l, s);
        if (rc || chunks == 1) return;
        const int groups = envs * L;
        hipLaunchKernelGGL(tbx_search_samples_pick_kernel, dim3((groups + 255) / 256), dim3(256), 0, s, reinterpret_cast<const long long*>(rows), a, L, chunks, (long long)env0 * L, groups, out_dev);
    });
    if (rc) return rc;
    EHIP(hipGetLastError());
    return TBX_OK;
}

// TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES, between two levels: one wave per (env, first action) group of envs from first_env on, as
// tbx_beam_select_kernel.  Per candidate it merges the `chunks` partial records of the play launch (TbxSampleSums::merge: integers,
// so the result does not depend on the cut; a chunk without a sample is skipped) and stages in LDS only what the order reads --
// TbxSearchSamplesKey and the code, 24 bytes a candidate -- then ranks by COUNTING under tbx_search_samples_better and writes the
// candidate of rank r < width to slot r of the next beam; on the env's last level rank 0 merges its full eight sums from scratch
// and stores the row of 9.  A refused env's rows are zeros, written at level 1; an env whose depth is below `level` idles.
struct TbxBeamSamplesCand {
    TbxSearchSamplesKey key;
    uint32_t code;
};
__global__ __launch_bounds__(64) void tbx_beam_samples_select_kernel(TbxEditArgs a, int game, int level, int slots, int chunks, int first_env, TbxBeamSamplesScratch sc,
                                                                     double* __restrict__ out)
{
    __shared__ TbxBeamSamplesCand lds[TBX_BEAM_MAX_CANDS];
    const int L = tbx_legal_count(game);
    const int group = blockIdx.x, lane = threadIdx.x;
    const int env = first_env + group / L;
    double* const o = out + ((size_t)first_env * L + group) * 9;
    int depth, objective, width, S;
    uint64_t salt;
    if (!tbx_beam_samples_row(game, a, env, depth, objective, width, S, salt)) {
        if (level == 1 && lane < 9) o[lane] = 0.0;
        return;
    }
    if (level > depth) return;
    const int kids = level == 1 ? 1 : L;
    const int n = tbx_beam_kept(L, width, level - 1) * kids;                     // at most width * L
    const long long* const recs = sc.recs + (size_t)group * slots * kids * chunks * 9;
    for (int i = lane; i < n; i += 64) {
        const long long* const p = recs + (size_t)i * chunks * 9;
        TbxSampleSums sum;
        for (int c = 0; c < chunks; c++) sum.merge(p + (size_t)c * 9);
        lds[i] = TbxBeamSamplesCand{TbxSearchSamplesKey{sum.ret_sum, (int)sum.lost, (int)sum.safe_sum}, (uint32_t)p[8]};
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const TbxBeamSamplesCand x = lds[i];
        int rank = 0;
        for (int j = 0; j < n; j++) rank += j != i && tbx_search_samples_better(objective, lds[j].key, lds[j].code, x.key, x.code) ? 1 : 0;
        if (level < depth && rank < width) sc.beam_out[(size_t)group * sc.stride + rank] = x.code;
        if (level == depth && rank == 0) {
            const long long* const p = recs + (size_t)i * chunks * 9;
            TbxSampleSums win;
            for (int c = 0; c < chunks; c++) win.merge(p + (size_t)c * 9);
            tbx_search_samples_store(o, win, x.code, false, false);
        }
    }
}

// What a TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES is budgeted for: the largest frames, depth, width and samples of a valid row and the most
// leaves (candidates of the last level x samples) a valid row plays in one level
struct TbxBeamSamplesBounds {
    long long frames;
    int depth, width, samples;
    long long leaves;
};
// tbx_reduce has per-env rows on the host: the bounds of the rows that tbx_beam_samples_values accepts (none: the smallest query)
static TbxBeamSamplesBounds beam_samples_scan(const tbx_engine* e, const double* rows, int n)
{
    const int L = tbx_legal_count(e->game);
    TbxBeamSamplesBounds b{1, 1, 1, 1, 1};
    for (int env = 0; env < e->n; env++) {
        const double* const r = rows + (size_t)env * n;
        auto geti = [&](int i, int otherwise) { return i < n ? TbxEditArgs::to_int(r[i]) : otherwise; };
        const int frames = geti(0, 0), depth = geti(2, 1), width = geti(9, 1), samples = geti(10, 1);
        if (!tbx_beam_samples_values(e->game, frames, geti(1, 1), depth, geti(3, 0), geti(4, -1), width, samples, n > 11 ? r[11] : 0.0)) continue;
        const long long leaves = (long long)L * tbx_beam_kept(L, width, depth - 1) * (depth == 1 ? 1 : L) * samples;
        if (frames > b.frames) b.frames = frames;
        if (depth > b.depth) b.depth = depth;
        if (width > b.width) b.width = width;
        if (samples > b.samples) b.samples = samples;
        if (leaves > b.leaves) b.leaves = leaves;
    }
    return b;
}

// TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES: shared values are refused here, before anything is launched; per-env rows are met by the
// kernels.  Env ranges keep a level's play launch under tbx_search_samples_budget leaf-frames (it runs the sample kernel's loop, so
// that kernel's measured rates apply) and TBX_LOOKAHEAD_PAIRS_PER_LAUNCH units and the scratch under TBX_BEAM_SCRATCH_BYTES
// (beam_scratch is shared with TBX_QUERY_LOOKAHEAD_BEAM: both run in stream order).  Per-env rows are budgeted by `rows` where the
// host form has scanned them, else as the largest valid row with every level up to TBX_PLAN_MAX_DEPTH run.  Each level cuts the
// samples into the smallest power of two of chunks that brings its units to TBX_SEARCH_FILL_WAVES waves -- level 1 has one
// candidate per group --, at most the largest power of two <= samples and at most TBX_OPT_BEAM_SAMPLES_MAX_CHUNKS where set; a
// chunked level has fewer than 2 * TBX_SEARCH_FILL_WAVES * 64 units, so its records (9.4 MB at most) stay under the scratch bound
// too.  Within a range, per level: play, select -- all on `s`, in stream order, no host synchronisation.
static int lookahead_beam_samples(tbx_engine* e, const TbxEditArgs& a, const TbxBeamSamplesBounds* rows, double* out_dev, hipStream_t s)
{
    const int L = tbx_legal_count(e->game);
    if (a.n < 1 || a.n > MAX_ARGS_BEAM_SAMPLES) return e->fail(TBX_E_INVALID, "beam over samples takes {frames[, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, width, samples, salt]}");
    // per-env rows the host has not seen: the most a valid row can ask for
    TbxBeamSamplesBounds b{TBX_LOOKAHEAD_MAX_FRAMES, tbx_plan_max_depth(e->game), TBX_BEAM_MAX_WIDTH, TBX_LOOKAHEAD_MAX_SAMPLES, TBX_LOOKAHEAD_MAX_LEAVES};
    if (!a.per_env) {
        if (int rc = shared_frames_hold(e, a)) return rc;
        const double dp = a.n > 2 ? a.v[2] : 1.0, w = a.n > 9 ? a.v[9] : 1.0, count = a.n > 10 ? a.v[10] : 1.0, salt = a.n > 11 ? a.v[11] : 0.0;
        if (int rc = shared_depth(e, "beam over samples", dp, 1)) return rc;
        if (int rc = shared_objective(e, "beam over samples", a)) return rc;
        if (int rc = shared_action(e, a, 4, "rest")) return rc;
        if (int rc = shared_width(e, "beam over samples", w)) return rc;
        if (int rc = shared_samples(e, "beam over samples", count)) return rc;
        b.frames = TbxEditArgs::to_int(a.v[0]);
        b.depth = TbxEditArgs::to_int(dp);
        b.width = TbxEditArgs::to_int(w);
        b.samples = TbxEditArgs::to_int(count);
        if (int rc = shared_salt(e, "beam over samples", salt, b.samples)) return rc;
        b.leaves = (long long)L * tbx_beam_kept(L, b.width, b.depth - 1) * (b.depth == 1 ? 1 : L) * b.samples;
        if (b.leaves > (long long)TBX_LOOKAHEAD_MAX_LEAVES)
            return e->fail(TBX_E_INVALID, "beam over samples: the candidates of the last level x samples must not exceed TBX_LOOKAHEAD_MAX_LEAVES");
    } else if (rows) b = *rows;
    const int lanes = e->ops->search_lanes();
    // per env: L groups of at most width * L candidates, and two beams of width codes per group
    const long long units_per_env = (long long)L * b.width * L;
    const size_t beam_bytes_per_env = 2 * (size_t)L * b.width * sizeof(uint32_t), rec_bytes = 9 * sizeof(long long);
    const size_t bytes_per_env = (size_t)units_per_env * rec_bytes + beam_bytes_per_env;
    const long long step = tbx_range_step(e->n, tbx_search_samples_budget(e->game, lanes), b.leaves * b.frames, units_per_env, bytes_per_env, e->beam_range_envs);
    const long long want = TBX_SEARCH_FILL_WAVES * (64 / lanes);
    auto level_units = [&](long long envs, int level) { return envs * L * tbx_beam_kept(L, b.width, level - 1) * (level == 1 ? 1 : L); };
    auto level_chunks = [&](long long envs, int level) {
        const long long units = level_units(envs, level);
        int chunks = 1;
        while (units * chunks < want && 2 * chunks <= b.samples && (e->beam_samples_max_chunks == 0 || 2 * chunks <= e->beam_samples_max_chunks)) chunks *= 2;
        return chunks;
    };
    // the scratch is sized for the level where candidates x chunks is largest, over the full ranges and the last, shorter one
    long long most_units = 0;
    for (long long envs : {step, (long long)e->n % step})
        for (int level = 1; envs > 0 && level <= b.depth; level++) {
            const long long units = level_units(envs, level) * level_chunks(envs, level);
            if (units > most_units) most_units = units;
        }
    const size_t recs_bytes = (size_t)most_units * rec_bytes;
    EHIP(e->beam_scratch.reserve(recs_bytes + beam_bytes_per_env * (size_t)step, e->stream, s));
    TbxBeamSamplesScratch sc;
    sc.stride = b.width;
    sc.recs = reinterpret_cast<long long*>(e->beam_scratch.p);
    sc.beam_in = reinterpret_cast<uint32_t*>(e->beam_scratch.p + recs_bytes);
    sc.beam_out = sc.beam_in + (size_t)L * b.width * (size_t)step;
    TbxPlanLaunch l{};
    l.query = TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES;
    int rc = TBX_OK, most_chunks = 1;
    const int ranges = tbx_each_range(e->n, step, [&](int env0, int envs) {
        l.first_env = env0;
        l.envs = envs;
        for (int level = 1; !rc && level <= b.depth; level++) {
            l.level = level;
            l.slots = tbx_beam_kept(L, b.width, level - 1);
            l.chunks = level_chunks(envs, level);
            l.beam_samples = sc;
            if (l.chunks > most_chunks) most_chunks = l.chunks;
            rc = e->ops->lookahead_play(e, a, l, s);
            if (rc) return;
            hipLaunchKernelGGL(tbx_beam_samples_select_kernel, dim3((unsigned)(envs * L)), dim3(64), 0, s, a, e->game, level, l.slots, l.chunks, env0, sc, out_dev);
            uint32_t* const t = sc.beam_in; sc.beam_in = sc.beam_out; sc.beam_out = t;
        }
    });
    if (rc) return rc;
    e->beam_samples_ranges = ranges;
    e->beam_samples_chunks = most_chunks;
    EHIP(hipGetLastError());
    return TBX_OK;
}

// ---- TBX_QUERY_LOOKAHEAD_ACT (include/toybox_amd.h): a planner's rows stay in engine-owned scratch, every env's winner is picked
// on the device and its action left where the device-pointer steps read it.

// planner 158 with init = -2: the shared row (all 15 columns: -2 can only stand in the last) spread to per-env rows [n][15] with
// column 14 = carry % L^depth, the modulus in 64 bits (L^depth reaches 2^32).  One thread per env.
__global__ __launch_bounds__(256) void tbx_act_spread_kernel(TbxEditArgs a, int game, int n, const uint32_t* __restrict__ carry, double* __restrict__ rows)
{
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= n) return;
    const uint64_t count = tbx_plan_count(game, TbxEditArgs::to_int(a.v[2]));      // (the host has checked the depth)
    double* const r = rows + (size_t)env * 15;
#pragma unroll
    for (int i = 0; i < 14; i++) r[i] = a.v[i];
    r[14] = (double)(uint32_t)((uint64_t)carry[env] % count);
}

// The winner among an env's L rows of `width` doubles, one thread per env, the running best in registers and compared in integers as
// the select kernels compare (the rows are exact integers in binary64).  width 6, the rows of queries 153 / 156 / 158: the search's
// order, then the smaller code -- codes of different first actions differ in digit 0.  width 9, the rows of 155 / 157: the order of
// the sampled search on (ret_sum, lost, safe_frames_sum), then the smaller action index.  Out: {legal[a*], a*, the row zero-padded
// to 9}, the action and the carry = code / L + (code % L) * L^(depth-1) in 32-bit arithmetic: L^(depth-1) <= 2^30 and the sum is
// below L^depth <= 2^32.
__global__ __launch_bounds__(256) void tbx_act_pick_kernel(const double* __restrict__ rows, int game, int n, int width, int objective, int depth, double* __restrict__ out,
                                                           int32_t* __restrict__ action, uint32_t* __restrict__ carry)
{
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= n) return;
    const uint32_t L = (uint32_t)tbx_legal_count(game);
    const bool sampled = width == 9;
    const double* p = rows + (size_t)env * L * width;
    double best[9];
    TbxLookFields bf{0, 0, 0, 0, 0};
    TbxSearchSamplesKey bk{0, 0, 0};
    uint32_t best_tie = 0;
    int best_a = 0;
    for (int a = 0; a < (int)L; a++, p += width) {
        double r[9];
#pragma unroll
        for (int i = 0; i < 9; i++) r[i] = i < 6 || sampled ? p[i] : 0.0;
        const TbxLookFields f{(long long)r[0], (int)r[1], (int)r[2], (int)r[3], (int)r[4]};
        const TbxSearchSamplesKey k{(long long)r[1], (int)r[5], (int)r[7]};
        const uint32_t tie = sampled ? (uint32_t)a : (uint32_t)r[5];
        const bool better = a == 0 || (sampled ? tbx_search_samples_better(objective, k, tie, bk, best_tie) : tbx_search_better(objective, f, tie, bf, best_tie));
        if (better) {
#pragma unroll
            for (int i = 0; i < 9; i++) best[i] = r[i];
            bf = f; bk = k; best_tie = tie; best_a = a;
        }
    }
    const uint32_t code = (uint32_t)(sampled ? best[8] : best[5]);
    uint32_t pow = 1;
    for (int i = 1; i < depth; i++) pow *= L;
    const int ale = tbx_legal_action(game, best_a);
    double* const o = out + (size_t)env * 11;
    o[0] = (double)ale;
    o[1] = (double)best_a;
#pragma unroll
    for (int i = 0; i < 9; i++) o[2 + i] = best[i];
    action[env] = ale;
    carry[env] = code / L + (code % L) * pow;
}

// TBX_BUF_PLAN_ACTION / TBX_BUF_PLAN_CARRY: made and zeroed by the first TBX_QUERY_LOOKAHEAD_ACT that names a planner
static int act_alloc(tbx_engine* e)
{
    if (e->plan_action && e->plan_carry) return TBX_OK;
    EHIP(hipSetDevice(e->device));
    const size_t bytes = sizeof(int32_t) * (size_t)e->n;
    if (!e->plan_action) {
        EHIP(hipMalloc((void**)&e->plan_action, bytes));
        EHIP(hipMemsetAsync(e->plan_action, 0, bytes, e->stream));
    }
    if (!e->plan_carry) {
        EHIP(hipMalloc((void**)&e->plan_carry, bytes));
        EHIP(hipMemsetAsync(e->plan_carry, 0, bytes, e->stream));
    }
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

// TBX_QUERY_LOOKAHEAD_ACT: {planner, the planner's columns}.  The planner's own function refuses what it refuses, before anything is
// launched; its rows go to act_scratch, and the pick follows on `s`.  Planner 158 with init = -2: the shared row is checked with
// init = -1, spread to per-env rows with the carry in column 14, and lookahead_evolve runs on those rows under the SHARED row's
// bounds -- the path tbx_reduce's host scan takes, so budgets, slots and generations are those of the shared call.
static int lookahead_act(tbx_engine* e, const TbxEditArgs& a, double* out_dev, hipStream_t s)
{
    if (a.per_env) return e->fail(TBX_E_INVALID, "act takes shared arguments only");
    if (a.n < 1) return e->fail(TBX_E_INVALID, "act takes {planner, the planner's arguments}");
    const double pl = a.v[0];
    const int most = pl == (double)TBX_QUERY_LOOKAHEAD_SEARCH ? MAX_ARGS_SEARCH : pl == (double)TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES ? MAX_ARGS_SEARCH_SAMPLES :
                     pl == (double)TBX_QUERY_LOOKAHEAD_BEAM ? MAX_ARGS_BEAM : pl == (double)TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES ? MAX_ARGS_BEAM_SAMPLES :
                     pl == (double)TBX_QUERY_LOOKAHEAD_EVOLVE ? MAX_ARGS_EVOLVE : -1;
    if (most < 0) return e->fail(TBX_E_INVALID, "act: planner must be 153, 155, 156, 157 or 158");
    if (a.n - 1 > most) return e->fail(TBX_E_INVALID, "act: more arguments than the planner takes");
    const int planner = (int)pl;
    TbxEditArgs b;
    memset(&b, 0, sizeof b);
    b.n = a.n - 1;
    for (int i = 0; i < b.n; i++) b.v[i] = a.v[i + 1];
    const bool sampled = planner == TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES || planner == TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES;
    const bool from_carry = planner == TBX_QUERY_LOOKAHEAD_EVOLVE && b.n > 14 && b.v[14] == -2.0;
    TbxEvolveBounds bounds{1, 1, 0, 1};
    if (from_carry) {
        b.v[14] = -1.0;
        const int rc = evolve_shared_check(e, b, bounds);
        if (rc) return rc;
    }
    const int L = tbx_legal_count(e->game);
    int rc = act_alloc(e);
    if (rc) return rc;
    EHIP(e->act_scratch.reserve(sizeof(double) * (size_t)e->n * ((size_t)L * 9 + 15), e->stream, s));
    double* const rows = e->act_scratch.p;
    const unsigned blocks = (unsigned)((e->n + 255) / 256);
    if (from_carry) {
        double* const own = rows + (size_t)e->n * L * 9;
        hipLaunchKernelGGL(tbx_act_spread_kernel, dim3(blocks), dim3(256), 0, s, b, e->game, e->n, e->plan_carry, own);
        TbxEditArgs pe;
        memset(&pe, 0, sizeof pe);
        pe.n = 15;
        pe.per_env = own;
        rc = lookahead_evolve(e, pe, &bounds, rows, s);
    } else if (planner == TBX_QUERY_LOOKAHEAD_SEARCH) rc = lookahead_plans(e, planner, b, rows, s);
    else if (planner == TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES) rc = lookahead_search_samples(e, b, rows, s);
    else if (planner == TBX_QUERY_LOOKAHEAD_BEAM) rc = lookahead_beam(e, b, rows, s);
    else if (planner == TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES) rc = lookahead_beam_samples(e, b, nullptr, rows, s);
    else rc = lookahead_evolve(e, b, nullptr, rows, s);
    if (rc) return rc;
    const int depth = b.n > 2 ? TbxEditArgs::to_int(b.v[2]) : 1, objective = b.n > 3 ? TbxEditArgs::to_int(b.v[3]) : 0;
    hipLaunchKernelGGL(tbx_act_pick_kernel, dim3(blocks), dim3(256), 0, s, rows, e->game, e->n, sampled ? 9 : 6, objective, depth, out_dev, e->plan_action, e->plan_carry);
    EHIP(hipGetLastError());
    return TBX_OK;
}

// TBX_QUERY_LOOKAHEAD_TREE_ACT: {the tree's columns, reuse}.  tree_check refuses what query 160 refuses, before anything is launched
// or allocated; then the buffers are made (the action buffer by act_alloc; the store where there is none or `simulations` changed
// its size, zeroed; the flags once), liveness is decided on the host -- the key is host state, and calls are in order -- and
// tree_run's kernels follow on `s`.  The key is written LAST, once everything is queued: a call that fails after the checks
// leaves a key that matches nothing, so a half-written store is never live.  A call that allocates nothing does not synchronise.
static int lookahead_tree_act(tbx_engine* e, const TbxEditArgs& a, double* out_dev, hipStream_t s)
{
    if (a.per_env) return e->fail(TBX_E_INVALID, "tree act takes shared arguments only");
    if (a.n < 1 || a.n > MAX_ARGS_TREE + 1)
        return e->fail(TBX_E_INVALID, "tree act takes {frames[, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, simulations, explore, salt, reuse]}");
    const double reuse = a.n > MAX_ARGS_TREE ? a.v[MAX_ARGS_TREE] : 0.0;
    if (!(reuse == 0.0 || reuse == 1.0)) return e->fail(TBX_E_INVALID, "tree act: reuse must be 0 or 1");
    TbxEditArgs b = a;
    if (b.n > MAX_ARGS_TREE) b.n = MAX_ARGS_TREE;
    TbxTreeBounds bounds;
    if (int rc = tree_check(e, b, nullptr, bounds)) return rc;
    const int L = tbx_legal_count(e->game);
    if (int rc = act_alloc(e)) return rc;
    const int key[5] = {TbxEditArgs::to_int(b.v[0]), b.n > 1 ? TbxEditArgs::to_int(b.v[1]) : 1, b.n > 2 ? TbxEditArgs::to_int(b.v[2]) : 1,
                        b.n > 3 ? TbxEditArgs::to_int(b.v[3]) : 0, bounds.simulations};
    const int store_stride = TbxTreeScratch::stride_for(bounds.simulations);
    const size_t bytes = (size_t)e->n * L * TbxTreeScratch::unit_bytes(store_stride);
    bool live = reuse == 1.0 && e->plan_tree;
    for (int i = 0; i < 5; i++) live = live && key[i] == e->plan_tree_key[i];
    e->plan_tree_key[4] = 0;                                  // until this call is queued whole, nothing in the store is live
    if (!e->plan_tree_drop) {
        EHIP(hipMalloc((void**)&e->plan_tree_drop, (size_t)e->n));
        EHIP(hipMemsetAsync(e->plan_tree_drop, 0, (size_t)e->n, s));
    }
    if (!e->plan_tree || e->plan_tree_bytes != bytes) {
        live = false;
        EHIP(hipStreamSynchronize(e->stream));
        EHIP(hipStreamSynchronize(s));
        if (e->plan_tree) EHIP(hipFree(e->plan_tree));
        e->plan_tree = nullptr;
        e->plan_tree_bytes = 0;
        EHIP(hipMalloc((void**)&e->plan_tree, bytes));
        e->plan_tree_bytes = bytes;
        EHIP(hipMemsetAsync(e->plan_tree, 0, bytes, s));
    }
    EHIP(e->act_scratch.reserve(sizeof(double) * (size_t)e->n * L * 12, e->stream, s));
    TbxTreeAct act{};
    act.store = e->plan_tree;
    act.drop = e->plan_tree_drop;
    act.action = e->plan_action;
    act.rows = e->act_scratch.p;
    act.store_stride = store_stride;
    act.live = live ? 1 : 0;
    act.keep = e->tree_carry_keep > 0 && e->tree_carry_keep < bounds.simulations + 1 ? e->tree_carry_keep : bounds.simulations + 1;
    act.max_visits = e->tree_carry_max_visits > 0 ? e->tree_carry_max_visits : TBX_TREE_CARRY_MAX_VISITS;
    act.objective = key[3];
    if (int rc = tree_run(e, b, bounds, out_dev, s, &act)) return rc;
    for (int i = 0; i < 5; i++) e->plan_tree_key[i] = key[i];
    return TBX_OK;
}

// TBX_EDIT_TREE_DROP: the drop flag of every masked env (mask NULL: all), one thread per env
__global__ __launch_bounds__(256) void tbx_tree_drop_kernel(const uint8_t* __restrict__ mask, int n, uint8_t* __restrict__ drop)
{
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env < n && (!mask || mask[env])) drop[env] = 1;
}
static int tree_drop(tbx_engine* e, const TbxEditArgs& a, const uint8_t* mask_dev, hipStream_t s)
{
    if (a.n != 0) return e->fail(TBX_E_INVALID, "TBX_EDIT_TREE_DROP takes no arguments");
    if (!e->plan_tree || !e->plan_tree_drop) return e->fail(TBX_E_INVALID, "TBX_QUERY_LOOKAHEAD_TREE_ACT has not been called");
    hipLaunchKernelGGL(tbx_tree_drop_kernel, dim3((unsigned)((e->n + 255) / 256)), dim3(256), 0, s, mask_dev, e->n, e->plan_tree_drop);
    EHIP(hipGetLastError());
    return TBX_OK;
}

// the queries every game has (the engine's own), else the game's.  rows_host: tbx_reduce has the per-env rows on the host, a.n doubles
// an env -- queries 157, 158 and 160 then budget for the rows there are, not for the largest row there could be
static int engine_reduce(tbx_engine* e, int query, const TbxEditArgs& a, double* out_dev, int width, hipStream_t s, const double* rows_host = nullptr)
{
    if (query == TBX_QUERY_LOOKAHEAD || query == TBX_QUERY_LOOKAHEAD_ALL) {
        // shared values are refused here, before anything is launched; per-env rows are met by the kernel (that env's row: zeros)
        if (a.n < 1 || a.n > MAX_ARGS_LOOKAHEAD) return e->fail(TBX_E_INVALID, "lookahead takes {frames[, hold, first, rest, seed_lo, seed_hi, t, env_offset]}");
        if (!a.per_env) {
            if (int rc = shared_frames_hold(e, a)) return rc;
            if (query == TBX_QUERY_LOOKAHEAD)                    // (_ALL tries every first action and ignores the column)
                if (int rc = shared_action(e, a, 2, "first")) return rc;
            if (int rc = shared_action(e, a, 3, "rest")) return rc;
        }
        TbxPlanLaunch l{};
        l.query = query;
        l.envs = e->n;
        l.rows = out_dev;
        return e->ops->lookahead_play(e, a, l, s);
    }
    if (query == TBX_QUERY_LOOKAHEAD_PLAN || query == TBX_QUERY_LOOKAHEAD_SEARCH) return lookahead_plans(e, query, a, out_dev, s);
    if (query == TBX_QUERY_LOOKAHEAD_BEAM) return lookahead_beam(e, a, out_dev, s);
    if (query == TBX_QUERY_LOOKAHEAD_SAMPLES) return lookahead_samples(e, a, out_dev, s);
    if (query == TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES) return lookahead_search_samples(e, a, out_dev, s);
    if (query == TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES) {
        TbxBeamSamplesBounds seen;
        const bool scanned = rows_host && a.per_env && a.n <= MAX_ARGS_BEAM_SAMPLES;
        if (scanned) seen = beam_samples_scan(e, rows_host, a.n);
        return lookahead_beam_samples(e, a, scanned ? &seen : nullptr, out_dev, s);
    }
    if (query == TBX_QUERY_LOOKAHEAD_EVOLVE) {
        TbxEvolveBounds seen;
        const bool scanned = rows_host && a.per_env && a.n <= MAX_ARGS_EVOLVE;
        if (scanned) seen = evolve_scan(e, rows_host, a.n);
        return lookahead_evolve(e, a, scanned ? &seen : nullptr, out_dev, s);
    }
    if (query == TBX_QUERY_LOOKAHEAD_TREE) {
        TbxTreeBounds seen;
        const bool scanned = rows_host && a.per_env && a.n <= MAX_ARGS_TREE;
        if (scanned) seen = tree_scan(e, rows_host, a.n);
        return lookahead_tree(e, a, scanned ? &seen : nullptr, out_dev, s);
    }
    if (query == TBX_QUERY_LOOKAHEAD_ACT) return lookahead_act(e, a, out_dev, s);
    if (query == TBX_QUERY_LOOKAHEAD_TREE_ACT) return lookahead_tree_act(e, a, out_dev, s);
    if (query != TBX_QUERY_CHECKPOINT_VALID) return e->ops->reduce(e, query, a, out_dev, width, s);
    return checkpoint_valid(e, a, out_dev, s);
}

int tbx_edit_device(tbx_engine* e, int op, const double* args, int n_args, int per_env, const uint8_t* mask_dev, void* stream)
{
    CHECK_ENGINE(e);
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, (hipStream_t)stream));
    TbxEditArgs a;
    int rc = edit_args(e, args, n_args, per_env, false, (hipStream_t)stream, a);
    if (rc) return rc;
    if (op == TBX_EDIT_COPY_ENV) return fork_envs(e, a, mask_dev, false, (hipStream_t)stream);
    if (op == TBX_EDIT_CHECKPOINT_SLOTS) return e->fail(TBX_E_INVALID, "TBX_EDIT_CHECKPOINT_SLOTS has a host form only (tbx_edit)");
    if (op == TBX_EDIT_CHECKPOINT_SAVE || op == TBX_EDIT_CHECKPOINT_RESTORE)
        return checkpoint_copy(e, op == TBX_EDIT_CHECKPOINT_SAVE, a, mask_dev, false, (hipStream_t)stream);
    if (op == TBX_EDIT_TREE_DROP) return tree_drop(e, a, mask_dev, (hipStream_t)stream);
    return e->ops->edit(e, op, a, mask_dev, (hipStream_t)stream);
}

int tbx_edit(tbx_engine* e, int op, const double* args, int n_args, int per_env, const uint8_t* mask_host)
{
    CHECK_ENGINE(e);
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    if (op == TBX_EDIT_CHECKPOINT_SLOTS) {
        EHIP(hipStreamSynchronize(e->stream));                 // (nothing reads the old store any more)
        return checkpoint_slots(e, args, n_args, per_env, mask_host);
    }
    bool fork_direct = false;
    if (op == TBX_EDIT_COPY_ENV) {
        int rc = fork_check_host(e, args, n_args, per_env, mask_host, fork_direct);
        if (rc) return rc;
    }
    TbxEditArgs a;
    int rc = edit_args(e, args, n_args, per_env, true, e->stream, a);
    if (rc) return rc;
    const uint8_t* m = nullptr;
    if (mask_host) {
        EHIP(hipMemcpyAsync(e->mask, mask_host, (size_t)e->n, hipMemcpyHostToDevice, e->stream));
        m = e->mask;
    }
    if (op == TBX_EDIT_CHECKPOINT_SAVE || op == TBX_EDIT_CHECKPOINT_RESTORE) rc = checkpoint_copy(e, op == TBX_EDIT_CHECKPOINT_SAVE, a, m, true, e->stream);
    else if (op == TBX_EDIT_TREE_DROP) rc = tree_drop(e, a, m, e->stream);
    else rc = op == TBX_EDIT_COPY_ENV ? fork_envs(e, a, m, fork_direct, e->stream) : e->ops->edit(e, op, a, m, e->stream);
    if (rc) return rc;
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int tbx_reduce_device(tbx_engine* e, int query, const double* args, int n_args, int per_env, double* out_dev, void* stream)
{
    CHECK_ENGINE(e);
    const int width = tbx_reduce_width(e->game, query);
    if (width < 0) return e->fail(TBX_E_INVALID, "unknown query for this game");
    if (!out_dev) return e->fail(TBX_E_INVALID, "output pointer is NULL");
    if ((query == TBX_QUERY_LOOKAHEAD_ACT || query == TBX_QUERY_LOOKAHEAD_TREE_ACT) && per_env) return e->fail(TBX_E_INVALID, "act takes shared arguments only");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, (hipStream_t)stream));
    TbxEditArgs a;
    int rc = edit_args(e, args, n_args, per_env, false, (hipStream_t)stream, a);
    if (rc) return rc;
    return engine_reduce(e, query, a, out_dev, width, (hipStream_t)stream);
}

int tbx_reduce(tbx_engine* e, int query, const double* args, int n_args, int per_env, double* out_host)
{
    CHECK_ENGINE(e);
    const int width = tbx_reduce_width(e->game, query);
    if (width < 0) return e->fail(TBX_E_INVALID, "unknown query for this game");
    if (!out_host) return e->fail(TBX_E_INVALID, "output pointer is NULL");
    if ((query == TBX_QUERY_LOOKAHEAD_ACT || query == TBX_QUERY_LOOKAHEAD_TREE_ACT) && per_env) return e->fail(TBX_E_INVALID, "act takes shared arguments only");
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    TbxEditArgs a;
    int rc = edit_args(e, args, n_args, per_env, true, e->stream, a);
    if (rc) return rc;
    const size_t bytes = sizeof(double) * (size_t)e->n * (size_t)width;
    EHIP(e->reduce_out.reserve(bytes, e->stream));
    rc = engine_reduce(e, query, a, e->reduce_out.p, width, e->stream, args);      // (the host's rows: queries 157, 158 and 160 scan them)
    if (rc) return rc;
    EHIP(hipMemcpyAsync(out_host, e->reduce_out.p, bytes, hipMemcpyDeviceToHost, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int tbx_query(tbx_engine* e, int env, int query_id, const int32_t* args, int n_args, int32_t* out, int n_out)
{
    CHECK_ENGINE(e);
    if (env < 0 || env >= e->n || !args || !out) return e->fail(TBX_E_INVALID, "bad query arguments");
    if (e->game == TBX_GAME_AMIDAR && n_args >= 2 && n_out >= 2) {
        // pure functions of the arguments (world = tile * (64, 80)); floor division for negative world coordinates
        if (query_id == TBX_QUERY_TILE_TO_WORLD) { out[0] = args[0] * TBX_AMI_TILE_WX; out[1] = args[1] * TBX_AMI_TILE_WY; return TBX_OK; }
        if (query_id == TBX_QUERY_WORLD_TO_TILE) {
            out[0] = args[0] >= 0 ? args[0] / TBX_AMI_TILE_WX : -((-args[0] + TBX_AMI_TILE_WX - 1) / TBX_AMI_TILE_WX);
            out[1] = args[1] >= 0 ? args[1] / TBX_AMI_TILE_WY : -((-args[1] + TBX_AMI_TILE_WY - 1) / TBX_AMI_TILE_WY);
            return TBX_OK;
        }
    }
    return e->fail(TBX_E_INVALID, "unknown query for this game");
}

int tbx_device_buffer(tbx_engine* e, int which, void** out_ptr, size_t* out_bytes)
{
    CHECK_ENGINE(e);
    if (!out_ptr) return e->fail(TBX_E_INVALID, "out_ptr is NULL");
    const size_t N = (size_t)e->n;
    void* p = nullptr;
    size_t b = 0;
    if (e->pipe_active && ((which >= TBX_BUF_REWARD && which <= TBX_BUF_PACKED) || which == TBX_BUF_ROLLOUT_FRAMES || which == TBX_BUF_ROLLOUT_PACKED)) {
        const int rc = pipe_reader_joins(e, which == TBX_BUF_FRAME || which == TBX_BUF_ROLLOUT_FRAMES);   // (overlapped fused launches, rollout chunks: the caller's stream joins here)
        if (rc) return rc;
    }
    switch (which) {
    case TBX_BUF_ROLLOUT_FRAMES:
        if (!e->rollout.k) return e->fail(TBX_E_INVALID, "tbx_rollout_synthetic has not been called");
        p = e->rollout.frames[e->rollout.cur].p;
        b = (size_t)e->rollout.k * N * e->ops->height() * e->ops->width() * e->rollout.channels;
        break;
    case TBX_BUF_ROLLOUT_PACKED:
        if (!e->rollout.k) return e->fail(TBX_E_INVALID, "tbx_rollout_synthetic has not been called");
        p = e->rollout.packed_base;
        b = sizeof(uint64_t) * (size_t)e->rollout.k * e->rollout.packed_stride;
        break;
    case TBX_BUF_REWARD: p = e->reward; b = N * 4; break;
    case TBX_BUF_DONE: p = e->done; b = N; break;
    case TBX_BUF_LIVES: p = e->lives_out; b = N * 4; break;
    case TBX_BUF_SCORE: p = e->score_out; b = N * 4; break;
    case TBX_BUF_FRAME: p = e->frame; b = e->frame_bytes; break;
    case TBX_BUF_PACKED: p = e->packed; b = N * 8; break;
    case TBX_BUF_AGENT_OBS: case TBX_BUF_AGENT_REWARD: case TBX_BUF_AGENT_DONE:
    case TBX_BUF_AGENT_EP_DONE: case TBX_BUF_AGENT_EP_RETURN: case TBX_BUF_AGENT_EP_LENGTH: case TBX_BUF_AGENT_PLANE: case TBX_BUF_AGENT_RING:
        return tbx_agent_buffer(e, which, out_ptr, out_bytes);
    case TBX_BUF_GATHERED: return tbx_gather_buffer(e, out_ptr, out_bytes);
    case TBX_BUF_PLAN_ACTION: case TBX_BUF_PLAN_CARRY: {
        if (!e->plan_action || !e->plan_carry) return e->fail(TBX_E_INVALID, "TBX_QUERY_LOOKAHEAD_ACT has not been called");
        p = which == TBX_BUF_PLAN_ACTION ? (void*)e->plan_action : (void*)e->plan_carry;
        b = N * 4;
        break;
    }
    case TBX_BUF_PLAN_TREE:
        if (!e->plan_tree) return e->fail(TBX_E_INVALID, "TBX_QUERY_LOOKAHEAD_TREE_ACT has not been called");
        p = e->plan_tree;
        b = e->plan_tree_bytes;
        break;
    default: return e->fail(TBX_E_INVALID, "unknown buffer id");
    }
    *out_ptr = p;
    if (out_bytes) *out_bytes = b;
    return TBX_OK;
}

int tbx_set_option(tbx_engine* e, int option, int value)
{
    CHECK_ENGINE(e);
    if (option == TBX_OPT_BEAM_RANGE_ENVS) {       // read by the host when a beam query is cut into ranges: nothing in flight depends on it
        if (value < 0) return e->fail(TBX_E_INVALID, "option value out of range");
        e->beam_range_envs = value;
        return TBX_OK;
    }
    if (option == TBX_OPT_BEAM_SAMPLES_MAX_CHUNKS) {   // read by the host when a level's samples are cut: nothing in flight depends on it
        if (value < 0 || value > TBX_LOOKAHEAD_MAX_SAMPLES) return e->fail(TBX_E_INVALID, "option value out of range");
        e->beam_samples_max_chunks = value;
        return TBX_OK;
    }
    if (option == TBX_OPT_TREE_LAUNCH_SIMULATIONS) {   // read by the host when a tree's simulations are cut into launches: nothing in flight depends on it
        if (value < 0 || value > TBX_TREE_MAX_SIMULATIONS) return e->fail(TBX_E_INVALID, "option value out of range");
        e->tree_launch_simulations = value;
        return TBX_OK;
    }
    if (option == TBX_OPT_TREE_CARRY_KEEP || option == TBX_OPT_TREE_CARRY_MAX_VISITS) {   // read by the host when a tree act is queued: nothing in flight depends on them
        const bool keep = option == TBX_OPT_TREE_CARRY_KEEP;
        if (value < 0 || value > (keep ? TBX_TREE_MAX_SIMULATIONS + 1 : TBX_TREE_CARRY_MAX_VISITS)) return e->fail(TBX_E_INVALID, "option value out of range");
        (keep ? e->tree_carry_keep : e->tree_carry_max_visits) = value;
        return TBX_OK;
    }
    bool ok = false;
    switch (option) {
    case TBX_OPT_PIPELINE: ok = value >= 0 && value <= 3; break;
    case TBX_OPT_STEP_FORM: ok = value >= 0 && value <= 2; break;
    case TBX_OPT_RENDER_SPLIT: ok = value >= 0 && value <= 64; break;
    case TBX_OPT_AGENT_GENERIC: case TBX_OPT_RESIDENT_STEP: case TBX_OPT_GATHER_TRANSPORT: ok = value == 0 || value == 1; break;
    case TBX_OPT_GATHER_EVERY: ok = value >= 1 && value <= 64; break;
    case TBX_OPT_FUSED_OVERLAP: ok = value >= 0 && value <= 2; break;
    case TBX_OPT_FUSED_OVERLAP_LEAD: ok = value >= 0 && value <= (1 << 20); break;
    case TBX_OPT_ROLLOUT_CHUNKS: ok = value >= 0 && value <= 4; break;
    default: return e->fail(TBX_E_INVALID, "unknown option");
    }
    if (!ok) return e->fail(TBX_E_INVALID, "option value out of range");
    if (e->opt[option] == value) return TBX_OK;
    // a launch-time choice must not change under work that is in flight
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_use_stream(e, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    e->opt[option] = value;
    e->ops->options_changed(e);
    return TBX_OK;
}

int tbx_get_option(tbx_engine* e, int option, int* value_out)
{
    CHECK_ENGINE(e);
    if (value_out && option == TBX_OPT_PIPELINE_ACTIVE) { *value_out = pipe_mode(e); return TBX_OK; }
    if (value_out && option == TBX_OPT_RECORDS_ACTIVE) { *value_out = e->ops->pipeline_ok() ? 1 : 0; return TBX_OK; }
    if (value_out && option == TBX_OPT_RENDER_STEP_FUSED) { *value_out = e->ops->render_step_fused(3) ? 1 : 0; return TBX_OK; }
    if (value_out && option == TBX_OPT_FUSED_OVERLAP_ACTIVE) { *value_out = fused_overlap_on(e, nullptr, 3) ? 1 : 0; return TBX_OK; }
    if (value_out && option == TBX_OPT_ROLLOUT_CHUNKS_ACTIVE) { *value_out = rollout_chunks_on(e, 3) ? 1 : 0; return TBX_OK; }
    if (value_out && option == TBX_OPT_SEARCH_CHUNKS) { *value_out = e->search_chunks; return TBX_OK; }
    if (value_out && option == TBX_OPT_SAMPLE_CHUNKS) { *value_out = e->sample_chunks; return TBX_OK; }
    if (value_out && option == TBX_OPT_SEARCH_SAMPLES_CHUNKS) { *value_out = e->search_samples_chunks; return TBX_OK; }
    if (value_out && option == TBX_OPT_BEAM_RANGES) { *value_out = e->beam_ranges; return TBX_OK; }
    if (value_out && option == TBX_OPT_BEAM_RANGE_ENVS) { *value_out = e->beam_range_envs; return TBX_OK; }
    if (value_out && option == TBX_OPT_BEAM_SAMPLES_RANGES) { *value_out = e->beam_samples_ranges; return TBX_OK; }
    if (value_out && option == TBX_OPT_BEAM_SAMPLES_CHUNKS) { *value_out = e->beam_samples_chunks; return TBX_OK; }
    if (value_out && option == TBX_OPT_BEAM_SAMPLES_MAX_CHUNKS) { *value_out = e->beam_samples_max_chunks; return TBX_OK; }
    if (value_out && option == TBX_OPT_EVOLVE_RANGES) { *value_out = e->evolve_ranges; return TBX_OK; }
    if (value_out && option == TBX_OPT_TREE_RANGES) { *value_out = e->tree_ranges; return TBX_OK; }
    if (value_out && option == TBX_OPT_TREE_LAUNCH_SIMULATIONS) { *value_out = e->tree_launch_simulations; return TBX_OK; }
    if (value_out && option == TBX_OPT_TREE_CARRY_KEEP) { *value_out = e->tree_carry_keep; return TBX_OK; }
    if (value_out && option == TBX_OPT_TREE_CARRY_MAX_VISITS) { *value_out = e->tree_carry_max_visits; return TBX_OK; }
    if (value_out && option == TBX_OPT_SEARCH_SAMPLES_LAUNCHES) { *value_out = e->search_samples_launches; return TBX_OK; }
    if (option < 0 || option >= TBX_OPT_COUNT || !value_out) return e->fail(TBX_E_INVALID, "unknown option");
    *value_out = e->opt[option];
    return TBX_OK;
}

int tbx_sync(tbx_engine* e)
{
    CHECK_ENGINE(e);
    EHIP(hipSetDevice(e->device));
    EHIP(tbx_serve_stop(e));
    EHIP(tbx_finish_pending(e));
    EHIP(hipDeviceSynchronize());
    e->has_last = false;              // nothing is pending any more: the stream of the last call is no longer needed
    e->pipe_active = false;
    return check_err_flag(e);
}

}  // extern "C"
