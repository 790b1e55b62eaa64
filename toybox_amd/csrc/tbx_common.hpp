// tbx_common.hpp -- shared pieces of the gfx950 engine: RNG, action tables, wave helpers,
// the engine object and the per-game operations table.  gfx950 (CDNA4, wave64) only.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/toybox_amd.h"

#define TBX_WAVE 64
#define TBX_WAVES_PER_BLOCK 4
#define TBX_BLOCK (TBX_WAVE * TBX_WAVES_PER_BLOCK)

#define TBX_HIP(call)                                                                      \
    do {                                                                                   \
        hipError_t _e = (call);                                                            \
        if (_e != hipSuccess) {                                                            \
            return e->fail(TBX_E_NO_DEVICE, std::string(#call) + ": " + hipGetErrorString(_e)); \
        }                                                                                  \
    } while (0)

// ------------------------------------------------------------------ device helpers

// xoroshiro128+ (55,14,36); pinned by tests/golden/rng_kat.json
struct Rng {
    uint64_t s0, s1;
    __device__ __forceinline__ uint64_t next()
    {
        uint64_t r = s0 + s1;
        uint64_t t = s1 ^ s0;
        s0 = ((s0 << 55) | (s0 >> 9)) ^ t ^ (t << 14);
        s1 = (t << 36) | (t >> 28);
        return r;
    }
    __device__ __forceinline__ Rng child()
    {
        Rng c;
        c.s0 = next();
        c.s1 = next();
        return c;
    }
    // uniform in [0,n): widening multiply + rejection zone (rand's UniformInt::sample_single)
    __device__ __forceinline__ uint64_t range(uint64_t n)
    {
        if (n <= 1) return 0;
        uint64_t zone = (n << __clzll((long long)n)) - 1;
        for (;;) {
            uint64_t v = next();
            uint64_t lo = v * n;
            if (lo <= zone) return __umul64hi(v, n);
        }
    }
};

__host__ __device__ __forceinline__ void tbx_seed_state(uint32_t seed, uint64_t& s0, uint64_t& s1)
{
    s0 = 0x193a6754a8a7d469ULL ^ (uint64_t)seed;
    s1 = 0x97830e05113ba7bbULL;
}

__host__ __device__ __forceinline__ uint64_t tbx_splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// ALE action id -> button mask (envs/atari/constants.py:16-35); 0xFF = illegal id
__host__ __device__ __forceinline__ uint32_t tbx_ale_buttons(int a)
{
    // packed table, one byte per action
    const uint8_t L = TBX_BTN_LEFT, R = TBX_BTN_RIGHT, U = TBX_BTN_UP, D = TBX_BTN_DOWN, F = TBX_BTN_BUTTON1;
    switch (a) {
    case 0: return 0;
    case 1: return F;
    case 2: return U;
    case 3: return R;
    case 4: return L;
    case 5: return D;
    case 6: return U | R;
    case 7: return U | L;
    case 8: return D | R;
    case 9: return D | L;
    case 10: return U | F;
    case 11: return R | F;
    case 12: return L | F;
    case 13: return D | F;
    case 14: return U | R | F;
    case 15: return U | L | F;
    case 16: return D | R | F;
    case 17: return D | L | F;
    default: return 0xFFu;
    }
}

__host__ __device__ __forceinline__ int tbx_legal_count(int game)
{
    return game == TBX_GAME_BREAKOUT ? 4 : game == TBX_GAME_GRIDWORLD ? 5 : 6;
}
__host__ __device__ __forceinline__ int tbx_legal_action(int game, int i)
{
    // Breakout [0,1,3,4]; Amidar [0..5]; SpaceInvaders [0,1,3,4,11,12]; GridWorld [0,2,3,4,5]
    if (game == TBX_GAME_BREAKOUT) return i == 0 ? 0 : i == 1 ? 1 : i == 2 ? 3 : 4;
    if (game == TBX_GAME_GRIDWORLD) return i == 0 ? 0 : i + 1;
    if (game == TBX_GAME_AMIDAR) return i;
    return i == 0 ? 0 : i == 1 ? 1 : i == 2 ? 3 : i == 3 ? 4 : i == 4 ? 11 : 12;
}
// Plans (TBX_QUERY_LOOKAHEAD_PLAN / _SEARCH): the largest depth whose n_legal^depth codes fit 2^32 (TBX_PLAN_MAX_DEPTH), and
// n_legal^depth for a depth in that range
__host__ __device__ __forceinline__ int tbx_plan_max_depth(int game) { return TBX_PLAN_MAX_DEPTH(game); }
__host__ __device__ __forceinline__ uint64_t tbx_plan_count(int game, int depth)
{
    uint64_t c = 1;
    for (int i = 0; i < depth; i++) c *= (uint64_t)tbx_legal_count(game);
    return c;
}

// how the step kernels obtain their action
struct ActionSource {
    const int32_t* actions;   // device array, or nullptr for synthetic
    uint64_t seed, t, env_offset;
    int single_env;           // >= 0: only this env steps, with buttons `single_buttons`
    uint32_t single_buttons;
    // agent layer (MaxAndSkipEnv.step, atari_wrappers.py:201-216): sum the rewards of the agent step's frames into
    // acc_reward[env] and latch acc_done[env]; an env whose game has ended does not run the remaining frames
    int32_t* acc_reward;
    uint8_t* acc_done;
    // one launch runs `frames` frames of the same action with the state held in registers (0 means 1; games with
    // GameOps::multi_frame_step run the whole action repeat in ONE launch); frame0 = frames of this agent step that earlier
    // launches already ran
    int frames;
    int frame0;
    // MaxAndSkipEnv._obs_buffer, kept as two persistent state snapshots per env ("slot A" / "slot B", what the rasteriser
    // needs to repaint the frame): written after snap_a_after / snap_b_after frames of the agent step (0 = never), i.e. by
    // frame skip-2 and frame skip-1, and only by envs that get that far.  buf_valid[env] bit 0 / 1: the slot has been written
    // since construction (until then it is the zero frame of np.zeros).
    int snap_a_after, snap_b_after;
    uint8_t* buf_valid;
    // single-frame launches (games without multi_frame_step): 1 if the env ran this frame, for the snapshot kernel that follows
    uint8_t* exec_flag;
};

// this env's game ended in an earlier launch of the same agent step: MaxAndSkipEnv has left its loop
__device__ __forceinline__ bool tbx_agent_env_finished(const ActionSource& src, int env)
{
    return src.acc_done && src.frame0 > 0 && src.acc_done[env] != 0;
}

// frame: index of this frame inside the launch
__device__ __forceinline__ void tbx_accumulate(const ActionSource& src, int env, int32_t rew, bool is_done, int frame = 0)
{
    if (!src.acc_reward) return;
    const bool first = src.frame0 + frame == 0;
    src.acc_reward[env] = (first ? 0 : src.acc_reward[env]) + rew;
    src.acc_done[env] = is_done ? 1 : 0;
}

// which buffer slots frame number `done_frames` (1-based count of frames run in this agent step) writes: bit 0 = A, bit 1 = B
__device__ __forceinline__ uint32_t tbx_snap_slots(const ActionSource& src, int frame)
{
    const int g = src.frame0 + frame + 1;
    return (g == src.snap_a_after ? 1u : 0u) | (g == src.snap_b_after ? 2u : 0u);
}

__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t wave_uniform64(uint64_t v)
{
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) | ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
}

// value of lane `src` for a WAVE-UNIFORM src: v_readlane_b32 (a few cycles, result in an SGPR) instead of ds_bpermute_b32
__device__ __forceinline__ int bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ uint32_t bcast(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }

__device__ __forceinline__ uint32_t gray_of(uint32_t rgba)
{
    uint32_t r = rgba & 255u, g = (rgba >> 8) & 255u, b = (rgba >> 16) & 255u;
    return (77u * r + 150u * g + 29u * b + 128u) >> 8;
}

__host__ __device__ __forceinline__ uint32_t pack_color(tbx_color_t c)
{
    return (uint32_t)c.r | ((uint32_t)c.g << 8) | ((uint32_t)c.b << 16) | ((uint32_t)c.a << 24);
}
__host__ __device__ __forceinline__ tbx_color_t unpack_color(uint32_t v)
{
    tbx_color_t c;
    c.r = (uint8_t)v; c.g = (uint8_t)(v >> 8); c.b = (uint8_t)(v >> 16); c.a = (uint8_t)(v >> 24);
    return c;
}

// double -> pixel coordinate: clamp, then truncate toward zero (matches the oracle's f2i)
__device__ __forceinline__ int f2i(double v)
{
    if (!(v > -1.0e6)) v = -1.0e6;
    if (v > 1.0e6) v = 1.0e6;
    return (int)v;
}

// ------------------------------------------------------------------ resident single-env step ("server" kernel)
//
// The reference's whole user-facing surface is single-env: Toybox.apply_ale_action + get_score / get_lives / game_over, one FFI
// round trip per frame (test/benchmark.py:50-56).  On a GPU that loop is pure latency: a launch, a host-device copy each
// way and a stream synchronisation are ~30 us.  For a one-env engine tbx_step1 therefore talks to a RESIDENT kernel
// instead: one wave that waits on a mailbox in host-coherent pinned memory, runs the game's ordinary step body for env 0
// and posts the outputs back -- two PCIe hops per frame, no launch, no copy, no synchronisation.  The wave leaves by
// itself after TBX_SERVE_IDLE_TICKS without a request (or when told to), and every other entry point of the handle stops
// it first, so nothing else ever runs beside it on the env's state.
struct TbxServeCtl {
    // host -> device: ONE 64-bit word, so that a single PCIe read per poll brings the whole request:
    //   bits 0..31 request number, 32..47 ALE action id (int16), 48..51 TBX_STEP_* flags, 52..53 frame wanted (0 none, 1 gray,
    //   2 RGB, 3 RGBA: the wave rasterises the env into `frame_dev` after the step), 63 "leave now"
    uint64_t req;
    uint64_t frame_dev;      // device address of the engine's mapped pinned frame buffer (written once before the launch)
    uint64_t _pad0[6];
    // device -> host (its own cache line): outputs, then the request number they belong to (written last)
    int32_t reward, lives, score;
    uint32_t done_err;       // bit 0 done, bit 1 illegal action id, bit 2 the frame was asked for but this kernel cannot paint it
    uint32_t ack_seq;
    uint32_t exited;
    uint32_t _pad1[10];
};
constexpr uint32_t TBX_SERVE_FRAME_SHIFT = 4;   // within the 8 flag bits of the request word
constexpr unsigned long long TBX_SERVE_IDLE_TICKS = 5000000ull;   // 50 ms of the 100 MHz s_memrealtime clock
constexpr uint64_t TBX_SERVE_STOP = 1ull << 63;

__host__ __device__ __forceinline__ uint64_t tbx_serve_word(uint32_t seq, int action, uint32_t flags)
{
    // ids outside int16 are all illegal anyway: clamp them onto one illegal id
    const int a = action < -32768 || action > 32767 ? 32767 : action;
    return (uint64_t)seq | ((uint64_t)(uint16_t)(int16_t)a << 32) | ((uint64_t)(flags & 0xFFu) << 48);
}

// The resident kernel is ONE block of TBX_SERVE_WAVES waves.  Wave 0 waits for requests and steps: step(src, flags) runs one
// frame of env 0 on it (every lane of wave 0 calls it; outputs land in out_* [0]).  When the request wants the picture, ALL
// waves paint: render(channels, frame, part, split) rasterises units part, part + split, ... of env 0 into `frame` (host
// memory, mapped) and returns false if this game's kernel cannot -- a lone wave needs ~45 us for a frame (one dependent
// instruction stream), eight need ~8.  The other waves sleep at the block barrier in between and take no issue slots.
constexpr int TBX_SERVE_WAVES = 8;

template <class StepFn, class RenderFn>
__device__ __forceinline__ void tbx_serve_loop(TbxServeCtl* ctl, int lane, StepFn step, RenderFn render, const int32_t* out_reward, const uint8_t* out_done,
                                               const int32_t* out_lives, const int32_t* out_score, uint32_t* err_flag)
{
    __shared__ uint32_t cmd[2];              // [0]: 0 = nothing to paint, 1 / 3 / 4 = paint that many channels, ~0u = leave; [1]: "cannot paint"
    const int wave = wave_uniform((int)(threadIdx.x >> 6));
    uint32_t last = __hip_atomic_load(&ctl->ack_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    uint8_t* const frame = reinterpret_cast<uint8_t*>(__hip_atomic_load(&ctl->frame_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
    for (;;) {
        uint32_t seq = last, err = 0;
        if (wave == 0) {
            bool leave = false;
            uint32_t hi = 0;
            for (;;) {
                uint64_t w = last;
                bool idle_out = false;
                if (lane == 0) {
                    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
                    unsigned polls = 0;
                    for (;;) {
                        w = __hip_atomic_load(&ctl->req, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
                        if ((uint32_t)w != last || (w & TBX_SERVE_STOP)) break;
                        if ((++polls & 63u) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > TBX_SERVE_IDLE_TICKS) { idle_out = true; break; }
                    }
                }
                seq = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w);
                hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w >> 32));
                idle_out = __builtin_amdgcn_readfirstlane((int)idle_out) != 0;
                if (seq != last) break;                          // a request (one that raced with the stop bit is served first)
                if ((hi >> 31) || idle_out) { leave = true; break; }   // told to leave, or idle for too long
            }
            if (leave) {
                if (lane == 0) cmd[0] = ~0u;
            } else {
                const int action = (int)(int16_t)(hi & 0xFFFFu);
                const uint32_t flags = (hi >> 16) & 0xFFu;
                ActionSource src{};
                uint32_t buttons = tbx_ale_buttons(action);
                if (buttons == 0xFFu) { buttons = 0; err = 2; }  // illegal id: NOOP + TBX_E_ACTION, as in the batch kernels
                src.single_env = 0;
                src.single_buttons = buttons;
                step(src, flags & 0x0Fu);
                const uint32_t want = (flags >> TBX_SERVE_FRAME_SHIFT) & 3u;
                if (want) __threadfence();                       // what the step stored, for the waves that paint
                if (lane == 0) { cmd[0] = want == 0 ? 0u : want == 1 ? 1u : want == 2 ? 3u : 4u; cmd[1] = 0u; }
            }
        }
        __syncthreads();
        const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)cmd[0]);
        if (c == ~0u) {
            if (wave == 0 && lane == 0) __hip_atomic_store(&ctl->exited, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        if (c) {
            if (!render((int)c, frame, wave, TBX_SERVE_WAVES) && lane == 0) cmd[1] = 1u;
            __threadfence_system();                              // this wave's part of the frame is in host memory ...
        }
        __syncthreads();                                         // ... and so is everybody's, before the acknowledgement
        if (wave == 0) {
            if (c && __builtin_amdgcn_readfirstlane((int)cmd[1])) err |= 4u;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            if (lane == 0) {
                ctl->reward = out_reward[0]; ctl->lives = out_lives[0]; ctl->score = out_score[0];
                ctl->done_err = (out_done[0] ? 1u : 0u) | err;
                __hip_atomic_store(&ctl->ack_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            last = seq;
        }
        __syncthreads();                                         // cmd[] may be rewritten
    }
}

// ------------------------------------------------------------------ host side

// a run-time value as a template argument: f(std::integral_constant<int, V>{}) for the V that equals v; false when none does
template <int... Vs, class F>
bool tbx_dispatch(int v, F&& f)
{
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
// the stack depth an observation kernel is built for: 0 the plane ring (new_plane = 2), any depth; 1 .. 3; anything else runs as 4
inline int tbx_stack_arm(bool obs, int stack) { return !obs ? 0 : stack >= 0 && stack <= 3 ? stack : 4; }

struct GameOps;

// the outputs of a batch step (TBX_BUF_REWARD / DONE / LIVES / SCORE / PACKED); two sets exist once the pipelined mode is on
struct TbxStepOut {
    int32_t* reward = nullptr;
    uint8_t* done = nullptr;
    int32_t* lives = nullptr;
    int32_t* score = nullptr;
    uint64_t* packed = nullptr;
};

// A device buffer that only grows.  reserve(): nothing while it is large enough; else the streams that may still use the old
// buffer run dry first (a null stream: none), it is freed and a new one made.  After a failed hipMalloc the buffer is empty, so
// a repeated call tries again.
template <class T>
struct TbxDevBuf {
    T* p = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t need, hipStream_t drain_a = nullptr, hipStream_t drain_b = nullptr)
    {
        if (bytes >= need) return hipSuccess;
        hipError_t r = drain_a ? hipStreamSynchronize(drain_a) : hipSuccess;
        if (r == hipSuccess && drain_b) r = hipStreamSynchronize(drain_b);
        if (r == hipSuccess && p) r = hipFree(p);
        if (r != hipSuccess) return r;
        p = nullptr;
        bytes = 0;
        r = hipMalloc((void**)&p, need);
        if (r == hipSuccess) bytes = need;
        else p = nullptr;
        return r;
    }
    void release()
    {
        hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// what TBX_BUF_ROLLOUT_FRAMES / TBX_BUF_ROLLOUT_PACKED name: the last chunk of tbx_rollout_synthetic, whichever form ran it
struct TbxRolloutResult {
    TbxDevBuf<uint8_t> frames[2];                    // [k][N][H][W][C] frames of the last chunk of parity q
    TbxDevBuf<uint64_t> packed[2];                   // [k][N] step records of that chunk when no gather ring takes them
    int cur = 0, k = 0, channels = 0;                // parity, frames and channels of the last chunk
    uint64_t* packed_base = nullptr;                 // ... and where its step records lie (a ring of the gather, or `packed`)
    size_t packed_stride = 0;
};

// what an overlapped fused launch gets from the engine: the counter its step blocks bump, the event that rides on the launch as
// its completion event; step_blocks comes back (how many arrivals the launch adds)
// measurement builds only (make DIAG=1; env TBX_OVERLAP_DIAG read in pipeline.hip; results are WRONG or racy with any bit set): parts of
// the overlapped launch switched off one at a time -- 1 the first build's step half: plain loads and stores behind a per-wave L2
// invalidate and write-back (+ 2: no write-back) instead of agent-scope loads and stores, 4 plain record load, 8 both launches on ONE lane (the machinery without any overlap), 16 no fence / wait on the caller's
// stream, 32 one frame buffer, 64 no wait kernel, 128 no completion event on the launch
#ifdef TBX_DIAG
#define OVL_DIAG(mask, bit) (((mask) & (bit)) != 0)
#else
#define OVL_DIAG(mask, bit) false
#endif

struct TbxOverlapLaunch {
    unsigned long long* arrive;     // [0] bumped by every step block when its stores are out, [1] by the release block when it starts
    hipEvent_t done;
    int lead;                       // TBX_OPT_FUSED_OVERLAP_LEAD (0: the engine's choice)
    int step_blocks;
    int diag;                       // OVL_DIAG mask (0 in product builds)
};

struct tbx_engine {
    int game = -1, n = 0, device = 0;
    mutable std::string err;
    hipStream_t stream = nullptr;   // engine-owned stream used by the host-pointer entry points
    // cross-stream ordering of everything queued through this handle (tbx_use_stream): the stream the last call used.  It may
    // be the caller's, which therefore has to outlive the next call on the handle (tbx_sync forgets it).
    hipStream_t last_stream = nullptr;
    bool has_last = false;
    hipEvent_t order_ev = nullptr;
    bool step_carries_order_ev = false;        // order_ev is the completion event of the last launch on last_stream (a batch step)
    int opt[TBX_OPT_COUNT] = {0, 0, 0, 0, 1, 1, 0, 0, 0, 0};
    bool gather_ring = false;                  // a K-step record ring is in force (TBX_OPT_GATHER_EVERY > 1 at tbx_gather_init): no pipelined mode
    int gather_ring_every = 0, gather_ring_width = 0;   // ... its K and its row width in records (tbx_rollout_synthetic)
    bool gather_wants_step_event = false;      // the next batch step is one a collective will wait for: its launch carries the ordering event
    struct TbxPipe* pipe = nullptr;            // pipelined mode and the overlapped loop forms (pipeline.hip), created by the first such call
    bool pipe_active = false;                  // the last call through the handle was one of them
    TbxRolloutResult rollout;
    // common device buffers (SoA over envs)
    uint64_t* sim_rng = nullptr;    // [2][N] simulator RNG
    int32_t* prev_score = nullptr;  // [N]
    TbxStepOut outs[2];             // [1] is allocated when the pipelined mode is switched on
    int out_par = 0;
    int32_t* reward = nullptr;      // [N]   == outs[out_par].* : the outputs of the most recently issued step
    uint8_t* done = nullptr;        // [N]
    int32_t* lives_out = nullptr;   // [N]
    int32_t* score_out = nullptr;   // [N]
    uint64_t* packed = nullptr;     // [N]
    int32_t* actions = nullptr;     // [N] staging for host actions
    uint8_t* mask = nullptr;        // [N] staging for new_game masks
    uint32_t* err_flag = nullptr;   // device word: bit0 = illegal action seen
    int32_t* scal = nullptr;        // [3][N] scratch of tbx_get_scalars
    int32_t* scal_host = nullptr;   // pinned mirror of it
    uint8_t* one_frame = nullptr;   // H*W*4 scratch of tbx_render_env
    // host-pointer step path: one device block [reward | lives | score | err | done] gathered by a kernel and ONE copy
    // into pinned host memory (five pageable copies cost ~100 us per call); actions go up through the pinned block too
    int32_t* io_dev = nullptr;      // 3N + 1 dwords + N bytes
    int32_t* io_host = nullptr;     // pinned mirror (+ N action dwords in front)
    bool host_pending = false;      // a tbx_step_begin whose outputs are on their way (tbx_step_end takes them)
    // "Any other call on the handle between _begin and _end ends the step first" (toybox_amd.h): which kind of step is pending
    // (0 none, 1 tbx_step_begin, 2 tbx_agent_step_begin), and -- once another entry point has ended it through
    // tbx_finish_pending -- the result its own "_end" call still has to report
    int pending_kind = 0;
    int ended_early_kind = 0;
    int ended_early_rc = 0;
    std::string ended_early_msg;
    tbx_step_host_out_t host_out{}; // where they go
    TbxDevBuf<uint8_t> frame_own;   // engine-owned frame buffer (lazy)
    uint8_t* frame = nullptr;       // what TBX_BUF_FRAME reports: frame_own, in the overlapped forms the buffer the last launch wrote,
                                    // after tbx_rollout_synthetic the last frame of the chunk's frames (include/toybox_amd.h)
    size_t frame_bytes = 0;         // ... and the size of that frame, N * H * W * channels of the call that produced it
    TbxDevBuf<double> edit_args;    // [N][n_args] per-env arguments of tbx_edit / tbx_reduce (host-pointer forms)
    TbxDevBuf<double> reduce_out;   // [N][width] result staging of tbx_reduce
    TbxDevBuf<double> search_parts; // [N][n_legal][chunks][6] partial rows of TBX_QUERY_LOOKAHEAD_SEARCH cut into chunks
    int search_chunks = 0;          // chunks of the last TBX_QUERY_LOOKAHEAD_SEARCH (0: none yet)
    TbxDevBuf<double> sample_parts; // [N][n_legal][chunks][8] partial rows of TBX_QUERY_LOOKAHEAD_SAMPLES cut into chunks (64-bit integers)
    int sample_chunks = 0;          // chunks of the last TBX_QUERY_LOOKAHEAD_SAMPLES (0: none yet)
    TbxDevBuf<double> search_samples_parts;  // [N][n_legal][chunks][9] partial rows of TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES (64-bit integers)
    int search_samples_chunks = 0, search_samples_launches = 0;   // chunks and launches of the last TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES (0: none yet)
    TbxDevBuf<uint8_t> beam_scratch;   // candidates and two beams of one env range of TBX_QUERY_LOOKAHEAD_BEAM (at most TBX_BEAM_SCRATCH_BYTES; twice that once query 161 has run)
    int beam_ranges = 0;               // env ranges of the last TBX_QUERY_LOOKAHEAD_BEAM (0: none yet)
    int beam_range_envs = 0;           // TBX_OPT_BEAM_RANGE_ENVS (0: the engine's choice)
    int beam_samples_ranges = 0, beam_samples_chunks = 0;   // env ranges, and the most sample chunks of a level, of the last TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES (0: none yet)
    int beam_samples_max_chunks = 0;   // TBX_OPT_BEAM_SAMPLES_MAX_CHUNKS (0: the engine's choice)
    int evolve_ranges = 0;             // env ranges of the last TBX_QUERY_LOOKAHEAD_EVOLVE (0: none yet); its scratch is beam_scratch
    int tree_ranges = 0;               // env ranges of the last TBX_QUERY_LOOKAHEAD_TREE (0: none yet); its scratch is beam_scratch
    int tree_launch_simulations = 0;   // TBX_OPT_TREE_LAUNCH_SIMULATIONS (0: the engine's choice)
    // TBX_QUERY_LOOKAHEAD_TREE_ACT: engine state, not env state -- made by the first accepted call (lookahead_tree_act, engine.hip)
    uint8_t* plan_tree = nullptr;      // TBX_BUF_PLAN_TREE: [N][n_legal] unit blocks of TbxTreeScratch::unit_bytes(stride_for(plan_tree_key[4]))
    size_t plan_tree_bytes = 0;
    uint8_t* plan_tree_drop = nullptr; // [N] drop flags (TBX_EDIT_TREE_DROP)
    int plan_tree_key[5] = {0, 0, 0, 0, 0};   // frames, hold, depth, objective, simulations of the call that wrote the store (simulations 0: no live content)
    int tree_carry_keep = 0, tree_carry_max_visits = 0;   // TBX_OPT_TREE_CARRY_KEEP, TBX_OPT_TREE_CARRY_MAX_VISITS (0: the defaults)
    // TBX_QUERY_LOOKAHEAD_ACT: not env state -- made and zeroed on first use (act_alloc, engine.hip), never forked or checkpointed
    int32_t* plan_action = nullptr;    // [N] TBX_BUF_PLAN_ACTION: the ALE action of every env's winner
    uint32_t* plan_carry = nullptr;    // [N] TBX_BUF_PLAN_CARRY: the winner's code shifted by one period
    TbxDevBuf<double> act_scratch;     // [N][n_legal][9] the planner's rows, then [N][15] per-env evolve rows (init from the carry)
    TbxDevBuf<void> staging;        // device POD staging for get/set state
    struct TbxEnvCopy* envcopy = nullptr;   // TBX_EDIT_COPY_ENV / TBX_EDIT_CHECKPOINT_*: the fork's scratch copy, the checkpoint store (envcopy.hip), made on first use
    GameOps* ops = nullptr;
    struct AgentState* agent = nullptr;   // fused agent-side preprocessing (agent.hip), lazily created
    struct GatherState* gather = nullptr; // multi-GPU record gather over RCCL (gather.hip), created by tbx_gather_init
    // resident single-env step kernel (tbx_step1 on one-env engines)
    TbxServeCtl* serve_ctl = nullptr;     // host-coherent pinned mailbox (host address)
    TbxServeCtl* serve_ctl_dev = nullptr; // its device address
    uint8_t* serve_frame = nullptr;       // mapped pinned frame buffer the resident kernel rasterises into (H * W * 4 bytes, host address)
    uint8_t* serve_frame_dev = nullptr;   // its device address
    hipStream_t serve_stream = nullptr;
    bool serve_running = false;           // a server kernel has been launched and not yet been seen to exit
    uint32_t serve_seq = 0;

    int fail(int code, const std::string& msg) const
    {
        err = msg;
        return code;
    }
};

hipError_t tbx_serve_stop(tbx_engine* e);   // engine.hip
hipError_t tbx_finish_pending(tbx_engine* e);   // engine.hip: ends a step that is between "_begin" and "_end" (outputs delivered, result kept)
int tbx_agent_deliver(tbx_engine* e);       // agent.hip: the waiting half of tbx_agent_step_end
void tbx_agent_copy_envs(tbx_engine* e, struct TbxEnvPlan& plan);   // agent.hip: the wrapper stack's per-env arrays of TBX_EDIT_COPY_ENV / TBX_EDIT_CHECKPOINT_*

// Stream `s` waits for everything queued so far on the stream the previous call used.  That stream may be the caller's: the
// handle is kept until the next call or tbx_sync (toybox_amd.h: a stream named in a call must stay alive that long -- the
// runtime does not survive an event record on a destroyed stream, so a stale handle cannot be detected here).
// after_step_only: the caller (the gather) needs nothing but the last batch step; when that step's launch carried the ordering
// event as its completion event (TBX_LAUNCH_STEP below) no event has to be recorded behind it.
inline hipError_t tbx_wait_tail(tbx_engine* e, hipStream_t s, bool after_step_only = false)
{
    if (!e->has_last || e->last_stream == s) return hipSuccess;
    if (!e->order_ev) {
        hipError_t r = hipEventCreateWithFlags(&e->order_ev, hipEventDisableTiming);
        if (r != hipSuccess) return r;
    }
    if (!(after_step_only && e->step_carries_order_ev)) {
        hipError_t r = hipEventRecord(e->order_ev, e->last_stream);
        if (r != hipSuccess) return r;
    }
    return hipStreamWaitEvent(s, e->order_ev, 0);
}

// The launch of a whole-batch step kernel.  With a per-step gather initialised the ordering event rides on the launch as its
// completion event (hipExtLaunchKernelGGL's stopEvent) instead of being recorded behind it: measured on this runtime
// (scripts/ubench/evgap.hip), an event record between two kernels of a stream that another stream waits for delays the second
// kernel by 5.7 us, the completion-event form by 2.4 (two kernels with nothing between them: 1.0).
inline hipEvent_t tbx_step_order_event(tbx_engine* e)
{
    if (!e->gather || !e->gather_wants_step_event) return nullptr;    // (ring mode: only the step that completes the ring)
    if (!e->order_ev && hipEventCreateWithFlags(&e->order_ev, hipEventDisableTiming) != hipSuccess) return nullptr;
    return e->order_ev;
}
#define TBX_LAUNCH_STEP(e, s, KERNEL, GRID, BLOCK, ...)                                                             \
    do {                                                                                                            \
        hipEvent_t tail_ev_ = tbx_step_order_event(e);                                                              \
        if (tail_ev_) {                                                                                             \
            hipExtLaunchKernelGGL(KERNEL, GRID, BLOCK, 0, s, nullptr, tail_ev_, 0, __VA_ARGS__);                    \
            (e)->step_carries_order_ev = true;                                                                      \
        } else                                                                                                      \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCK, 0, s, __VA_ARGS__);                                             \
    } while (0)

hipError_t tbx_packed_leaves_chunk(tbx_engine* e, hipStream_t s);   // engine.hip: TBX_BUF_PACKED out of a chunk's record array
hipError_t pipe_leave(tbx_engine* e, hipStream_t s);                // pipeline.hip: the joins that leave a pipelined form

// Every entry point that queues work names the stream it is about to use.  When that differs from the stream the previous
// entry point used (the "_device" forms run on the caller's stream -- including the NULL stream, which does not order itself
// against the engine's non-blocking stream -- the host-pointer forms on the engine's own), the new stream first waits for an
// event recorded on the old one, so calls on one handle take effect in program order whatever streams they name.  (Pipelined
// calls make the caller's stream wait for their internal work and leave it as `last_stream`, so this also joins the pipeline.)
inline hipError_t tbx_use_stream(tbx_engine* e, hipStream_t s)
{
    if (e->pending_kind) {                     // a step between "_begin" and "_end": this call ends it first
        hipError_t r = tbx_finish_pending(e);
        if (r != hipSuccess) return r;
    }
    if (e->serve_running) {                    // nothing else runs beside the resident step kernel
        hipError_t r = tbx_serve_stop(e);
        if (r != hipSuccess) return r;
    }
    hipError_t r = tbx_wait_tail(e, s);
    if (r != hipSuccess) return r;
    if (e->pipe_active) {
        r = pipe_leave(e, s);
        if (r != hipSuccess) return r;
    }
    // after a rollout chunk without a record ring TBX_BUF_PACKED names the LAST ROW of the chunk's records: a step of any other
    // form would write its records there, so the row moves into the engine's own array first (behind the joins above)
    if (!e->gather_ring && e->packed != e->outs[e->out_par].packed) {
        r = tbx_packed_leaves_chunk(e, s);
        if (r != hipSuccess) return r;
    }
    e->step_carries_order_ev = false;          // whatever this call queues moves the tail
    e->pipe_active = false;
    e->last_stream = s;
    e->has_last = true;
    return hipSuccess;
}

// arguments of a batched intervention (tbx_edit / tbx_reduce): the same row for every env, or one row per env in HBM
struct TbxEditArgs {
    double v[TBX_EDIT_MAX_ARGS];
    int n;
    const double* per_env;        // device [N][n] or nullptr
    __device__ __forceinline__ double get(int env, int i) const { return i >= n ? 0.0 : per_env ? per_env[(size_t)env * n + i] : v[i]; }
    // an unsigned 32-bit argument (masks, seeds, counters: integers below 2^32 are exact in binary64)
    __device__ __forceinline__ uint32_t getu(int env, int i) const
    {
        const double x = get(env, i);
        return x >= 4294967295.0 ? 0xFFFFFFFFu : x > 0.0 ? (uint32_t)x : 0u;
    }
    // an integer argument: clamped to +-2e9, NaN reads -2e9 (the host forms check their rows with the same rule)
    __host__ __device__ __forceinline__ static int to_int(double x)
    {
        if (!(x > -2.0e9)) x = -2.0e9;
        if (x > 2.0e9) x = 2.0e9;
        return (int)x;
    }
    __device__ __forceinline__ int geti(int env, int i) const { return to_int(get(env, i)); }
};

// TBX_QUERY_LOOKAHEAD / _ALL (include/toybox_amd.h): the schedule of one (env, candidate) pair and the loop every game's
// leaf policy runs around its own step body.  The state lives in the caller's registers between one load and NO store.
// The five fields of one played schedule, as TbxLookahead::run_fields leaves them in registers.
struct TbxLookFields {
    long long ret;
    int score, lives, frames_run, lost_at;
};
// PLAN (TBX_QUERY_LOOKAHEAD_PLAN / _SEARCH): the action of period p < depth is digit p of `code` in base n_legal instead of
// `first`; the branch exists in that instantiation only (depth and code are dead members in the other), so tbx_lookahead_kernel
// pays nothing for it (profiles/lookahead.md).
template <int GAME, bool PLAN = false>
struct TbxLookahead {
    int frames, hold, first, rest;
    uint64_t key;                 // seed ^ ((env_offset + env) << 32)
    uint64_t t;
    int depth = 0;                // PLAN: periods that play a digit of the code
    uint32_t code = 0;            // PLAN: sum of digit_p * n_legal^p, below n_legal^depth <= 2^32 (a full 4^16 tree: codes 0 .. 2^32-1)
    static __device__ __forceinline__ bool playable(int a)
    {
        if (a == -1) return true;
        bool ok = false;
#pragma unroll
        for (int i = 0; i < tbx_legal_count(GAME); i++) ok = ok || a == tbx_legal_action(GAME, i);
        return ok;
    }
    // cand >= 0: candidate `cand` of TBX_QUERY_LOOKAHEAD_ALL (its first action is legal[cand]); false: this env's row is refused
    __device__ __forceinline__ bool read(const TbxEditArgs& a, int env, int cand)
    {
        frames = a.geti(env, 0);
        hold = a.n > 1 ? a.geti(env, 1) : 1;
        first = cand >= 0 ? tbx_legal_action(GAME, cand) : a.n > 2 ? a.geti(env, 2) : -1;
        rest = a.n > 3 ? a.geti(env, 3) : -1;
        const uint64_t seed = (uint64_t)a.getu(env, 4) | ((uint64_t)a.getu(env, 5) << 32);
        t = a.getu(env, 6);
        key = seed ^ (((uint64_t)a.getu(env, 7) + (uint64_t)env) << 32);
        return frames >= 1 && frames <= TBX_LOOKAHEAD_MAX_FRAMES && hold >= 1 && playable(first) && playable(rest);
    }
    // wave-per-env callers: every lane read the same row -- say so, and the frame loop's control runs on the scalar unit
    __device__ __forceinline__ void uniform()
    {
        frames = wave_uniform(frames); hold = wave_uniform(hold); first = wave_uniform(first); rest = wave_uniform(rest);
        key = wave_uniform64(key); t = wave_uniform64(t);
    }
    // PLAN, {frames, hold, depth, code | objective, rest, seed_lo, seed_hi, t, env_offset}: everything but column 3, which the
    // caller reads (the plan query its code, the search its objective and then every code of its chunk in turn)
    __device__ __forceinline__ bool read_plan(const TbxEditArgs& a, int env, int depth_default)
    {
        frames = a.geti(env, 0);
        hold = a.n > 1 ? a.geti(env, 1) : 1;
        depth = a.n > 2 ? a.geti(env, 2) : depth_default;
        first = -1;
        rest = a.n > 4 ? a.geti(env, 4) : -1;
        const uint64_t seed = (uint64_t)a.getu(env, 5) | ((uint64_t)a.getu(env, 6) << 32);
        t = a.getu(env, 7);
        key = seed ^ (((uint64_t)a.getu(env, 8) + (uint64_t)env) << 32);
        return frames >= 1 && frames <= TBX_LOOKAHEAD_MAX_FRAMES && hold >= 1 && depth >= 0 && depth <= tbx_plan_max_depth(GAME) && playable(rest);
    }
    __device__ __forceinline__ void uniform_plan()
    {
        uniform();
        depth = wave_uniform(depth); code = (uint32_t)wave_uniform((int)code);
    }
    // SAMPLES, {frames, hold, samples, salt, rest, seed_lo, seed_hi, t, env_offset}: a plan of depth 1 whose code is the candidate.
    // The caller reads columns 2 and 3 and sets the key of every future (seed: as the row has it, env_key: the env's part of a key).
    __device__ __forceinline__ bool read_samples(const TbxEditArgs& a, int env, int cand, uint64_t& seed, uint64_t& env_key)
    {
        frames = a.geti(env, 0);
        hold = a.n > 1 ? a.geti(env, 1) : 1;
        depth = 1;
        code = (uint32_t)cand;
        first = -1;
        rest = a.n > 4 ? a.geti(env, 4) : -1;
        seed = (uint64_t)a.getu(env, 5) | ((uint64_t)a.getu(env, 6) << 32);
        t = a.getu(env, 7);
        env_key = ((uint64_t)a.getu(env, 8) + (uint64_t)env) << 32;
        key = seed ^ env_key;
        return frames >= 1 && frames <= TBX_LOOKAHEAD_MAX_FRAMES && hold >= 1 && playable(rest);
    }
    __device__ __forceinline__ uint32_t buttons(int period) const
    {
        int a = period == 0 ? first : rest;
        if constexpr (PLAN) {
            a = rest;
            if (period < depth) {                       // once per period: `period` divisions by a constant
                uint32_t c = code;
                for (int i = 0; i < period; i++) c /= (uint32_t)tbx_legal_count(GAME);
                a = tbx_legal_action(GAME, (int)(c % (uint32_t)tbx_legal_count(GAME)));
            }
        }
        if (a < 0) a = tbx_legal_action(GAME, (int)(tbx_splitmix64(key ^ (t + (uint64_t)period)) % (uint64_t)tbx_legal_count(GAME)));
        return tbx_ale_buttons(a);
    }
    // step(buttons) runs one frame; score() / lives() read the state.  The five fields stay in registers: the caller stores them
    // (tbx_lookahead_store) or compares leaf after leaf and stores once.  Wave-per-env callers hand in wave-uniform score() /
    // lives(), so the exit at game over is wave-uniform; in thread-per-env callers it masks the finished lanes.
    template <class Step, class Score, class Lives>
    __device__ __forceinline__ TbxLookFields run_fields(Step&& step, Score&& score, Lives&& lives) const
    {
        int prev = score();
        const int lives0 = lives();
        long long ret = 0;
        int run_frames = 0, lost_at = -1, period = 0, left = hold, lv = lives0;
        uint32_t b = buttons(0);
#pragma clang loop unroll(disable)
        for (int j = 0; j < frames; j++) {
            if (left == 0) { left = hold; b = buttons(++period); }
            left--;
            step(b);
            const int sc = score();
            if (sc > prev) ret += (long long)sc - (long long)prev;
            prev = sc;
            lv = lives();
            if (lost_at < 0 && lv < lives0) lost_at = j;
            run_frames = j + 1;
            if (lv <= 0) break;
        }
        return TbxLookFields{ret, prev, lv, run_frames, lost_at};
    }
};
// a refused row: frames run = 0
__device__ __forceinline__ void tbx_lookahead_refuse(double* out)
{
#pragma unroll
    for (int i = 0; i < 5; i++) out[i] = 0.0;
}
// a played row: the five doubles of TBX_QUERY_LOOKAHEAD / _ALL / _PLAN
__device__ __forceinline__ void tbx_lookahead_store(double* out, const TbxLookFields& f)
{
    out[0] = (double)f.ret; out[1] = (double)f.score; out[2] = (double)f.lives; out[3] = (double)f.frames_run; out[4] = (double)f.lost_at;
}
// the (env, candidate) pairs of one launch: the grids of a query stay below 2^30 pairs each
constexpr long long TBX_LOOKAHEAD_PAIRS_PER_LAUNCH = 1ll << 30;
// f(first_pair, count) per launch
template <class F>
void tbx_lookahead_launches(int n, int cands, F&& f)
{
    const long long pairs = (long long)n * cands;
    for (long long p0 = 0; p0 < pairs; p0 += TBX_LOOKAHEAD_PAIRS_PER_LAUNCH)
        f(p0, (int)(pairs - p0 < TBX_LOOKAHEAD_PAIRS_PER_LAUNCH ? pairs - p0 : TBX_LOOKAHEAD_PAIRS_PER_LAUNCH));
}

// ---- The play kernels of every lookahead query (include/toybox_amd.h), written once.  A game hands in a leaf policy G:
//   G::GAME, G::WAVE (a wave per unit, else a thread), G::BLOCK, and
//   TbxLookFields G::leaf(env, lane, look[, salt]) const  -- load env from HBM, play `look` on the registers (run_fields), store
//   nothing; `look` is a TbxLookahead<GAME, PLAN> of either action source.

// TBX_QUERY_LOOKAHEAD / _ALL: a unit per (env, candidate) pair, pair = first_pair + rel; cands = 1: the single form, the first
// action from the arguments.  Thread form: the candidates of an env sit in neighbouring lanes (their state loads hit the same lines).
template <class G>
__global__ __launch_bounds__(G::BLOCK) void tbx_lookahead_kernel(G g, TbxEditArgs a, int cands, long long first_pair, int count, double* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int rel = G::WAVE ? wave_uniform((int)(blockIdx.x * (G::BLOCK / 64) + (threadIdx.x >> 6))) : (int)(blockIdx.x * G::BLOCK + threadIdx.x);
    if (rel >= count) return;
    const long long pair = first_pair + rel;
    int env = (int)(pair / cands), cand = cands > 1 ? (int)(pair - (long long)env * cands) : -1;
    if (G::WAVE) { env = wave_uniform(env); cand = wave_uniform(cand); }
    double* const o = out + pair * 5;
    TbxLookahead<G::GAME> look;
    bool ok = look.read(a, env, cand);
    if (G::WAVE) ok = wave_uniform(ok);
    if (!ok) {
        if (!G::WAVE || lane == 0) tbx_lookahead_refuse(o);
        return;
    }
    if (G::WAVE) look.uniform();
    const TbxLookFields f = g.leaf(env, lane, look);
    if (!G::WAVE || lane == 0) tbx_lookahead_store(o, f);
}

template <class G>
void tbx_launch_lookahead(const G& g, const TbxEditArgs& a, int n, int cands, double* out_dev, hipStream_t s)
{
    tbx_lookahead_launches(n, cands, [&](long long p0, int count) {
        const long long threads = (long long)count * (G::WAVE ? 64 : 1);
        hipLaunchKernelGGL(tbx_lookahead_kernel<G>, dim3((unsigned)((threads + G::BLOCK - 1) / G::BLOCK)), dim3(G::BLOCK), 0, s, g, a, cands, p0, count, out_dev);
    });
}

// "x beats y": a total order once the code breaks the last tie, so the winner does not depend on how the leaves are cut up.
// objective 0 (return): ret, lives, loss; objective 1 (survival): lives, loss, ret; larger wins, then the smaller code.
__device__ __forceinline__ bool tbx_search_better(int objective, const TbxLookFields& x, uint32_t xcode, const TbxLookFields& y, uint32_t ycode)
{
    const int lx = x.lost_at < 0 ? TBX_LOOKAHEAD_MAX_FRAMES + 1 : x.lost_at, ly = y.lost_at < 0 ? TBX_LOOKAHEAD_MAX_FRAMES + 1 : y.lost_at;
    if (objective == 0 && x.ret != y.ret) return x.ret > y.ret;
    if (x.lives != y.lives) return x.lives > y.lives;
    if (lx != ly) return lx > ly;
    if (x.ret != y.ret) return x.ret > y.ret;
    return xcode < ycode;
}
// TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES: "plan x beats plan y" on the integer sums of their S futures -- the order of
// sample_best_action (toybox_amd/envs/vec_env.py) with the code as the last tie-break, so it is total and the winner does not
// depend on how the plans are cut up.  objective 0 (return): larger ret_sum, smaller lost, larger safe_frames_sum; objective 1
// (survival): smaller lost, larger safe_frames_sum, larger ret_sum; then the smaller code.  With one sample this is NOT
// tbx_search_better: that one reads lives, this one the lost flag.
struct TbxSearchSamplesKey {
    long long ret_sum;
    int lost, safe_sum;           // at most TBX_LOOKAHEAD_MAX_SAMPLES futures of at most TBX_LOOKAHEAD_MAX_FRAMES frames: below 2^23
};
__device__ __forceinline__ bool tbx_search_samples_better(int objective, const TbxSearchSamplesKey& x, uint32_t xcode, const TbxSearchSamplesKey& y, uint32_t ycode)
{
    if (objective == 0 && x.ret_sum != y.ret_sum) return x.ret_sum > y.ret_sum;
    if (x.lost != y.lost) return x.lost < y.lost;
    if (x.safe_sum != y.safe_sum) return x.safe_sum > y.safe_sum;
    if (x.ret_sum != y.ret_sum) return x.ret_sum > y.ret_sum;
    return xcode < ycode;
}
// a row of 6 doubles; `none`: no leaf behind it -- the final row of a refused env is zeros, a partial row carries code -1
__device__ __forceinline__ void tbx_search_store(double* o, const TbxLookFields& f, uint32_t code, bool none, bool partial)
{
    o[0] = none ? 0.0 : (double)f.ret; o[1] = none ? 0.0 : (double)f.score; o[2] = none ? 0.0 : (double)f.lives;
    o[3] = none ? 0.0 : (double)f.frames_run; o[4] = none ? 0.0 : (double)f.lost_at; o[5] = none ? (partial ? -1.0 : 0.0) : (double)code;
}

// TBX_QUERY_LOOKAHEAD_PLAN: the cands = 1 form of tbx_lookahead_kernel with the plan as the action source, a unit per env
template <class G>
__global__ __launch_bounds__(G::BLOCK) void tbx_plan_kernel(G g, TbxEditArgs a, int n, double* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int env = G::WAVE ? wave_uniform((int)(blockIdx.x * (G::BLOCK / 64) + (threadIdx.x >> 6))) : (int)(blockIdx.x * G::BLOCK + threadIdx.x);
    if (env >= n) return;
    double* const o = out + (size_t)env * 5;
    TbxLookahead<G::GAME, true> look;
    bool ok = look.read_plan(a, env, 0);
    const double code = a.get(env, 3);
    ok = ok && code >= 0.0 && code < (double)tbx_plan_count(G::GAME, ok ? look.depth : 0);
    look.code = ok ? (uint32_t)code : 0u;
    if (G::WAVE) ok = wave_uniform(ok);
    if (!ok) {
        if (!G::WAVE || lane == 0) tbx_lookahead_refuse(o);
        return;
    }
    if (G::WAVE) look.uniform_plan();
    const TbxLookFields f = g.leaf(env, lane, look);
    if (!G::WAVE || lane == 0) tbx_lookahead_store(o, f);
}

template <class G>
void tbx_launch_plan(const G& g, const TbxEditArgs& a, int n, double* out_dev, hipStream_t s)
{
    const long long threads = (long long)n * (G::WAVE ? 64 : 1);
    hipLaunchKernelGGL(tbx_plan_kernel<G>, dim3((unsigned)((threads + G::BLOCK - 1) / G::BLOCK)), dim3(G::BLOCK), 0, s, g, a, n, out_dev);
}

// TBX_QUERY_LOOKAHEAD_SEARCH: a unit is (env, first action, chunk), unit = (env * n_legal + cand) * chunks + chunk.  It walks the
// suffix codes [chunk * S / chunks, (chunk + 1) * S / chunks) of its env's S = n_legal^(depth - 1) one after the other -- reload,
// play, compare with the best so far (wave forms: in SGPRs) -- and stores ONE row: rows[unit], which with chunks = 1 is the
// query's own output row, otherwise a partial row for tbx_search_pick_kernel.
template <class G>
__global__ __launch_bounds__(G::BLOCK) void tbx_search_kernel(G g, TbxEditArgs a, int chunks, long long first_unit, int count, double* __restrict__ rows)
{
    const int L = tbx_legal_count(G::GAME);
    const int lane = threadIdx.x & 63;
    const int rel = G::WAVE ? wave_uniform((int)(blockIdx.x * (G::BLOCK / 64) + (threadIdx.x >> 6))) : (int)(blockIdx.x * G::BLOCK + threadIdx.x);
    if (rel >= count) return;
    const long long unit = first_unit + rel;
    int env = (int)(unit / (L * chunks));
    const int r = (int)(unit - (long long)env * (L * chunks));
    int cand = r / chunks, chunk = r - cand * chunks;
    TbxLookahead<G::GAME, true> look;
    bool ok = look.read_plan(a, env, 1);
    int objective = a.n > 3 ? a.geti(env, 3) : 0;
    ok = ok && look.depth >= 1 && (objective == 0 || objective == 1);
    uint32_t S = ok ? (uint32_t)tbx_plan_count(G::GAME, look.depth - 1) : 0u;     // (depth <= TBX_PLAN_MAX_DEPTH: below 2^32)
    ok = ok && (uint64_t)S * (uint64_t)L <= (uint64_t)TBX_LOOKAHEAD_MAX_PLANS;
    if (G::WAVE) {
        env = wave_uniform(env); cand = wave_uniform(cand); chunk = wave_uniform(chunk); objective = wave_uniform(objective);
        ok = wave_uniform(ok); S = (uint32_t)wave_uniform((int)S);
        look.uniform_plan();
    }
    TbxLookFields best{0, 0, 0, 0, 0};
    uint32_t best_code = 0;
    bool none = true;
    if (ok) {
        const uint32_t lo = (uint32_t)((uint64_t)chunk * S / (uint32_t)chunks), hi = (uint32_t)((uint64_t)(chunk + 1) * S / (uint32_t)chunks);
        for (uint32_t sfx = lo; sfx < hi; sfx++) {
            look.code = (uint32_t)cand + (uint32_t)L * sfx;
            // every leaf RELOADS its env: with the index opaque the compiler cannot keep a second, pristine copy of the state in
            // registers across the loop (it did: Amidar 85 -> 132 VGPRs, two waves of occupancy) -- the reload hits L2
            int env_now = env;
            if (G::WAVE) asm volatile("" : "+s"(env_now));
            else asm volatile("" : "+v"(env_now));
            const TbxLookFields f = g.leaf(env_now, lane, look);
            if (none || tbx_search_better(objective, f, look.code, best, best_code)) { best = f; best_code = look.code; none = false; }
        }
    }
    if (!G::WAVE || lane == 0) tbx_search_store(rows + unit * 6, best, best_code, none, chunks > 1);
}

template <class G>
void tbx_launch_search(const G& g, const TbxEditArgs& a, int chunks, int first_env, int envs, double* rows, hipStream_t s)
{
    const long long per_env = (long long)tbx_legal_count(G::GAME) * chunks, count = per_env * envs;     // (tbx_range_step: below 2^30)
    const long long threads = count * (G::WAVE ? 64 : 1);
    hipLaunchKernelGGL(tbx_search_kernel<G>, dim3((unsigned)((threads + G::BLOCK - 1) / G::BLOCK)), dim3(G::BLOCK), 0, s, g, a, chunks, per_env * first_env, (int)count, rows);
}

// How many chunks a search is cut into: a power of two, the smallest that brings (env, first action, chunk) units to
// TBX_SEARCH_FILL_WAVES waves -- one per SIMD of an MI355X (256 CUs x 4) -- and at most `suffixes` (the largest power of two
// below it; per-env rows: the suffixes of the deepest tree TBX_LOOKAHEAD_MAX_PLANS allows, a shallower env leaves chunks empty).
// lanes: 64 where a wave is the unit, 1 where a thread is.
constexpr long long TBX_SEARCH_FILL_WAVES = 1024;
inline int tbx_search_chunks(int n, int legal, long long suffixes, int lanes)
{
    const long long want = TBX_SEARCH_FILL_WAVES * (64 / lanes);
    int chunks = 1;
    while ((long long)n * legal * chunks < want && 2ll * chunks <= suffixes) chunks *= 2;
    return chunks;
}
// One launch of a search plays at most this many leaf-frames (plans x frames), so that a single kernel on a shared card stays
// near half a second: profiles/search.md has the rate behind the number.
constexpr long long TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH = 1ll << 31;
// One env range of a beam holds candidates plus two beams in engine-owned scratch; the ranges keep it under this, whatever N and
// width are (a starting value: profiles/beam.md).  It is the budget of every planner query but TBX_QUERY_LOOKAHEAD_TREE_ACT, which
// asks tbx_range_step for TWICE this (its working trees are twice as long as query 160's, and its ranges must not be smaller: a
// second, nearly empty range costs a whole range again).  beam_scratch only grows: an engine that has run that query keeps up to
// 512 MiB for every later planner query, until tbx_destroy.
constexpr size_t TBX_BEAM_SCRATCH_BYTES = 256ull << 20;
// How every planner query cuts its n envs into ranges, the one copy of the rule: the envs of a range stay under `budget`
// leaf-frames (leaf_frames_per_env: leaves x frames of one env; per-env rows: the largest a valid row can ask for) and under
// TBX_LOOKAHEAD_PAIRS_PER_LAUNCH units, where the range keeps scratch (bytes_per_env > 0) under TBX_BEAM_SCRATCH_BYTES, and where
// TBX_OPT_BEAM_RANGE_ENVS is set (range_envs > 0) under that; at most n, at least 1.  scratch_bytes: the scratch budget where it is
// not TBX_BEAM_SCRATCH_BYTES (TBX_QUERY_LOOKAHEAD_TREE_ACT: twice that for trees twice as long, so that its ranges are query 160's).
inline long long tbx_range_step(int n, long long budget, long long leaf_frames_per_env, long long units_per_env, size_t bytes_per_env = 0, int range_envs = 0,
                                size_t scratch_bytes = TBX_BEAM_SCRATCH_BYTES)
{
    long long step = budget / leaf_frames_per_env;
    if (step > TBX_LOOKAHEAD_PAIRS_PER_LAUNCH / units_per_env) step = TBX_LOOKAHEAD_PAIRS_PER_LAUNCH / units_per_env;
    if (bytes_per_env > 0 && step > (long long)(scratch_bytes / bytes_per_env)) step = (long long)(scratch_bytes / bytes_per_env);
    if (range_envs > 0 && step > range_envs) step = range_envs;
    if (step > n) step = n;
    if (step < 1) step = 1;
    return step;
}
// f(first_env, envs) per range of `step` envs, the last one shorter; returns the ranges
template <class F>
int tbx_each_range(int n, long long step, F&& f)
{
    int ranges = 0;
    for (long long e0 = 0; e0 < n; e0 += step, ranges++) f((int)e0, (int)(n - e0 < step ? n - e0 : step));
    return ranges;
}

// ---- TBX_QUERY_LOOKAHEAD_BEAM (include/toybox_amd.h): level after level, tbx_beam_kernel plays the candidates of a level and
// tbx_beam_select_kernel (engine.hip) ranks them per (env, first action) group and writes the kept prefixes of the next level.

// A row {frames, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, width} is a valid beam row; both kernels ask here,
// so they cannot disagree about which envs play.  `game` is a constant in the play kernel and a value in the select kernel.
__device__ __forceinline__ bool tbx_beam_row(int game, const TbxEditArgs& a, int env, int& depth, int& objective, int& width)
{
    const int frames = a.geti(env, 0), hold = a.n > 1 ? a.geti(env, 1) : 1, rest = a.n > 4 ? a.geti(env, 4) : -1;
    depth = a.n > 2 ? a.geti(env, 2) : 1;
    objective = a.n > 3 ? a.geti(env, 3) : 0;
    width = a.n > 9 ? a.geti(env, 9) : 1;
    bool playable = rest == -1;
    for (int i = 0; i < tbx_legal_count(game); i++) playable = playable || rest == tbx_legal_action(game, i);
    return frames >= 1 && frames <= TBX_LOOKAHEAD_MAX_FRAMES && hold >= 1 && depth >= 1 && depth <= tbx_plan_max_depth(game) &&
           (objective == 0 || objective == 1) && playable && width >= 1 && width <= TBX_BEAM_MAX_WIDTH;
}
// |B_level|: how many prefixes a beam of `width` keeps at `level` >= 1 -- 1, then min(width, L * the level before)
__host__ __device__ __forceinline__ int tbx_beam_kept(int legal, int width, int level)
{
    int kept = 1;
    for (int d = 2; d <= level && kept < width; d++) kept = kept * legal < width ? kept * legal : width;
    return kept;
}
// One played candidate: the five fields and the code, integers as the leaf leaves them (32 bytes)
struct TbxBeamCand {
    TbxLookFields f;
    uint32_t code, pad;
};
// The scratch of one env range, indexed by the group's number WITHIN the range: cands[group][stride * L] (candidate slot * L + k
// is child k of the prefix in slot `slot`), beam_in / beam_out[group][stride] the kept prefixes of the level before / of this
// level in rank order.  stride: the widest beam of the range (shared arguments: the width; per-env rows: TBX_BEAM_MAX_WIDTH).
struct TbxBeamScratch {
    TbxBeamCand* cands;
    uint32_t *beam_in, *beam_out;
    int stride;
};

// A unit is (env, first action, beam slot, digit) -- ONE leaf, so at 4 096 envs and width 4 a level is 65 536 waves (or threads)
// and needs no loop, no reload and no running best: unit = ((env - first_env) * L + cand) * slots * kids + slot * kids + k, with
// slots = the most prefixes any env of the launch keeps at level - 1 and kids = L (level 1: one slot, one kid, the prefix {cand}
// itself).  An env whose row is refused, whose own depth is below `level` or whose beam has no prefix in `slot` exits at once.
template <class G>
__global__ __launch_bounds__(G::BLOCK) void tbx_beam_kernel(G g, TbxEditArgs a, int level, int slots, int first_env, int count, TbxBeamScratch sc)
{
    const int L = tbx_legal_count(G::GAME);
    const int lane = threadIdx.x & 63;
    const int rel = G::WAVE ? wave_uniform((int)(blockIdx.x * (G::BLOCK / 64) + (threadIdx.x >> 6))) : (int)(blockIdx.x * G::BLOCK + threadIdx.x);
    if (rel >= count) return;
    const int kids = level == 1 ? 1 : L, per_group = slots * kids;
    const int group = rel / per_group, r = rel - group * per_group;
    int slot = r / kids, k = r - slot * kids;
    int env = first_env + group / L, cand = group % L;
    TbxLookahead<G::GAME, true> look;
    int depth, objective, width;
    bool ok = look.read_plan(a, env, 1);
    ok = tbx_beam_row(G::GAME, a, env, depth, objective, width) && ok;
    ok = ok && level <= depth && slot < tbx_beam_kept(L, width, level - 1);
    uint32_t code = (uint32_t)cand;
    if (ok && level > 1) code = sc.beam_in[(size_t)group * sc.stride + slot] + (uint32_t)k * (uint32_t)tbx_plan_count(G::GAME, level - 1);
    look.depth = level;
    look.code = code;
    if (G::WAVE) {
        env = wave_uniform(env); ok = wave_uniform(ok);
        look.uniform_plan();
    }
    if (!ok) return;
    const TbxLookFields f = g.leaf(env, lane, look);
    if (!G::WAVE || lane == 0) sc.cands[((size_t)group * sc.stride + slot) * L + k] = TbxBeamCand{f, look.code, 0u};
}

template <class G>
void tbx_launch_beam(const G& g, const TbxEditArgs& a, int level, int slots, int first_env, int envs, const TbxBeamScratch& sc, hipStream_t s)
{
    const int L = tbx_legal_count(G::GAME);
    const long long count = (long long)envs * L * slots * (level == 1 ? 1 : L);     // (lookahead_beam, engine.hip: below 2^30)
    const long long threads = count * (G::WAVE ? 64 : 1);
    hipLaunchKernelGGL(tbx_beam_kernel<G>, dim3((unsigned)((threads + G::BLOCK - 1) / G::BLOCK)), dim3(G::BLOCK), 0, s, g, a, level, slots, first_env, (int)count, sc);
}

// ---- TBX_QUERY_LOOKAHEAD_EVOLVE (include/toybox_amd.h): generation after generation, tbx_evolve_kernel plays the individuals of a
// population and tbx_evolve_select_kernel (engine.hip) ranks them per (env, first action) group and breeds the next generation.
// An individual is a whole plan of the row's depth, so the leaf is the plan query's and TbxLookahead gets no branch of its own.

// The values of a row {frames, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, population, generations, elite,
// plan_seed, mutation, init} are a valid evolve row; both kernels ask here (tbx_evolve_row), and so does the host where it has the
// rows (tbx_reduce), so they cannot disagree about which envs play.  `game` is a constant in the play kernel, a value elsewhere.
__host__ __device__ __forceinline__ bool tbx_evolve_values(int game, int frames, int hold, int depth, int objective, int rest, int population, int generations, int elite,
                                                           double plan_seed, int mutation, double init)
{
    bool playable = rest == -1;
    for (int i = 0; i < tbx_legal_count(game); i++) playable = playable || rest == tbx_legal_action(game, i);
    const bool ok = frames >= 1 && frames <= TBX_LOOKAHEAD_MAX_FRAMES && hold >= 1 && depth >= 1 && depth <= tbx_plan_max_depth(game) &&
                    (objective == 0 || objective == 1) && playable && population >= 1 && population <= TBX_EVOLVE_MAX_POPULATION &&
                    generations >= 0 && generations <= TBX_EVOLVE_MAX_GENERATIONS && elite >= 1 && elite <= population &&
                    plan_seed >= 0.0 && plan_seed < 4294967296.0 && mutation >= 0 && mutation <= 256;
    return ok && (init == -1.0 || (init >= 0.0 && init < (double)tbx_plan_count(game, depth)));
}
// What the kernels read of a row beyond the plan query's columns
struct TbxEvolveRow {
    int depth, objective, population, generations, elite, mutation;
    uint32_t plan_seed, init;     // init: read only where has_init
    bool has_init;
};
__device__ __forceinline__ bool tbx_evolve_row(int game, const TbxEditArgs& a, int env, TbxEvolveRow& r)
{
    r.depth = a.n > 2 ? a.geti(env, 2) : 1;
    r.objective = a.n > 3 ? a.geti(env, 3) : 0;
    r.population = a.n > 9 ? a.geti(env, 9) : 1;
    r.generations = a.n > 10 ? a.geti(env, 10) : 0;
    r.elite = a.n > 11 ? a.geti(env, 11) : 1;
    const double plan_seed = a.n > 12 ? a.get(env, 12) : 0.0, init = a.n > 14 ? a.get(env, 14) : -1.0;
    r.mutation = a.n > 13 ? a.geti(env, 13) : 64;
    const bool ok = tbx_evolve_values(game, a.geti(env, 0), a.n > 1 ? a.geti(env, 1) : 1, r.depth, r.objective, a.n > 4 ? a.geti(env, 4) : -1, r.population,
                                      r.generations, r.elite, plan_seed, r.mutation, init);
    r.plan_seed = ok ? (uint32_t)plan_seed : 0u;
    r.has_init = ok && init >= 0.0;
    r.init = r.has_init ? (uint32_t)init : 0u;
    return ok;
}
// The words of the definition: base(plan_seed, first action, env_offset + env), then one draw per (generation, individual, period)
__host__ __device__ __forceinline__ uint64_t tbx_evolve_base(uint32_t plan_seed, int cand, uint64_t env_key)
{
    return tbx_splitmix64(tbx_splitmix64((uint64_t)plan_seed ^ ((uint64_t)cand << 32)) ^ env_key);
}
__host__ __device__ __forceinline__ uint64_t tbx_evolve_word(uint64_t base, int g, int i, int p)
{
    return tbx_splitmix64(base ^ ((uint64_t)g << 40) ^ ((uint64_t)i << 8) ^ (uint64_t)p);
}
// Individual i of generation 0: digit_0 = cand, the others drawn -- or, for individual 0 of a row with an init, taken from it.
// 32-bit arithmetic throughout: a Breakout code of depth 16 reaches 2^32 - 1, and `pow` wraps only after its last use.
__device__ __forceinline__ uint32_t tbx_evolve_first_code(int game, const TbxEvolveRow& r, uint64_t base, int cand, int i)
{
    const uint32_t L = (uint32_t)tbx_legal_count(game);
    if (i == 0 && r.has_init) return r.init - r.init % L + (uint32_t)cand;
    uint32_t code = (uint32_t)cand, pow = L;
    for (int p = 1; p < r.depth; p++, pow *= L) code += (uint32_t)((tbx_evolve_word(base, 0, i, p) >> 32) % L) * pow;
    return code;
}
// The scratch of one env range, indexed by the group's number WITHIN the range: recs[group][stride] the played individuals (slots
// 0 .. elite-1 of a later generation: the records the select pass carried), codes[group][stride] the codes of the generation about
// to be played.  stride: the largest population of the range (shared arguments: the population; per-env rows: the largest there
// can be, or the largest the host saw).
struct TbxEvolveScratch {
    TbxBeamCand* recs;
    uint32_t* codes;
    int stride;
};

// A unit is (env, first action, individual) -- ONE leaf: unit = ((env - first_env) * L + cand) * slots + (i - first_slot), with
// slots individuals from first_slot on per group (generation 0: all of them from 0; later: the elites below first_slot are nobody's
// unit).  An env whose row is refused, whose own generations are below `gen`, whose population has no individual i or whose
// individual i is an elite of this generation (its record was carried) exits at once.
template <class G>
__global__ __launch_bounds__(G::BLOCK) void tbx_evolve_kernel(G g, TbxEditArgs a, int gen, int first_slot, int slots, int first_env, int count, TbxEvolveScratch sc)
{
    const int L = tbx_legal_count(G::GAME);
    const int lane = threadIdx.x & 63;
    const int rel = G::WAVE ? wave_uniform((int)(blockIdx.x * (G::BLOCK / 64) + (threadIdx.x >> 6))) : (int)(blockIdx.x * G::BLOCK + threadIdx.x);
    if (rel >= count) return;
    const int group = rel / slots;
    int i = first_slot + (rel - group * slots);
    int env = first_env + group / L, cand = group % L;
    TbxLookahead<G::GAME, true> look;
    TbxEvolveRow r;
    bool ok = look.read_plan(a, env, 1);
    ok = tbx_evolve_row(G::GAME, a, env, r) && ok;
    ok = ok && gen <= r.generations && i < r.population && (gen == 0 || i >= r.elite);
    uint32_t code = 0;
    if (ok) {
        if (gen == 0) code = tbx_evolve_first_code(G::GAME, r, tbx_evolve_base(r.plan_seed, cand, (uint64_t)a.getu(env, 8) + (uint64_t)env), cand, i);
        else code = sc.codes[(size_t)group * sc.stride + i];
    }
    look.depth = r.depth;
    look.code = code;
    if (G::WAVE) {
        env = wave_uniform(env); ok = wave_uniform(ok); i = wave_uniform(i);
        look.uniform_plan();
    }
    if (!ok) return;
    const TbxLookFields f = g.leaf(env, lane, look);
    if (!G::WAVE || lane == 0) sc.recs[(size_t)group * sc.stride + i] = TbxBeamCand{f, look.code, 0u};
}

template <class G>
void tbx_launch_evolve(const G& g, const TbxEditArgs& a, int gen, int first_slot, int slots, int first_env, int envs, const TbxEvolveScratch& sc, hipStream_t s)
{
    const long long count = (long long)envs * tbx_legal_count(G::GAME) * slots;     // (lookahead_evolve, engine.hip: below 2^30)
    const long long threads = count * (G::WAVE ? 64 : 1);
    hipLaunchKernelGGL(tbx_evolve_kernel<G>, dim3((unsigned)((threads + G::BLOCK - 1) / G::BLOCK)), dim3(G::BLOCK), 0, s, g, a, gen, first_slot, slots, first_env, (int)count, sc);
}

// ---- TBX_QUERY_LOOKAHEAD_SAMPLES (include/toybox_amd.h): `samples` futures per (env, first action), summed on the device.

// The game RNG of a future, between the load and the play: salt 0 leaves it as it stands, otherwise both words become
// splitmix64(word ^ salt) -- the fork's rule (envcopy.hip: env_salt_kernel), here on the registers and never stored.  The leaf()
// of every game policy calls it with its trailing `salt` argument; the plan and search kernels pass none and compile without it.
__device__ __forceinline__ void tbx_salt_rng(Rng& r, uint64_t salt)
{
    if (salt) { r.s0 = tbx_splitmix64(r.s0 ^ salt); r.s1 = tbx_splitmix64(r.s1 ^ salt); }
}

// The eight fields of a row while they are summed: 64-bit integers, so a row does not depend on how its samples are cut up.
struct TbxSampleSums {
    long long n = 0, ret_sum = 0, ret_min = 0, ret_max = 0, lives_sum = 0, lost = 0, ended = 0, safe_sum = 0;
    __device__ __forceinline__ void add(const TbxLookFields& f)
    {
        ret_min = n == 0 || f.ret < ret_min ? f.ret : ret_min;
        ret_max = n == 0 || f.ret > ret_max ? f.ret : ret_max;
        n++;
        ret_sum += f.ret;
        lives_sum += f.lives;
        lost += f.lost_at >= 0 ? 1 : 0;
        ended += f.lives <= 0 ? 1 : 0;
        safe_sum += f.lost_at < 0 ? f.frames_run : f.lost_at;
    }
    // a partial row (n = 0: no sample behind it)
    __device__ __forceinline__ void merge(const long long* p)
    {
        if (p[0] == 0) return;
        ret_min = n == 0 || p[2] < ret_min ? p[2] : ret_min;
        ret_max = n == 0 || p[3] > ret_max ? p[3] : ret_max;
        n += p[0]; ret_sum += p[1]; lives_sum += p[4]; lost += p[5]; ended += p[6]; safe_sum += p[7];
    }
    // the query's own row: converted to binary64 once, here; a refused row (n = 0) is zeros
    __device__ __forceinline__ void store(double* o) const
    {
        o[0] = (double)n; o[1] = (double)ret_sum; o[2] = (double)ret_min; o[3] = (double)ret_max;
        o[4] = (double)lives_sum; o[5] = (double)lost; o[6] = (double)ended; o[7] = (double)safe_sum;
    }
    __device__ __forceinline__ void store_partial(long long* o) const
    {
        o[0] = n; o[1] = ret_sum; o[2] = ret_min; o[3] = ret_max; o[4] = lives_sum; o[5] = lost; o[6] = ended; o[7] = safe_sum;
    }
};

// A unit is (env, first action, chunk), unit = (env * n_legal + cand) * chunks + chunk, as in the search.  It walks the samples
// [chunk * S / chunks, (chunk + 1) * S / chunks) of its env's S one after the other -- reload, salt, play, add (wave forms: in
// SGPRs) -- and stores ONE row of eight: with chunks = 1 the query's own output row (doubles), otherwise a partial row (the 64-bit
// integers as they are, in the same eight words) for tbx_sample_sum_kernel.
template <class G>
__global__ __launch_bounds__(G::BLOCK) void tbx_sample_kernel(G g, TbxEditArgs a, int chunks, long long first_unit, int count, double* __restrict__ rows)
{
    const int L = tbx_legal_count(G::GAME);
    const int lane = threadIdx.x & 63;
    const int rel = G::WAVE ? wave_uniform((int)(blockIdx.x * (G::BLOCK / 64) + (threadIdx.x >> 6))) : (int)(blockIdx.x * G::BLOCK + threadIdx.x);
    if (rel >= count) return;
    const long long unit = first_unit + rel;
    int env = (int)(unit / (L * chunks));
    const int r = (int)(unit - (long long)env * (L * chunks));
    int cand = r / chunks, chunk = r - cand * chunks;
    TbxLookahead<G::GAME, true> look;
    uint64_t seed, env_key;
    bool ok = look.read_samples(a, env, cand, seed, env_key);
    int S = a.n > 2 ? a.geti(env, 2) : 1;
    const double salt_arg = a.n > 3 ? a.get(env, 3) : 0.0;
    ok = ok && S >= 1 && S <= TBX_LOOKAHEAD_MAX_SAMPLES && salt_arg >= 0.0 && salt_arg < 4294967296.0;
    uint64_t salt = ok ? (uint64_t)salt_arg : 0ull;
    ok = ok && (salt == 0 || salt + (uint64_t)S - 1 < (1ull << 32));
    if (G::WAVE) {
        env = wave_uniform(env); cand = wave_uniform(cand); chunk = wave_uniform(chunk);
        ok = wave_uniform(ok); S = wave_uniform(S);
        salt = wave_uniform64(salt); seed = wave_uniform64(seed); env_key = wave_uniform64(env_key);
        look.uniform_plan();
    }
    TbxSampleSums sum;
    if (ok) {
        const int lo = (int)((long long)chunk * S / chunks), hi = (int)((long long)(chunk + 1) * S / chunks);
        for (int s = lo; s < hi; s++) {
            look.key = tbx_splitmix64(seed + (uint64_t)s) ^ env_key;
            // every sample RELOADS its env through an opaque index, as every leaf of the search does (profiles/search.md)
            int env_now = env;
            if (G::WAVE) asm volatile("" : "+s"(env_now));
            else asm volatile("" : "+v"(env_now));
            TbxLookFields f = g.leaf(env_now, lane, look, salt ? salt + (uint64_t)s : 0ull);
            if (G::WAVE) {
                f.ret = (long long)wave_uniform64((uint64_t)f.ret);
                f.lives = wave_uniform(f.lives); f.frames_run = wave_uniform(f.frames_run); f.lost_at = wave_uniform(f.lost_at);
            }
            sum.add(f);
        }
    }
    if (!G::WAVE || lane == 0) {
        if (chunks > 1) sum.store_partial(reinterpret_cast<long long*>(rows) + unit * 8);
        else sum.store(rows + unit * 8);
    }
}

template <class G>
void tbx_launch_sample(const G& g, const TbxEditArgs& a, int chunks, int first_env, int envs, double* rows, hipStream_t s)
{
    const long long per_env = (long long)tbx_legal_count(G::GAME) * chunks, count = per_env * envs;     // (tbx_range_step: below 2^30)
    const long long threads = count * (G::WAVE ? 64 : 1);
    hipLaunchKernelGGL(tbx_sample_kernel<G>, dim3((unsigned)((threads + G::BLOCK - 1) / G::BLOCK)), dim3(G::BLOCK), 0, s, g, a, chunks, per_env * first_env, (int)count, rows);
}

// ---- TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES (include/toybox_amd.h): every plan of a depth on the same `samples` futures, the best
// plan per (env, first action) by the summed outcome.

// A row of 9: the eight sums, then the code.  `none`: no plan behind it -- the final row of a refused env is zeros, a partial row
// carries code -1 (as the search's partial rows do).  Final rows are doubles, partial rows the 64-bit integers as they are.
__device__ __forceinline__ void tbx_search_samples_store(double* o, const TbxSampleSums& sum, uint32_t code, bool none, bool partial)
{
    if (partial) {
        long long* const p = reinterpret_cast<long long*>(o);
        sum.store_partial(p);
        p[8] = none ? -1ll : (long long)code;
    } else {
        sum.store(o);
        o[8] = none ? 0.0 : (double)code;
    }
}

// A unit is (env, first action, chunk), unit = (env * n_legal + cand) * chunks + chunk, as in the search.  It walks the suffix
// codes [chunk * X / chunks, (chunk + 1) * X / chunks) of its env's X = n_legal^(depth - 1) one after the other; per code it runs
// the sample loop of tbx_sample_kernel -- reload, salt, play, add -- over ALL S futures of the env (the same S for every code:
// common random numbers) and compares the sums with the best so far by tbx_search_samples_better.  Wave forms: sums, the best's
// eight sums and control live in SGPRs, one pass.  Thread form (Breakout, 163 VGPRs in the sample kernel, 168 for three waves): a
// second set of sums is 32 registers, so only what the order reads is kept of the running best (TbxSearchSamplesKey and the code:
// the other five sums of the loop are dead there) and a second, short pass replays the S futures of the unit's winner for the full
// eight; a chunk of one code has its winner without the first pass.  The unit stores ONE row of 9: with chunks = 1 the query's own
// output row, otherwise a partial row for tbx_search_samples_pick_kernel.
template <class G>
__global__ __launch_bounds__(G::BLOCK) void tbx_search_samples_kernel(G g, TbxEditArgs a, int chunks, long long first_unit, int count, double* __restrict__ rows)
{
    const int L = tbx_legal_count(G::GAME);
    const int lane = threadIdx.x & 63;
    const int rel = G::WAVE ? wave_uniform((int)(blockIdx.x * (G::BLOCK / 64) + (threadIdx.x >> 6))) : (int)(blockIdx.x * G::BLOCK + threadIdx.x);
    if (rel >= count) return;
    const long long unit = first_unit + rel;
    int env = (int)(unit / (L * chunks));
    const int r = (int)(unit - (long long)env * (L * chunks));
    int cand = r / chunks, chunk = r - cand * chunks;
    TbxLookahead<G::GAME, true> look;
    bool ok = look.read_plan(a, env, 1);
    int objective = a.n > 3 ? a.geti(env, 3) : 0;
    ok = ok && look.depth >= 1 && (objective == 0 || objective == 1);
    uint32_t X = ok ? (uint32_t)tbx_plan_count(G::GAME, look.depth - 1) : 0u;     // (depth <= TBX_PLAN_MAX_DEPTH: below 2^32)
    ok = ok && (uint64_t)X * (uint64_t)L <= (uint64_t)TBX_LOOKAHEAD_MAX_PLANS;
    int S = a.n > 9 ? a.geti(env, 9) : 1;
    const double salt_arg = a.n > 10 ? a.get(env, 10) : 0.0;
    ok = ok && S >= 1 && S <= TBX_LOOKAHEAD_MAX_SAMPLES && (uint64_t)X * (uint64_t)L * (uint64_t)S <= (uint64_t)TBX_LOOKAHEAD_MAX_LEAVES;
    ok = ok && salt_arg >= 0.0 && salt_arg < 4294967296.0;
    uint64_t salt = ok ? (uint64_t)salt_arg : 0ull;
    ok = ok && (salt == 0 || salt + (uint64_t)S - 1 < (1ull << 32));
    uint64_t seed = (uint64_t)a.getu(env, 5) | ((uint64_t)a.getu(env, 6) << 32);
    uint64_t env_key = ((uint64_t)a.getu(env, 8) + (uint64_t)env) << 32;
    if (G::WAVE) {
        env = wave_uniform(env); cand = wave_uniform(cand); chunk = wave_uniform(chunk); objective = wave_uniform(objective);
        ok = wave_uniform(ok); X = (uint32_t)wave_uniform((int)X); S = wave_uniform(S);
        salt = wave_uniform64(salt); seed = wave_uniform64(seed); env_key = wave_uniform64(env_key);
        look.uniform_plan();
    }
    // the S futures of one plan, summed
    auto play = [&](uint32_t code) {
        look.code = code;
        TbxSampleSums sum;
        for (int s = 0; s < S; s++) {
            look.key = tbx_splitmix64(seed + (uint64_t)s) ^ env_key;
            // every leaf RELOADS its env through an opaque index, as every leaf of the search does (profiles/search.md)
            int env_now = env;
            if (G::WAVE) asm volatile("" : "+s"(env_now));
            else asm volatile("" : "+v"(env_now));
            TbxLookFields f = g.leaf(env_now, lane, look, salt ? salt + (uint64_t)s : 0ull);
            if (G::WAVE) {
                f.ret = (long long)wave_uniform64((uint64_t)f.ret);
                f.lives = wave_uniform(f.lives); f.frames_run = wave_uniform(f.frames_run); f.lost_at = wave_uniform(f.lost_at);
            }
            sum.add(f);
        }
        return sum;
    };
    TbxSearchSamplesKey best{0, 0, 0};
    TbxSampleSums win;
    uint32_t best_code = 0;
    bool none = true;
    if (ok) {
        const uint32_t lo = (uint32_t)((uint64_t)chunk * X / (uint32_t)chunks), hi = (uint32_t)((uint64_t)(chunk + 1) * X / (uint32_t)chunks);
        if (!G::WAVE && hi - lo == 1) { best_code = (uint32_t)cand + (uint32_t)L * lo; none = false; }
        else
            for (uint32_t sfx = lo; sfx < hi; sfx++) {
                const uint32_t code = (uint32_t)cand + (uint32_t)L * sfx;
                const TbxSampleSums sum = play(code);
                const TbxSearchSamplesKey key{sum.ret_sum, (int)sum.lost, (int)sum.safe_sum};
                if (none || tbx_search_samples_better(objective, key, code, best, best_code)) {
                    best = key; best_code = code; none = false;
                    if (G::WAVE) win = sum;
                }
            }
    }
    if (!G::WAVE && !none) win = play(best_code);
    if (!G::WAVE || lane == 0) tbx_search_samples_store(rows + unit * 9, win, best_code, none, chunks > 1);
}

template <class G>
void tbx_launch_search_samples(const G& g, const TbxEditArgs& a, int chunks, int first_env, int envs, double* rows, hipStream_t s)
{
    const long long per_env = (long long)tbx_legal_count(G::GAME) * chunks, count = per_env * envs;     // (tbx_range_step: below 2^30)
    const long long threads = count * (G::WAVE ? 64 : 1);
    hipLaunchKernelGGL(tbx_search_samples_kernel<G>, dim3((unsigned)((threads + G::BLOCK - 1) / G::BLOCK)), dim3(G::BLOCK), 0, s, g, a, chunks, per_env * first_env, (int)count, rows);
}

// One launch of TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES plays at most this many leaf-frames, counted over ALL first actions, plans and
// samples of its envs (plans x samples x frames per env): the largest power of two that stays at or below 0.25 s at the rate
// measured for the game's sample kernel (profiles/samples.md, M leaf-frames/s): Breakout, a thread per unit, 21 986 -> 5.50 G in
// 0.25 s -> 2^32; SpaceInvaders 2 915 -> 729 M -> 2^29; Amidar 1 057 -> 264 M -> 2^27 (2^28 = 268 M is above it); GridWorld
// 7 262 -> 1.82 G -> 2^30.  Breakout's wave forms (lanes = 64) have no measured rate: they get the smallest of the four.
// profiles/search_samples.md has the derivation.  TBX_SEARCH_LEAF_FRAMES_PER_LAUNCH and the queries 153 / 154 are left alone.
inline long long tbx_search_samples_budget(int game, int lanes)
{
    switch (game) {
    case TBX_GAME_BREAKOUT: return lanes == 1 ? 1ll << 32 : 1ll << 27;
    case TBX_GAME_SPACE_INVADERS: return 1ll << 29;
    case TBX_GAME_AMIDAR: return 1ll << 27;
    default: return 1ll << 30;
    }
}

// ---- TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES (include/toybox_amd.h): the beam's levels, every candidate valued by the eight sums of its
// `samples` futures (common random numbers: seed_s and salt_s depend on s alone) and ranked by tbx_search_samples_better.
// tbx_beam_samples_kernel plays, tbx_beam_samples_select_kernel (engine.hip) merges, ranks and writes the next beam.

// The values of a row {frames, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, width, samples, salt} are a valid row:
// the beam's ranges, the sample count and salt ranges of TBX_QUERY_LOOKAHEAD_SAMPLES and the leaf cap -- the candidates of the
// widest level (the last) times the samples stay at or below TBX_LOOKAHEAD_MAX_LEAVES.  Both kernels ask here through
// tbx_beam_samples_row, and so does the host where it has the rows (tbx_reduce), so they cannot disagree about which envs play.
__host__ __device__ __forceinline__ bool tbx_beam_samples_values(int game, int frames, int hold, int depth, int objective, int rest, int width, int samples, double salt)
{
    const int L = tbx_legal_count(game);
    bool playable = rest == -1;
    for (int i = 0; i < L; i++) playable = playable || rest == tbx_legal_action(game, i);
    bool ok = frames >= 1 && frames <= TBX_LOOKAHEAD_MAX_FRAMES && hold >= 1 && depth >= 1 && depth <= tbx_plan_max_depth(game) &&
              (objective == 0 || objective == 1) && playable && width >= 1 && width <= TBX_BEAM_MAX_WIDTH;
    ok = ok && samples >= 1 && samples <= TBX_LOOKAHEAD_MAX_SAMPLES && salt >= 0.0 && salt < 4294967296.0;
    ok = ok && ((uint64_t)salt == 0 || (uint64_t)salt + (uint64_t)samples - 1 < (1ull << 32));
    return ok && (long long)L * tbx_beam_kept(L, width, depth - 1) * (depth == 1 ? 1 : L) * samples <= (long long)TBX_LOOKAHEAD_MAX_LEAVES;
}
__device__ __forceinline__ bool tbx_beam_samples_row(int game, const TbxEditArgs& a, int env, int& depth, int& objective, int& width, int& samples, uint64_t& salt)
{
    depth = a.n > 2 ? a.geti(env, 2) : 1;
    objective = a.n > 3 ? a.geti(env, 3) : 0;
    width = a.n > 9 ? a.geti(env, 9) : 1;
    samples = a.n > 10 ? a.geti(env, 10) : 1;
    const double salt_arg = a.n > 11 ? a.get(env, 11) : 0.0;
    const bool ok = tbx_beam_samples_values(game, a.geti(env, 0), a.n > 1 ? a.geti(env, 1) : 1, depth, objective, a.n > 4 ? a.geti(env, 4) : -1, width, samples, salt_arg);
    salt = ok ? (uint64_t)salt_arg : 0ull;
    return ok;
}
// The scratch of one env range: recs[unit][9], one record per unit of the level's play launch in the launch's own unit order (the
// eight sums of the unit's sample chunk as 64-bit integers, then the candidate's code); beam_in / beam_out[group][stride] as in
// TbxBeamScratch, the group's number counted WITHIN the range.
struct TbxBeamSamplesScratch {
    long long* recs;
    uint32_t *beam_in, *beam_out;
    int stride;
};

// A unit is (env, first action, beam slot, digit, sample chunk), indexed as tbx_beam_kernel indexes its units with the chunk
// innermost: unit = (((env - first_env) * L + cand) * slots * kids + slot * kids + k) * chunks + chunk.  It plays the futures
// [chunk * S / chunks, (chunk + 1) * S / chunks) of ONE candidate -- the loop of tbx_sample_kernel: reload through the opaque env
// index, salt, play, add (wave forms: in SGPRs) -- and stores ONE record at its own unit index.  No loop over candidates, no
// running best, nothing between lanes.  A chunk without a sample (an env with fewer samples than the launch has chunks) stores an
// empty record; an env whose row is refused, whose own depth is below `level` or whose beam has no prefix in `slot` exits at once.
template <class G>
__global__ __launch_bounds__(G::BLOCK) void tbx_beam_samples_kernel(G g, TbxEditArgs a, int level, int slots, int chunks, int first_env, int count, TbxBeamSamplesScratch sc)
{
    const int L = tbx_legal_count(G::GAME);
    const int lane = threadIdx.x & 63;
    const int rel = G::WAVE ? wave_uniform((int)(blockIdx.x * (G::BLOCK / 64) + (threadIdx.x >> 6))) : (int)(blockIdx.x * G::BLOCK + threadIdx.x);
    if (rel >= count) return;
    const int kids = level == 1 ? 1 : L, per_group = slots * kids * chunks;
    const int group = rel / per_group, r = rel - group * per_group;
    const int c = r / chunks;
    int chunk = r - c * chunks;
    const int slot = c / kids, k = c - slot * kids;
    int env = first_env + group / L;
    const int cand = group % L;
    TbxLookahead<G::GAME, true> look;
    int depth, objective, width, S;
    uint64_t salt;
    bool ok = look.read_plan(a, env, 1);
    ok = tbx_beam_samples_row(G::GAME, a, env, depth, objective, width, S, salt) && ok;
    ok = ok && level <= depth && slot < tbx_beam_kept(L, width, level - 1);
    uint32_t code = (uint32_t)cand;
    if (ok && level > 1) code = sc.beam_in[(size_t)group * sc.stride + slot] + (uint32_t)k * (uint32_t)tbx_plan_count(G::GAME, level - 1);
    look.depth = level;
    look.code = code;
    uint64_t seed = (uint64_t)a.getu(env, 5) | ((uint64_t)a.getu(env, 6) << 32);
    uint64_t env_key = ((uint64_t)a.getu(env, 8) + (uint64_t)env) << 32;
    if (G::WAVE) {
        env = wave_uniform(env); chunk = wave_uniform(chunk); ok = wave_uniform(ok); S = wave_uniform(S);
        salt = wave_uniform64(salt); seed = wave_uniform64(seed); env_key = wave_uniform64(env_key);
        look.uniform_plan();
    }
    if (!ok) return;
    TbxSampleSums sum;
    const int lo = (int)((long long)chunk * S / chunks), hi = (int)((long long)(chunk + 1) * S / chunks);
    for (int s = lo; s < hi; s++) {
        look.key = tbx_splitmix64(seed + (uint64_t)s) ^ env_key;
        // every future RELOADS its env through an opaque index, as every sample of tbx_sample_kernel does (profiles/search.md)
        int env_now = env;
        if (G::WAVE) asm volatile("" : "+s"(env_now));
        else asm volatile("" : "+v"(env_now));
        TbxLookFields f = g.leaf(env_now, lane, look, salt ? salt + (uint64_t)s : 0ull);
        if (G::WAVE) {
            f.ret = (long long)wave_uniform64((uint64_t)f.ret);
            f.lives = wave_uniform(f.lives); f.frames_run = wave_uniform(f.frames_run); f.lost_at = wave_uniform(f.lost_at);
        }
        sum.add(f);
    }
    if (!G::WAVE || lane == 0) {
        long long* const p = sc.recs + (size_t)rel * 9;
        sum.store_partial(p);
        p[8] = (long long)look.code;
    }
}

template <class G>
void tbx_launch_beam_samples(const G& g, const TbxEditArgs& a, int level, int slots, int chunks, int first_env, int envs, const TbxBeamSamplesScratch& sc, hipStream_t s)
{
    const int L = tbx_legal_count(G::GAME);
    const long long count = (long long)envs * L * slots * (level == 1 ? 1 : L) * chunks;     // (lookahead_beam_samples, engine.hip: below 2^30)
    const long long threads = count * (G::WAVE ? 64 : 1);
    hipLaunchKernelGGL(tbx_beam_samples_kernel<G>, dim3((unsigned)((threads + G::BLOCK - 1) / G::BLOCK)), dim3(G::BLOCK), 0, s, g, a, level, slots, chunks, first_env, (int)count, sc);
}

// ---- TBX_QUERY_LOOKAHEAD_TREE (include/toybox_amd.h): open-loop tree search over plan prefixes.  A node of depth d IS a plan code
// of depth d, selection reads visit statistics and never simulated state, and one simulation is the plan query's leaf on future m --
// so the play step is leaf(env, lane, look, salt_m), unchanged, and the tree is all that is new.

// The values of a row {frames, hold, depth, objective, rest, seed_lo, seed_hi, t, env_offset, simulations, explore, salt} are a valid
// tree row; the kernel asks here (tbx_tree_row), and so does the host where it has the rows (tbx_reduce).
__host__ __device__ __forceinline__ bool tbx_tree_values(int game, int frames, int hold, int depth, int objective, int rest, int simulations, int explore, double salt)
{
    bool playable = rest == -1;
    for (int i = 0; i < tbx_legal_count(game); i++) playable = playable || rest == tbx_legal_action(game, i);
    const bool ok = frames >= 1 && frames <= TBX_LOOKAHEAD_MAX_FRAMES && hold >= 1 && depth >= 1 && depth <= tbx_plan_max_depth(game) &&
                    (objective == 0 || objective == 1) && playable && simulations >= 1 && simulations <= TBX_TREE_MAX_SIMULATIONS &&
                    explore >= 0 && explore <= TBX_TREE_MAX_EXPLORE && salt >= 0.0 && salt < 4294967296.0;
    return ok && ((uint64_t)salt == 0 || (uint64_t)salt + (uint64_t)simulations - 1 < (1ull << 32));
}
__device__ __forceinline__ bool tbx_tree_row(int game, const TbxEditArgs& a, int env, int& depth, int& objective, int& simulations, int& explore, uint64_t& salt)
{
    depth = a.n > 2 ? a.geti(env, 2) : 1;
    objective = a.n > 3 ? a.geti(env, 3) : 0;
    simulations = a.n > 9 ? a.geti(env, 9) : 1;
    explore = a.n > 10 ? a.geti(env, 10) : 0;
    const double salt_arg = a.n > 11 ? a.get(env, 11) : 0.0;
    const bool ok = tbx_tree_values(game, a.geti(env, 0), a.n > 1 ? a.geti(env, 1) : 1, depth, objective, a.n > 4 ? a.geti(env, 4) : -1, simulations, explore, salt_arg);
    salt = ok ? (uint64_t)salt_arg : 0ull;
    return ok;
}
// One node, 32 bytes: link 0 is "no child" (node 0 is the root, nobody's child), and TBX_TREE_MAX_SIMULATIONS + 1 nodes keep the
// ids in 16 bits.  `nodes`, the nodes of the tree so far, is read in the root alone.
struct TbxTreeNode {
    long long v_sum;
    uint32_t n;
    uint16_t child[6];
    uint32_t nodes, pad;
};
static_assert(sizeof(TbxTreeNode) == 32, "two nodes a 64-byte line");
// The scratch of one env range, indexed by the unit's number WITHIN the range: per unit a block of unit_bytes() -- the root's eight
// sums (64-bit integers, one 64-byte line), then `stride` nodes in creation order, stride even -- so a block is whole 64-byte lines
// and no lane's stores share a line with another lane's.  A lane's loads are its own lines too: nothing here coalesces, and nothing
// needs to (profiles/tree.md: a path of at most 16 nodes per `frames` steps of play).
struct TbxTreeScratch {
    uint8_t* base;
    int stride;
    int preloaded;      // TBX_QUERY_LOOKAHEAD_TREE_ACT: the start trees are in place (tbx_tree_load_kernel, engine.hip); the launch with m0 = 0 makes none
    __host__ __device__ static size_t unit_bytes(int stride) { return 64 + (size_t)stride * sizeof(TbxTreeNode); }
    __host__ __device__ static int stride_for(int simulations) { return (simulations + 2) & ~1; }       // simulations + 1 nodes, rounded up to even
    __device__ __forceinline__ long long* sums(int unit) const { return reinterpret_cast<long long*>(base + (size_t)unit * unit_bytes(stride)); }
    __device__ __forceinline__ TbxTreeNode* nodes(int unit) const { return reinterpret_cast<TbxTreeNode*>(base + (size_t)unit * unit_bytes(stride) + 64); }
};
// The exact floor square root of 0 <= x < 2^52.  Such an x is a double, and its double square root is correctly rounded (IEEE 754):
// within half a unit in the last place of the real root, far less than 1 at these sizes.  So the truncated r is at most one off the
// floor root -- one above where the rounding went up across an integer -- and the one correction step below repairs an r that is
// off by one in either direction.  The result is therefore exact far beyond the tree's largest argument, n << 16 with n <= 5120
// (TBX_QUERY_LOOKAHEAD_TREE_ACT: below 2^29); r * r stays far inside 64 bits.
__host__ __device__ __forceinline__ long long tbx_isqrt(long long x)
{
    long long r = (long long)sqrt((double)x);
    if (r * r > x) r--;
    else if ((r + 1) * (r + 1) <= x) r++;
    return r;
}
// Selection of one simulation in the tree `nd` of first action `cand`: walks from the root by priority, expands at most one node,
// and leaves the plan to play in depth_out / code_out.  Every node is read where it lies; nothing is kept in a per-thread array.
template <int GAME>
__device__ __forceinline__ void tbx_tree_select(TbxTreeNode* nd, int stride, int cand, int depth, long long explore, int& depth_out, uint32_t& code_out)
{
    const int L = tbx_legal_count(GAME);
    int cur = 0, d = 1;
    uint32_t code = (uint32_t)cand, pow = (uint32_t)L;        // (pow wraps only after its last use, as in tbx_evolve_first_code)
    while (d < depth) {
        int miss = -1;
#pragma unroll
        for (int k = L - 1; k >= 0; k--) miss = nd[cur].child[k] == 0 ? k : miss;
        if (miss >= 0) {
            const uint32_t id = nd[0].nodes;
            if (id >= (uint32_t)stride) break;                 // (never: a simulation adds at most one node, and stride > simulations)
            nd[0].nodes = id + 1;
            TbxTreeNode fresh{};
            nd[id] = fresh;
            nd[cur].child[miss] = (uint16_t)id;
            code += (uint32_t)miss * pow;
            d++;
            break;
        }
        const long long root_term = explore * tbx_isqrt((long long)nd[cur].n << 16);
        int best = 0, best_child = 0;
        long long best_p = 0;
#pragma unroll
        for (int k = 0; k < L; k++) {
            const int c = nd[cur].child[k];
            const long long n_k = nd[c].n;
            const long long p = nd[c].v_sum * 256 / (n_k > 0 ? n_k : 1) + root_term / (1 + n_k);
            if (k == 0 || p > best_p) { best = k; best_child = c; best_p = p; }
        }
        code += (uint32_t)best * pow;
        pow *= (uint32_t)L;
        d++;
        cur = best_child;
    }
    depth_out = d;
    code_out = code;
}
// Backup of value v along the path of `code` at depth d: a second descent from the root by the digits of the code -- no path stack
template <int GAME>
__device__ __forceinline__ void tbx_tree_backup(TbxTreeNode* nd, int d, uint32_t code, long long v)
{
    const uint32_t L = (uint32_t)tbx_legal_count(GAME);
    int cur = 0;
    uint32_t c = code / L;
    for (int level = 1; level <= d; level++, c /= L) {
        nd[cur].n += 1;
        nd[cur].v_sum += v;
        if (level < d) cur = nd[cur].child[c % L];
    }
}
// The row's last four: the principal variation from the root -- the child with the largest n, then the larger v_sum, then the smaller k
template <int GAME>
__device__ __forceinline__ void tbx_tree_store_pv(const TbxTreeNode* nd, int cand, double* o)
{
    const int L = tbx_legal_count(GAME);
    int cur = 0, d = 1;
    uint32_t code = (uint32_t)cand, pow = (uint32_t)L;
    for (;;) {
        int best = -1, best_child = 0;
#pragma unroll
        for (int k = 0; k < L; k++) {
            const int c = nd[cur].child[k];
            if (c == 0) continue;
            if (best < 0 || nd[c].n > nd[best_child].n || (nd[c].n == nd[best_child].n && nd[c].v_sum > nd[best_child].v_sum)) { best = k; best_child = c; }
        }
        if (best < 0) break;
        code += (uint32_t)best * pow;
        pow *= (uint32_t)L;
        d++;
        cur = best_child;
    }
    o[8] = (double)code; o[9] = (double)d; o[10] = (double)nd[cur].n; o[11] = (double)nd[cur].v_sum;
}

// A unit is (env, first action), unit = (env - first_env) * L + cand: neighbouring lanes hold the actions of one env, as in
// tbx_lookahead_kernel.  It runs the simulations m0 .. m1-1 of its tree (its own row may have fewer) one after the other -- select,
// play through the opaque env index (reload, salt: the loop of tbx_sample_kernel), back up, add to the root's sums -- with the tree
// and the sums in scratch from launch to launch: the launch with m0 = 0 makes the empty tree, the one that holds the row's last
// simulation stores the row (sc.preloaded: the start trees are there already, only the sums are zeroed).  Wave forms: lane 0 walks
// and updates the tree, depth and code are broadcast before the play.  A refused row answers zeros at m0 = 0.
template <class G>
__global__ __launch_bounds__(G::BLOCK) void tbx_tree_kernel(G g, TbxEditArgs a, int m0, int m1, int first_env, int count, TbxTreeScratch sc, double* __restrict__ out)
{
    const int L = tbx_legal_count(G::GAME);
    const int lane = threadIdx.x & 63;
    const int rel = G::WAVE ? wave_uniform((int)(blockIdx.x * (G::BLOCK / 64) + (threadIdx.x >> 6))) : (int)(blockIdx.x * G::BLOCK + threadIdx.x);
    if (rel >= count) return;
    int env = first_env + rel / L, cand = rel % L;
    const bool writer = !G::WAVE || lane == 0;
    double* const o = out + ((size_t)env * L + cand) * 12;
    TbxLookahead<G::GAME, true> look;
    int depth, objective, M, explore;
    uint64_t salt;
    bool ok = look.read_plan(a, env, 1);
    ok = tbx_tree_row(G::GAME, a, env, depth, objective, M, explore, salt) && ok;
    uint64_t seed = (uint64_t)a.getu(env, 5) | ((uint64_t)a.getu(env, 6) << 32);
    uint64_t env_key = ((uint64_t)a.getu(env, 8) + (uint64_t)env) << 32;
    if (G::WAVE) {
        env = wave_uniform(env); cand = wave_uniform(cand); ok = wave_uniform(ok);
        depth = wave_uniform(depth); objective = wave_uniform(objective); M = wave_uniform(M); explore = wave_uniform(explore);
        salt = wave_uniform64(salt); seed = wave_uniform64(seed); env_key = wave_uniform64(env_key);
    }
    if (!ok) {
        if (writer && m0 == 0)
            for (int i = 0; i < 12; i++) o[i] = 0.0;
        return;
    }
    if (m0 >= M) return;
    const int last = m1 < M ? m1 : M;
    long long* const sums = sc.sums(rel);
    TbxTreeNode* const nd = sc.nodes(rel);
    if (writer && m0 == 0) {
        for (int i = 0; i < 8; i++) sums[i] = 0;
        if (!sc.preloaded) {
            TbxTreeNode root{};
            root.nodes = 1;
            nd[0] = root;
        }
    }
    for (int m = m0; m < last; m++) {
        int d = 1;
        uint32_t code = (uint32_t)cand;
        if (writer) tbx_tree_select<G::GAME>(nd, sc.stride, cand, depth, (long long)explore, d, code);
        look.depth = d;
        look.code = code;
        look.key = tbx_splitmix64(seed + (uint64_t)m) ^ env_key;
        if (G::WAVE) look.uniform_plan();
        // every simulation RELOADS its env through an opaque index, as every sample of tbx_sample_kernel does (profiles/search.md)
        int env_now = env;
        if (G::WAVE) asm volatile("" : "+s"(env_now));
        else asm volatile("" : "+v"(env_now));
        TbxLookFields f = g.leaf(env_now, lane, look, salt ? salt + (uint64_t)m : 0ull);
        if (G::WAVE) {
            f.ret = (long long)wave_uniform64((uint64_t)f.ret);
            f.lives = wave_uniform(f.lives); f.frames_run = wave_uniform(f.frames_run); f.lost_at = wave_uniform(f.lost_at);
        }
        if (writer) {
            const long long safe = f.lost_at < 0 ? f.frames_run : f.lost_at;
            tbx_tree_backup<G::GAME>(nd, look.depth, look.code, objective == 0 ? f.ret : safe);
            const bool first = sums[0] == 0;
            sums[2] = first || f.ret < sums[2] ? f.ret : sums[2];
            sums[3] = first || f.ret > sums[3] ? f.ret : sums[3];
            sums[0] += 1; sums[1] += f.ret; sums[4] += f.lives; sums[5] += f.lost_at >= 0 ? 1 : 0; sums[6] += f.lives <= 0 ? 1 : 0; sums[7] += safe;
        }
    }
    if (writer && last == M) {
        for (int i = 0; i < 8; i++) o[i] = (double)sums[i];
        tbx_tree_store_pv<G::GAME>(nd, cand, o);
    }
}

template <class G>
void tbx_launch_tree(const G& g, const TbxEditArgs& a, int m0, int m1, int first_env, int envs, const TbxTreeScratch& sc, double* out, hipStream_t s)
{
    const long long count = (long long)envs * tbx_legal_count(G::GAME);     // (lookahead_tree, engine.hip: below 2^30)
    const long long threads = count * (G::WAVE ? 64 : 1);
    hipLaunchKernelGGL(tbx_tree_kernel<G>, dim3((unsigned)((threads + G::BLOCK - 1) / G::BLOCK)), dim3(G::BLOCK), 0, s, g, a, m0, m1, first_env, (int)count, sc, out);
}

// One play launch of a planner query as the engine hands it to the game (GameOps::lookahead_play): which query, the env range, and
// of the rest what that query's tbx_launch_* above takes.  TBX_QUERY_LOOKAHEAD / _ALL / _PLAN: every env, first_env = 0, rows = the
// output.
struct TbxPlanLaunch {
    int query;                       // TBX_QUERY_LOOKAHEAD / _ALL / _PLAN / _SEARCH / _SAMPLES / _SEARCH_SAMPLES / _BEAM / _EVOLVE / _BEAM_SAMPLES / _TREE
    int first_env, envs, chunks;
    int level, first_slot, slots;    // level: the beam's level or the generation; the tree: simulations first_slot .. first_slot + slots - 1
    double* rows;
    union {                          // the scratch view of the query
        TbxBeamScratch beam;
        TbxEvolveScratch evolve;
        TbxBeamSamplesScratch beam_samples;
        TbxTreeScratch tree;
    };
};
// the play kernel of l.query with the game's leaf policy g; false: no arm for that query, nothing launched.  A plain switch: every
// arm is instantiated for every policy handed in.
template <class G>
bool tbx_launch_planner(const G& g, const TbxEditArgs& a, const TbxPlanLaunch& l, hipStream_t s)
{
    switch (l.query) {
    case TBX_QUERY_LOOKAHEAD: tbx_launch_lookahead(g, a, l.envs, 1, l.rows, s); break;
    case TBX_QUERY_LOOKAHEAD_ALL: tbx_launch_lookahead(g, a, l.envs, tbx_legal_count(G::GAME), l.rows, s); break;
    case TBX_QUERY_LOOKAHEAD_PLAN: tbx_launch_plan(g, a, l.envs, l.rows, s); break;
    case TBX_QUERY_LOOKAHEAD_SEARCH: tbx_launch_search(g, a, l.chunks, l.first_env, l.envs, l.rows, s); break;
    case TBX_QUERY_LOOKAHEAD_SAMPLES: tbx_launch_sample(g, a, l.chunks, l.first_env, l.envs, l.rows, s); break;
    case TBX_QUERY_LOOKAHEAD_SEARCH_SAMPLES: tbx_launch_search_samples(g, a, l.chunks, l.first_env, l.envs, l.rows, s); break;
    case TBX_QUERY_LOOKAHEAD_BEAM: tbx_launch_beam(g, a, l.level, l.slots, l.first_env, l.envs, l.beam, s); break;
    case TBX_QUERY_LOOKAHEAD_EVOLVE: tbx_launch_evolve(g, a, l.level, l.first_slot, l.slots, l.first_env, l.envs, l.evolve, s); break;
    case TBX_QUERY_LOOKAHEAD_BEAM_SAMPLES: tbx_launch_beam_samples(g, a, l.level, l.slots, l.chunks, l.first_env, l.envs, l.beam_samples, s); break;
    case TBX_QUERY_LOOKAHEAD_TREE: tbx_launch_tree(g, a, l.first_slot, l.first_slot + l.slots, l.first_env, l.envs, l.tree, l.rows, s); break;
    default: return false;
    }
    return true;
}

// One per-env array of an engine as the env-copy kernels see it (envcopy.hip: fork, checkpoint save and restore) -- `fields`
// planes of N rows of row_bytes each, [fields][N][row_bytes].  A struct-of-arrays scalar [F][N] is F planes of 4- or 8-byte rows,
// an env-major table [N][R] one plane of R-byte rows, the plane ring `stack` planes of out_h * out_w bytes.  rng_words > 0: every
// row holds that many 64-bit RNG words at byte rng_off (what a `salt` argument rewrites in the envs that were written).
// A row is LIVE (in the engine's array at `base`, planes as they lie) or PACKED (in a packed copy of all arrays -- the fork's
// scratch, a slot of the checkpoint store -- at byte packed_off of it, planes in LOGICAL order).  rot: the live plane that is
// first in logical order (the plane ring: its oldest plane, head + 1); plane c of a packed copy is live plane (rot + c) % fields.
struct TbxEnvSeg {
    uint8_t* base;
    uint64_t packed_off;          // filled in by env_plan (envcopy.hip)
    uint32_t fields, row_bytes, rng_off, rng_words, rot;
};
struct TbxEnvPlan {
    std::vector<TbxEnvSeg> segs;
    template <typename T>
    void soa(T* base, int fields, int rng_words = 0)           // [fields][N] scalars
    {
        if (base) segs.push_back(TbxEnvSeg{reinterpret_cast<uint8_t*>(base), 0, (uint32_t)fields, (uint32_t)sizeof(T), 0u, (uint32_t)rng_words, 0u});
    }
    void rows(void* base, size_t row_bytes, int fields = 1, size_t rng_off = 0, int rng_words = 0)   // [fields][N][row_bytes]
    {
        if (base) segs.push_back(TbxEnvSeg{static_cast<uint8_t*>(base), 0, (uint32_t)fields, (uint32_t)row_bytes, (uint32_t)rng_off, (uint32_t)rng_words, 0u});
    }
};

// How one per-env device array of a state struct (AmiDev, SiDev, GwDev, BrkDev, ...) lies in memory, in the two forms the env
// plan takes.  Every such struct lists its arrays ONCE, in a constexpr member template `arrays(f)` that calls f(member, TbxLayout)
// per array; allocation, release and the env plan of an instance are derived from that list by the helpers below, and a
// static_assert next to the list compares tbx_array_count with the struct's size, so a pointer member without an entry does not build.
struct TbxLayout {
    uint32_t fields, row_bytes, rng_off, rng_words;   // row_bytes 0: the element's size
    bool lazy;                                        // made on demand by a call of its own, not with the instance (BrkDev::custom)
};
constexpr TbxLayout tbx_soa(int fields, int rng_words = 0) { return TbxLayout{(uint32_t)fields, 0u, 0u, (uint32_t)rng_words, false}; }   // [fields][N] elements
constexpr TbxLayout tbx_rows(size_t row_bytes, int fields = 1, size_t rng_off = 0, int rng_words = 0)                            // [fields][N][row_bytes]
{
    return TbxLayout{(uint32_t)fields, (uint32_t)row_bytes, (uint32_t)rng_off, (uint32_t)rng_words, false};
}
constexpr TbxLayout tbx_lazy(TbxLayout l) { l.lazy = true; return l; }
template <class Dev>
constexpr int tbx_array_count()
{
    Dev x{};
    int k = 0;
    x.arrays([&k](auto*&, TbxLayout) { k++; });
    return k;
}
// f(void** member, layout with row_bytes filled in, bytes for n envs) per array
template <class Dev, class F>
void tbx_each_array(Dev& x, size_t n, F&& f)
{
    x.arrays([&](auto*& p, TbxLayout l) {
        if (!l.row_bytes) l.row_bytes = (uint32_t)sizeof(*p);
        f(reinterpret_cast<void**>(&p), l, (size_t)l.fields * n * l.row_bytes);
    });
}
template <class Dev>
void tbx_free_arrays(Dev& x)
{
    tbx_each_array(x, 0, [](void** p, TbxLayout, size_t) { hipFree(*p); *p = nullptr; });
}
// Every listed array of one instance for n envs (lazy: the lazy ones instead).  All or nothing: after a failed hipMalloc what was
// made is freed again and every one of these pointers is null, so "already made" is any one of them.  (What the pointers held
// before is NOT freed: a snapshot slot starts as a copy of the live state.)
template <class Dev>
hipError_t tbx_alloc_arrays(Dev& x, size_t n, bool lazy = false)
{
    hipError_t r = hipSuccess;
    tbx_each_array(x, n, [&](void** p, TbxLayout l, size_t) { if (l.lazy == lazy) *p = nullptr; });
    tbx_each_array(x, n, [&](void** p, TbxLayout l, size_t bytes) {
        if (l.lazy == lazy && r == hipSuccess && (r = hipMalloc(p, bytes)) != hipSuccess) *p = nullptr;
    });
    if (r != hipSuccess) tbx_each_array(x, n, [&](void** p, TbxLayout l, size_t) { if (l.lazy == lazy) { hipFree(*p); *p = nullptr; } });
    return r;
}
template <class Dev>
hipError_t tbx_zero_arrays(Dev& x, size_t n)
{
    hipError_t r = hipSuccess;
    tbx_each_array(x, n, [&](void** p, TbxLayout, size_t bytes) { if (r == hipSuccess && *p) r = hipMemset(*p, 0, bytes); });
    return r;
}
// the arrays of one instance that exist, appended to an env plan; live: its RNG words are the ones a `salt` rewrites
template <class Dev>
void tbx_list_arrays(TbxEnvPlan& plan, Dev& x, bool live)
{
    tbx_each_array(x, 0, [&](void** p, TbxLayout l, size_t) { plan.rows(*p, l.row_bytes, (int)l.fields, live ? l.rng_off : 0, live ? (int)l.rng_words : 0); });
}
// what every game's state struct holds of the engine's common buffers (duck-typed: the structs order these members differently)
template <class Dev>
void tbx_bind_outputs(Dev& d, const tbx_engine* e)
{
    d.reward = e->reward; d.done = e->done; d.lives_out = e->lives_out; d.score_out = e->score_out; d.packed = e->packed;
}
template <class Dev>
void tbx_bind_engine(Dev& d, const tbx_engine* e)
{
    d.n = e->n;
    d.sim_rng = e->sim_rng; d.prev_score = e->prev_score; d.err_flag = e->err_flag;
    tbx_bind_outputs(d, e);
}
// one wave per item, TBX_WAVES_PER_BLOCK waves per block
inline dim3 grid_for(int count) { return dim3((count + TBX_WAVES_PER_BLOCK - 1) / TBX_WAVES_PER_BLOCK); }

// per-game operations; all launches are asynchronous on `s`
struct GameOps {
    virtual ~GameOps() {}
    virtual int init(tbx_engine* e, const void* cfg, size_t cfg_size) = 0;
    virtual void destroy(tbx_engine* e) = 0;
    virtual int height() const = 0;
    virtual int width() const = 0;
    virtual size_t state_size() const = 0;
    virtual size_t config_size() const = 0;
    virtual int get_config(tbx_engine* e, void* pod) = 0;
    virtual int set_config(tbx_engine* e, const void* pod) = 0;
    virtual int new_game(tbx_engine* e, const uint8_t* mask_dev, hipStream_t s) = 0;
    virtual int step(tbx_engine* e, const ActionSource& src, uint32_t flags, hipStream_t s) = 0;
    virtual int render(tbx_engine* e, uint8_t* out_dev, int channels, int first_env, int n_envs, hipStream_t s) = 0;
    // pack envs [env, env+count) -> e->staging (device, count records), unpack host records -> those envs
    virtual int pack_state(tbx_engine* e, int env, int count, hipStream_t s) = 0;
    virtual int unpack_state(tbx_engine* e, int env, int count, const void* pod_host, hipStream_t s) = 0;
    virtual int scalars(tbx_engine* e, int32_t* score_dev, int32_t* lives_dev, int32_t* level_dev, hipStream_t s) = 0;
    // launch the resident single-env step kernel for env 0 on `s` (tbx_serve_loop); optional
    virtual int serve(tbx_engine*, TbxServeCtl* /*ctl_dev*/, hipStream_t) { return TBX_E_UNSUPPORTED; }
    virtual bool serve_paints() const { return false; }        // the resident kernel can rasterise env 0 on request
    // ---- agent layer (agent.hip).  The two-frame buffer of MaxAndSkipEnv lives with the game as two snapshot slots.
    virtual int agent_prepare(tbx_engine*) { return TBX_OK; }  // allocate the slots
    virtual bool multi_frame_step() const { return false; }   // step() honours ActionSource::frames and writes the slots itself
    // single-frame launches: copy the live state of the envs with exec_flag set into slot 0 (A) / 1 (B), set their valid bit
    virtual int agent_snapshot(tbx_engine*, int /*slot*/, const uint8_t* /*exec_flag*/, uint8_t* /*buf_valid*/, hipStream_t) { return TBX_E_UNSUPPORTED; }
    // fused observation kernels (no full-resolution frame leaves the chip)
    virtual bool agent_fused() const { return false; }
    virtual int agent_warp(tbx_engine*, const struct AgentWarpArgs&, hipStream_t) { return TBX_E_UNSUPPORTED; }
    // pipelined mode: the rasteriser reads records the step kernel writes, and there are two buffers of them -- a batch step
    // may then run while the previous frame is still being rasterised.  pipeline_ok(): this engine can (canonical state
    // layout, thread-per-env step); records_parity(): the buffer a render launched now reads; step_ahead(): one frame of
    // every env on stream s, records into the OTHER buffer, which becomes the current one.  The step outputs go wherever
    // tbx_engine::reward / done / ... point at the time of the launch (rebind_outputs() after the engine moved them).
    virtual bool pipeline_ok() const { return false; }
    // TBX_OPT_PIPELINE = 1, the engine's choice: the mode (0, 2 or 3) for a batch of n envs, with or without a per-step gather.
    // Large batches: stream order for every game since the rasterisers stagger their first waves (raster.hpp) -- what values 2
    // and 3 bought Breakout and SpaceInvaders there was a rasteriser launch that did not start against an idle memory system.
    // Small batches without a gather: overlapped launches (value 3) where they measure faster (BrkOps, SiOps); a gather adds
    // cross-queue dependencies that cost more than the overlap gains.
    virtual int pipeline_auto(int /*n*/, bool /*gather*/) const { return 0; }
    virtual int records_parity() const { return 0; }
    virtual bool records_valid() const { return true; }        // false: the next render starts from live state (prep kernel / state-reading rasteriser)
    virtual int step_ahead(tbx_engine*, const ActionSource&, uint32_t, hipStream_t) { return TBX_E_UNSUPPORTED; }
    virtual void rebind_outputs(tbx_engine*) {}
    // tbx_render_step_synthetic: the rasteriser of the current frame and the batch step to the next one as ONE launch on s
    // (engines whose rasteriser reads step-written records); render_step_fused() false: the engine runs render(), then step()
    virtual bool render_step_fused(int /*channels*/) const { return false; }
    // ov != nullptr: an overlapped launch (pipeline.hip, fused_overlapped) -- its step blocks bump ov->arrive when their stores are visible
    // device-wide, ov->done rides on the launch as its completion event, ov->step_blocks is filled in
    virtual int render_step(tbx_engine*, uint8_t* /*out_dev*/, int /*channels*/, const ActionSource&, uint32_t /*flags*/, hipStream_t,
                            TbxOverlapLaunch* /*ov*/ = nullptr) { return TBX_E_UNSUPPORTED; }
    // TBX_OPT_FUSED_OVERLAP = 0, the engine's choice: overlap consecutive fused launches for a batch of n envs?
    // (gather_kind: 0 no record gather, 1 one collective per step, 2 a K-step ring)
    virtual bool fused_overlap_auto(int /*n*/, int /*gather_kind*/) const { return false; }
    // tbx_rollout_synthetic as chunks (pipeline.hip, rollout_chunked).  rollout_ok(): this engine can right now (canonical state layout, RGB /
    // RGBA); rollout_auto(): the engine's choice for n envs; rollout_step(): frames t .. t + k - 1 of every env in ONE launch on s --
    // render record j (the state BEFORE frame j) into the chunk's record buffer of parity q, step record j into packed + j * stride,
    // the last frame's outputs into tbx_engine::reward / ...; rollout_render(): the rasteriser of record j of parity q into out.
    virtual bool rollout_ok(int /*channels*/) const { return false; }
    virtual bool rollout_auto(int /*n*/, int /*gather_kind*/) const { return false; }
    virtual int rollout_step(tbx_engine*, const ActionSource&, uint32_t /*flags*/, int /*k*/, int /*q*/, uint64_t* /*packed*/, size_t /*stride*/, hipStream_t) { return TBX_E_UNSUPPORTED; }
    virtual int rollout_render(tbx_engine*, uint8_t* /*out*/, int /*channels*/, int /*q*/, int /*j*/, hipStream_t) { return TBX_E_UNSUPPORTED; }
    // rollout_render_span(): records j0 .. j0 + count - 1 of parity q in ONE rasteriser launch (they lie one behind the other, and so do
    // their frames: count x n "envs" to the rasteriser; behind_rasteriser: another rasteriser launch is still running in front of it on
    // s, so its first waves start against draining stores -- raster.hpp); rollout_span_auto(): the engine's choice between one such
    // launch per chunk on one internal stream and a launch per frame on two
    virtual bool rollout_span_ok() const { return false; }
    virtual bool rollout_span_auto(int /*n*/, int /*gather_kind*/) const { return false; }
    virtual int rollout_render_span(tbx_engine*, uint8_t* /*out*/, int /*channels*/, int /*q*/, int /*j0*/, int /*count*/, bool /*behind_rasteriser*/, hipStream_t) { return TBX_E_UNSUPPORTED; }
    // batched interventions (include/toybox_amd.h, tbx_edit / tbx_reduce): one kernel over the selected envs
    virtual int edit(tbx_engine* e, int /*op*/, const TbxEditArgs&, const uint8_t* /*mask_dev*/, hipStream_t) { return e->fail(TBX_E_INVALID, "this game has no such edit"); }
    virtual int reduce(tbx_engine* e, int /*query*/, const TbxEditArgs&, double* /*out_dev*/, int /*width*/, hipStream_t) { return e->fail(TBX_E_INVALID, "this game has no such query"); }
    // TBX_QUERY_LOOKAHEAD .. _TREE: the play kernel of l.query with the game's leaf policy (tbx_launch_planner) over the units of
    // envs [l.first_env, l.first_env + l.envs); the arguments' shared values are already checked (engine.hip).  search_lanes(): the
    // lanes one unit takes in the form the engine is in (64 or 1)
    virtual int lookahead_play(tbx_engine* e, const TbxEditArgs&, const TbxPlanLaunch&, hipStream_t) { return e->fail(TBX_E_UNSUPPORTED, "this game has no lookahead"); }
    virtual int search_lanes() const { return 64; }
    // TBX_EDIT_COPY_ENV, TBX_EDIT_CHECKPOINT_*: every per-env array that decides the env's future outputs -- the game state, its
    // device-only mirrors and (once tbx_agent_init has made them) MaxAndSkipEnv's two buffer slots -- appended to the plan.  The
    // engine adds sim_rng, prev_score and the agent layer and runs the copy.  Listing changes nothing; a copy that WROTE live
    // envs (a fork, a restore -- not a save) says so with envs_rewritten(): step-written render records no longer describe the state.
    virtual void list_envs(tbx_engine* e, TbxEnvPlan& plan) = 0;
    virtual void envs_rewritten(tbx_engine*) {}
    // an engine option changed (tbx_set_option): pick it up
    virtual void options_changed(tbx_engine*) {}
    // generic path: full-resolution gray frames of slot A (source 1), slot B (2) or the live state (0); envs whose
    // pick_live byte is non-zero are painted from the live state instead
    virtual int render_from(tbx_engine*, int /*source*/, const uint8_t* /*pick_live*/, uint8_t* /*out_dev*/, int /*channels*/, hipStream_t) { return TBX_E_UNSUPPORTED; }
    // the reset path of the wrapper stack, run in-kernel for the envs flagged in AgentResetArgs::kind
    virtual bool agent_reset_supported() const { return false; }
    virtual int agent_reset_envs(tbx_engine*, const struct AgentResetArgs&, hipStream_t) { return TBX_E_UNSUPPORTED; }
};

void tbx_agent_free(tbx_engine* e);
void tbx_gather_free(tbx_engine* e);
hipError_t tbx_gather_before_step(tbx_engine* e, hipStream_t s);   // a step must not overwrite records a queued gather still reads
void tbx_set_out_parity(tbx_engine* e, int p);                    // engine.hip: which TbxStepOut set the next step writes
void tbx_set_create_error(const std::string& msg);                 // text behind tbx_last_error(NULL)
int tbx_gather_buffer(tbx_engine* e, void** out_ptr, size_t* out_bytes);
// gather.hip, for tbx_rollout_synthetic over a K-step ring: the ring the next K steps fill (stream s is made to wait for the collective
// that last read it) and, once ONE launch has filled it, the collective behind that launch's event
int tbx_gather_ring_open(tbx_engine* e, hipStream_t s, int k, uint64_t** base, size_t* stride);
int tbx_gather_ring_filled(tbx_engine* e, hipEvent_t filled_ev);
GameOps* tbx_make_breakout_ops();
GameOps* tbx_make_si_ops();
GameOps* tbx_make_amidar_ops();
GameOps* tbx_make_gridworld_ops();
