// envcopy.hip -- what an env is made of and how it is moved: TBX_EDIT_COPY_ENV (fork), TBX_EDIT_CHECKPOINT_SLOTS / _SAVE /
// _RESTORE and TBX_QUERY_CHECKPOINT_VALID (include/toybox_amd.h).
//
// The per-env state is a list of arrays [fields][N][row_bytes] (TbxEnvSeg; env_plan() lists them).  A row of an array lies in
// one of two kinds of PLACE:
//   live       the engine's own array seg.base, planes as they lie;
//   packed(p)  a packed copy of all arrays at base pointer p -- the fork's scratch, or one slot plane of the checkpoint store:
//              every array at its 256-byte-aligned offset packed_off, planes in LOGICAL order (plane c of the packed copy is
//              live plane (rot + c) % fields: the plane ring's head is batch-wide and has usually moved between a save and the
//              restore; it does not move between the two passes of a fork).
// A copy is a ROUTE: per destination env, whether it is selected and the (place, row) it comes from and goes to.
//   fork, one pass   live[src]          -> live[i]            (the host form has seen that no selected destination is a source)
//   fork gather      live[src]          -> packed(scratch)[i]
//   fork scatter     packed(scratch)[i] -> live[i]            (behind the gather in stream order: simultaneous assignment)
//   save             live[i]            -> packed(slot)[i]
//   restore          packed(slot)[row]  -> live[i]
// Two kernels carry out any route: scalars (rows of 1 .. 8 bytes, one THREAD per env walks every plane of every such array --
// the stores of a wave are coalesced) and rows (anything wider, one WAVE per env row, 16 bytes per lane: the 28 KB observation
// stack is where the bytes are).  A third rewrites the RNG words of the envs a route wrote (`salt`).
// The checkpoint store is `slots` packed copies; behind them valid[slots][N], then the two words the host forms' check writes.

#include "engine_host.hpp"
#include "envcopy.hpp"

#include <algorithm>
#include <new>

struct CkptStore {
    uint8_t* planes;
    uint8_t* valid;               // [slots][N]
    uint64_t slot_bytes;
    int slots;
};
struct TbxEnvCopy {
    TbxDevBuf<uint8_t> scratch;    // the gathered rows between the two passes of a fork
    TbxDevBuf<uint8_t> store;      // the checkpoint store ...
    CkptStore st{};                // ... as the kernels see it (no store: zeros)
    std::vector<std::pair<uint32_t, uint32_t>> sig;   // {fields, row_bytes} of the arrays the store was made for, in plan order
};

constexpr int FORK_SEGS = 16;                 // arrays per launch
constexpr unsigned FORK_MAX_BLOCKS = 2048;    // rows kernel: the grid is capped and strides over the rest
struct EnvBatch {
    TbxEnvSeg seg[FORK_SEGS];
    int n_segs;
};

// what a route says about one selected env: where its rows come from and go to (the packed base of a live place is not read),
// and a byte to set once the env has arrived (nullptr: none; the first scalars launch of a copy does)
struct EnvMove {
    uint8_t* from_p;
    uint8_t* to_p;
    size_t from, to;
    uint8_t* note;
};

// plane c (in logical order) of array g at a place
template <bool PACKED>
__device__ __forceinline__ uint8_t* place_plane(const TbxEnvSeg& g, uint8_t* p, uint32_t c, size_t plane)
{
    if (PACKED) return p + g.packed_off + c * plane;
    uint32_t f = g.rot + c;
    if (f >= g.fields) f -= g.fields;
    return g.base + f * plane;
}
template <bool PACKED>
__device__ __forceinline__ uint8_t* place_base(const TbxEnvSeg& g, uint8_t* p) { return PACKED ? p + g.packed_off : g.base; }

// ---- the routes

// args {src[, salt]}; <false, false> one pass, <false, true> gather, <true, false> scatter.  Not selected: a masked env, a source
// outside the batch (the device form leaves such an env untouched) and, unless self_counts (the salt pass does), the env itself
template <bool FROM_PACKED, bool TO_PACKED>
struct ForkRoute {
    static constexpr bool from_packed = FROM_PACKED, to_packed = TO_PACKED, notes = false;
    TbxEditArgs a;
    const uint8_t* mask;
    uint8_t* scratch;
    bool self_counts;
    __device__ __forceinline__ bool move(int i, int n, EnvMove& m) const
    {
        if (mask && !mask[i]) return false;
        const int src = a.geti(i, 0);
        if (src < 0 || src >= n || (!self_counts && src == i)) return false;
        m = EnvMove{scratch, scratch, FROM_PACKED ? (size_t)i : (size_t)src, (size_t)i, nullptr};
        return true;
    }
};

constexpr int CKPT_BAD_SLOT = 1, CKPT_BAD_ROW = 2, CKPT_EMPTY = 3;

// the cell of selected env i: -> slot (row in `row`), -1 not selected, or -(1 + CKPT_*) for a row the op cannot carry out
template <bool SAVE>
__device__ __forceinline__ int ckpt_cell(const CkptStore& st, const TbxEditArgs& a, const uint8_t* mask, int i, int n, int& row)
{
    if (mask && !mask[i]) return -1;
    const int slot = a.geti(i, 0);
    if (slot < 0 || slot >= st.slots) return -(1 + CKPT_BAD_SLOT);
    row = i;
    if (!SAVE) {
        const int r = a.n >= 2 ? a.geti(i, 1) : -1;
        if (r != -1) row = r;
        if (row < 0 || row >= n) return -(1 + CKPT_BAD_ROW);
        if (!st.valid[(size_t)slot * n + row]) return -(1 + CKPT_EMPTY);
    }
    return slot;
}

// args {slot} (save) / {slot[, row[, salt]]} (restore); a saved cell's valid byte is the one to set on arrival
template <bool SAVE>
struct CkptRoute {
    static constexpr bool from_packed = !SAVE, to_packed = SAVE, notes = SAVE;
    TbxEditArgs a;
    const uint8_t* mask;
    CkptStore st;
    __device__ __forceinline__ bool move(int i, int n, EnvMove& m) const
    {
        int row;
        const int slot = ckpt_cell<SAVE>(st, a, mask, i, n, row);
        if (slot < 0) return false;
        uint8_t* cell = st.planes + (size_t)slot * st.slot_bytes;
        m = EnvMove{cell, cell, SAVE ? (size_t)i : (size_t)row, SAVE ? (size_t)row : (size_t)i, SAVE ? st.valid + (size_t)slot * n + row : nullptr};
        return true;
    }
};

// ---- the kernels

// one row of rb bytes by one wave: 16 bytes per lane where row length and both arrays allow it (align 16), else 4, else 1
__device__ __forceinline__ uint32_t row_align(uint32_t rb, const uint8_t* rd0, const uint8_t* wr0)
{
    const uint32_t bits = rb | (uint32_t)(uintptr_t)rd0 | (uint32_t)(uintptr_t)wr0;
    return (bits & 15u) == 0 ? 16u : (bits & 3u) == 0 ? 4u : 1u;
}
__device__ __forceinline__ void copy_row(const uint8_t* rd, uint8_t* wr, uint32_t rb, int lane, uint32_t align)
{
    if (align == 16u) {
        uint32_t o = (uint32_t)lane * 16u;
        for (; o + 3072u < rb; o += 4096u) {     // four 16-byte loads in flight per lane, then their stores
            const uint4 v0 = *reinterpret_cast<const uint4*>(rd + o), v1 = *reinterpret_cast<const uint4*>(rd + o + 1024u);
            const uint4 v2 = *reinterpret_cast<const uint4*>(rd + o + 2048u), v3 = *reinterpret_cast<const uint4*>(rd + o + 3072u);
            *reinterpret_cast<uint4*>(wr + o) = v0; *reinterpret_cast<uint4*>(wr + o + 1024u) = v1;
            *reinterpret_cast<uint4*>(wr + o + 2048u) = v2; *reinterpret_cast<uint4*>(wr + o + 3072u) = v3;
        }
        for (; o < rb; o += 1024u) *reinterpret_cast<uint4*>(wr + o) = *reinterpret_cast<const uint4*>(rd + o);
    } else if (align == 4u) {
        for (uint32_t o = (uint32_t)lane * 4u; o < rb; o += 256u) *reinterpret_cast<uint32_t*>(wr + o) = *reinterpret_cast<const uint32_t*>(rd + o);
    } else {
        for (uint32_t o = (uint32_t)lane; o < rb; o += 64u) wr[o] = rd[o];
    }
}
// ... and one scalar row (1 .. 8 bytes) by one thread: element `from` of plane rd -> element `to` of plane wr
__device__ __forceinline__ void copy_scalar(const uint8_t* rd, uint8_t* wr, uint32_t rb, size_t from, size_t to)
{
    switch (rb) {
    case 8: reinterpret_cast<uint64_t*>(wr)[to] = reinterpret_cast<const uint64_t*>(rd)[from]; break;
    case 4: reinterpret_cast<uint32_t*>(wr)[to] = reinterpret_cast<const uint32_t*>(rd)[from]; break;
    case 2: reinterpret_cast<uint16_t*>(wr)[to] = reinterpret_cast<const uint16_t*>(rd)[from]; break;
    default:
        for (uint32_t o = 0; o < rb; o++) wr[to * rb + o] = rd[from * rb + o];
    }
}

template <class ROUTE>
__global__ __launch_bounds__(256) void env_scalars_kernel(EnvBatch b, ROUTE r, int n, int first)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    EnvMove m;
    if (!r.move(i, n, m)) return;
    for (int k = 0; k < b.n_segs; k++) {
        const TbxEnvSeg& g = b.seg[k];
        if (g.row_bytes > 8) continue;
        const size_t plane = (size_t)n * g.row_bytes;
        for (uint32_t c = 0; c < g.fields; c++)
            copy_scalar(place_plane<ROUTE::from_packed>(g, m.from_p, c, plane), place_plane<ROUTE::to_packed>(g, m.to_p, c, plane), g.row_bytes, m.from, m.to);
    }
    if (ROUTE::notes && first) *m.note = 1;
}

template <class ROUTE>
__global__ __launch_bounds__(TBX_BLOCK) void env_rows_kernel(EnvBatch b, ROUTE r, int n)
{
    const int lane = threadIdx.x & 63;
    const int wave0 = wave_uniform((int)(blockIdx.x * TBX_WAVES_PER_BLOCK + (threadIdx.x >> 6)));
    const int n_waves = (int)(gridDim.x * TBX_WAVES_PER_BLOCK);
    for (int i = wave0; i < n; i += n_waves) {               // destination envs, several in flight per block
        EnvMove m;
        if (!r.move(i, n, m)) continue;
        for (int k = 0; k < b.n_segs; k++) {
            const TbxEnvSeg& g = b.seg[k];
            if (g.row_bytes <= 8) continue;
            const uint32_t rb = g.row_bytes;
            const size_t plane = (size_t)n * rb;
            const uint32_t align = row_align(rb, place_base<ROUTE::from_packed>(g, m.from_p), place_base<ROUTE::to_packed>(g, m.to_p));
            for (uint32_t c = 0; c < g.fields; c++)
                copy_row(place_plane<ROUTE::from_packed>(g, m.from_p, c, plane) + m.from * rb, place_plane<ROUTE::to_packed>(g, m.to_p, c, plane) + m.to * rb, rb, lane, align);
        }
    }
}

// `salt` (argument salt_arg of the route's rows), behind the copy in stream order: every RNG word of an env the route wrote
// becomes splitmix64(word ^ salt) in the listed live arrays
template <class ROUTE>
__global__ __launch_bounds__(256) void env_salt_kernel(EnvBatch b, ROUTE r, int n, int salt_arg)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    EnvMove m;
    if (i >= n || !r.move(i, n, m)) return;
    const uint64_t salt = r.a.getu(i, salt_arg);
    if (!salt) return;
    for (int k = 0; k < b.n_segs; k++) {
        const TbxEnvSeg& g = b.seg[k];
        for (uint32_t f = 0; f < g.fields; f++) {
            uint64_t* w = reinterpret_cast<uint64_t*>(g.base + ((size_t)f * n + (size_t)i) * g.row_bytes + g.rng_off);
            for (uint32_t j = 0; j < g.rng_words; j++) w[j] = tbx_splitmix64(w[j] ^ salt);
        }
    }
}

// the host forms' check: word 0 = min over the rows that cannot be carried out of (env << 2 | CKPT_*), word 1 = their number - 1
// (both start as all ones)
template <bool SAVE>
__global__ __launch_bounds__(256) void ckpt_check_kernel(CkptStore st, uint32_t* words, TbxEditArgs a, const uint8_t* __restrict__ mask, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int row;
    const int c = ckpt_cell<SAVE>(st, a, mask, i, n, row);
    if (c >= -1) return;
    atomicMin(&words[0], ((uint32_t)i << 2) | (uint32_t)(-c - 1));
    atomicAdd(&words[1], 1u);
}

__global__ __launch_bounds__(256) void ckpt_valid_kernel(CkptStore st, TbxEditArgs a, double* __restrict__ out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int slot = a.n >= 1 ? a.geti(i, 0) : -1;
    int row = a.n >= 2 ? a.geti(i, 1) : -1;
    if (row == -1) row = i;
    out[i] = (!st.valid || slot < 0 || slot >= st.slots || row < 0 || row >= n) ? -1.0 : st.valid[(size_t)slot * n + row] ? 1.0 : 0.0;
}

// ---- the plan and the launcher

// Every per-env array of the engine as it is now, each with its offset in a packed copy of them all (256-byte-aligned, so a row
// copy that can take 16 bytes per lane still can); -> that copy's size.  Listing changes nothing in the engine.
static size_t env_plan(tbx_engine* e, TbxEnvPlan& plan)
{
    e->ops->list_envs(e, plan);
    plan.soa(e->sim_rng, 2, 1);
    plan.soa(e->prev_score, 1);
    tbx_agent_copy_envs(e, plan);
    size_t bytes = 0;
    for (TbxEnvSeg& g : plan.segs) {
        g.packed_off = bytes;
        bytes += ((size_t)g.fields * (size_t)e->n * g.row_bytes + 255) & ~(size_t)255;
    }
    return bytes;
}

static std::vector<std::pair<uint32_t, uint32_t>> plan_signature(const TbxEnvPlan& plan)
{
    std::vector<std::pair<uint32_t, uint32_t>> sig;
    for (const TbxEnvSeg& g : plan.segs) sig.emplace_back(g.fields, g.row_bytes);
    return sig;
}

// The plan in batches of FORK_SEGS arrays: launch(batch, it has scalar rows, wider rows, RNG words, the thread-per-env grid, the
// wave-per-env grid) queues what the batch needs
template <class LAUNCH>
static int each_batch(tbx_engine* e, const TbxEnvPlan& plan, LAUNCH&& launch)
{
    const size_t N = (size_t)e->n;
    const dim3 sgrid((unsigned)((N + 255) / 256));
    const dim3 rgrid(std::min((unsigned)((N + TBX_WAVES_PER_BLOCK - 1) / TBX_WAVES_PER_BLOCK), FORK_MAX_BLOCKS));
    for (size_t k0 = 0; k0 < plan.segs.size(); k0 += FORK_SEGS) {
        EnvBatch b;
        b.n_segs = 0;
        bool sc = false, rw = false, rng = false;
        for (size_t k = k0; k < plan.segs.size() && k < k0 + FORK_SEGS; k++) {
            const TbxEnvSeg& g = b.seg[b.n_segs++] = plan.segs[k];
            (g.row_bytes <= 8 ? sc : rw) = true;
            rng |= g.rng_words != 0;
        }
        launch(b, sc, rw, rng, sgrid, rgrid);
    }
    EHIP(hipGetLastError());
    return TBX_OK;
}

template <class ROUTE>
static int copy_envs(tbx_engine* e, const TbxEnvPlan& plan, const ROUTE& r, hipStream_t s)
{
    int first = 1;
    return each_batch(e, plan, [&](const EnvBatch& b, bool sc, bool rw, bool, dim3 sgrid, dim3 rgrid) {
        if (sc || (ROUTE::notes && first)) {                   // (the first launch of a route with a byte to set is a scalars launch)
            hipLaunchKernelGGL(env_scalars_kernel<ROUTE>, sgrid, dim3(256), 0, s, b, r, e->n, first);
            first = 0;
        }
        if (rw) hipLaunchKernelGGL(env_rows_kernel<ROUTE>, rgrid, dim3(TBX_BLOCK), 0, s, b, r, e->n);
    });
}

template <class ROUTE>
static int salt_envs(tbx_engine* e, const TbxEnvPlan& plan, const ROUTE& r, int salt_arg, hipStream_t s)
{
    return each_batch(e, plan, [&](const EnvBatch& b, bool, bool, bool rng, dim3 sgrid, dim3) {
        if (rng) hipLaunchKernelGGL(env_salt_kernel<ROUTE>, sgrid, dim3(256), 0, s, b, r, e->n, salt_arg);
    });
}

static TbxEnvCopy* state(tbx_engine* e)
{
    if (!e->envcopy) e->envcopy = new (std::nothrow) TbxEnvCopy();
    return e->envcopy;
}

static CkptStore ckpt_view(const tbx_engine* e) { return e->envcopy ? e->envcopy->st : CkptStore{}; }

// SAVE / RESTORE on stream s.  check: the host form -- rows that cannot be carried out are an error, and nothing is changed
template <bool SAVE>
static int checkpoint_move(tbx_engine* e, const TbxEditArgs& a, const uint8_t* mask_dev, bool check, hipStream_t s)
{
    const std::string name = SAVE ? "TBX_EDIT_CHECKPOINT_SAVE" : "TBX_EDIT_CHECKPOINT_RESTORE";
    if (a.n < 1 || a.n > (SAVE ? 1 : 3)) return e->fail(TBX_E_INVALID, name + (SAVE ? " takes {slot}" : " takes {slot[, row[, salt]]}"));
    const CkptStore st = ckpt_view(e);
    if (!st.slots) return e->fail(TBX_E_INVALID, name + ": env 0: there is no checkpoint store (TBX_EDIT_CHECKPOINT_SLOTS makes one)");
    TbxEnvPlan plan;
    env_plan(e, plan);
    if (plan_signature(plan) != e->envcopy->sig)
        return e->fail(TBX_E_UNSUPPORTED, name + ": the engine's per-env arrays are no longer the ones the checkpoint store was made for; TBX_EDIT_CHECKPOINT_SLOTS makes a new store");
    if (check) {
        uint32_t* words = reinterpret_cast<uint32_t*>(st.valid + (((size_t)st.slots * (size_t)e->n + 7) & ~(size_t)7));
        uint32_t got[2];
        EHIP(hipMemsetAsync(words, 0xFF, sizeof got, s));
        hipLaunchKernelGGL(ckpt_check_kernel<SAVE>, dim3((e->n + 255) / 256), dim3(256), 0, s, st, words, a, mask_dev, e->n);
        EHIP(hipGetLastError());
        EHIP(hipMemcpyAsync(got, words, sizeof got, hipMemcpyDeviceToHost, s));
        EHIP(hipStreamSynchronize(s));
        if (got[0] != 0xFFFFFFFFu) {
            const int why = (int)(got[0] & 3u);
            const std::string what = why == CKPT_BAD_SLOT ? "names a slot outside 0 .. " + std::to_string(st.slots - 1)
                                   : why == CKPT_BAD_ROW ? "names a row outside 0 .. " + std::to_string(e->n - 1) : "names an empty cell";
            return e->fail(TBX_E_INVALID, name + ": env " + std::to_string(got[0] >> 2) + " " + what + " (" + std::to_string(got[1] + 1u) + " such envs; nothing was changed)");
        }
    }
    if (!SAVE) e->ops->envs_rewritten(e);
    const CkptRoute<SAVE> route{a, mask_dev, st};
    int rc = copy_envs(e, plan, route, s);
    if constexpr (!SAVE)
        if (!rc && a.n >= 3) rc = salt_envs(e, plan, route, 2, s);
    return rc;
}

// direct: one pass (the caller has checked that no selected destination is a selected row's source)
int fork_envs(tbx_engine* e, const TbxEditArgs& a, const uint8_t* mask_dev, bool direct, hipStream_t s)
{
    if (a.n < 1) return e->fail(TBX_E_INVALID, "TBX_EDIT_COPY_ENV takes {src[, salt]}");
    TbxEnvPlan plan;
    const size_t packed = env_plan(e, plan);
    e->ops->envs_rewritten(e);
    uint8_t* scratch = nullptr;
    if (!direct) {
        if (!state(e)) return e->fail(TBX_E_NOMEM, "out of host memory");
        EHIP(e->envcopy->scratch.reserve(packed));             // (freeing the old one waits for whatever still reads it)
        scratch = e->envcopy->scratch.p;
    }
    int rc = direct ? copy_envs(e, plan, ForkRoute<false, false>{a, mask_dev, nullptr, false}, s)
                    : copy_envs(e, plan, ForkRoute<false, true>{a, mask_dev, scratch, false}, s);
    if (!rc && !direct) rc = copy_envs(e, plan, ForkRoute<true, false>{a, mask_dev, scratch, false}, s);
    if (!rc && a.n >= 2) rc = salt_envs(e, plan, ForkRoute<false, false>{a, mask_dev, nullptr, true}, 1, s);
    return rc;
}

// the host form sees the rows: a selected row with a source outside the batch is an error (nothing has been changed), and the
// one-pass copy is safe when no selected destination (other than a copy of itself) is the source of another selected row
int fork_check_host(tbx_engine* e, const double* args, int n_args, int per_env, const uint8_t* mask_host, bool& direct)
{
    if (n_args < 1 || !args) return e->fail(TBX_E_INVALID, "TBX_EDIT_COPY_ENV takes {src[, salt]}");
    const int n = e->n;
    auto source = [&](int i) { return TbxEditArgs::to_int(args[per_env ? (size_t)i * n_args : 0]); };
    std::vector<uint8_t> is_source((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        if (mask_host && !mask_host[i]) continue;
        const int src = source(i);
        if (src < 0 || src >= n)
            return e->fail(TBX_E_INVALID, "TBX_EDIT_COPY_ENV: env " + std::to_string(i) + " names source " + std::to_string(src) + ", outside 0 .. " + std::to_string(n - 1));
        if (src != i) is_source[(size_t)src] = 1;
    }
    direct = true;
    for (int i = 0; i < n && direct; i++)
        if ((!mask_host || mask_host[i]) && source(i) != i && is_source[(size_t)i]) direct = false;
    return TBX_OK;
}

// TBX_EDIT_CHECKPOINT_SLOTS: the stream has been drained by the caller
int checkpoint_slots(tbx_engine* e, const double* args, int n_args, int per_env, const uint8_t* mask_host)
{
    if (n_args != 1 || !args || per_env || mask_host || !(args[0] >= 0.0 && args[0] <= 1048576.0) || args[0] != (double)(int)args[0])
        return e->fail(TBX_E_INVALID, "TBX_EDIT_CHECKPOINT_SLOTS takes {slots} (an integer >= 0), the same for every env and without a mask");
    if (!state(e)) return e->fail(TBX_E_NOMEM, "out of host memory");
    TbxEnvCopy& c = *e->envcopy;
    c.store.release();
    c.st = CkptStore{};
    c.sig.clear();
    const int slots = (int)args[0];
    if (!slots) return TBX_OK;
    TbxEnvPlan plan;
    const size_t slot_bytes = env_plan(e, plan);
    const size_t valid_bytes = ((size_t)slots * (size_t)e->n + 7) & ~(size_t)7;
    const size_t total = (size_t)slots * slot_bytes + valid_bytes + 2 * sizeof(uint32_t);
    if (c.store.reserve(total) != hipSuccess) {
        (void)hipGetLastError();
        return e->fail(TBX_E_NOMEM, "TBX_EDIT_CHECKPOINT_SLOTS: no device memory for " + std::to_string(slots) + " slots of " + std::to_string(slot_bytes) + " bytes");
    }
    c.st = CkptStore{c.store.p, c.store.p + (size_t)slots * slot_bytes, slot_bytes, slots};
    c.sig = plan_signature(plan);
    EHIP(hipMemsetAsync(c.st.valid, 0, valid_bytes, e->stream));
    EHIP(hipStreamSynchronize(e->stream));
    return TBX_OK;
}

int checkpoint_copy(tbx_engine* e, bool save, const TbxEditArgs& a, const uint8_t* mask_dev, bool check, hipStream_t s)
{
    return save ? checkpoint_move<true>(e, a, mask_dev, check, s) : checkpoint_move<false>(e, a, mask_dev, check, s);
}

int checkpoint_valid(tbx_engine* e, const TbxEditArgs& a, double* out_dev, hipStream_t s)
{
    if (a.n < 1 || a.n > 2) return e->fail(TBX_E_INVALID, "TBX_QUERY_CHECKPOINT_VALID takes {slot[, row]}");
    hipLaunchKernelGGL(ckpt_valid_kernel, dim3((e->n + 255) / 256), dim3(256), 0, s, ckpt_view(e), a, out_dev, e->n);
    EHIP(hipGetLastError());
    return TBX_OK;
}

void envcopy_free(tbx_engine* e)
{
    if (e->envcopy) { e->envcopy->scratch.release(); e->envcopy->store.release(); }
    delete e->envcopy;
    e->envcopy = nullptr;
}
