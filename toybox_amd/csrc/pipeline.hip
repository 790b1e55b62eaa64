// pipeline.hip -- the pipelined step / render mode (TBX_OPT_PIPELINE) and the overlapped loop forms on top of it: overlapped fused
// launches (TBX_OPT_FUSED_OVERLAP) and rollout chunks (tbx_rollout_synthetic).  Host-side orchestration on internal streams; the one
// kernel here waits for a device counter.

#include "pipeline.hpp"
#include "engine_host.hpp"

#include <algorithm>
#include <cstdlib>
#include <new>

namespace {

// the form the calls since the pipeline was entered take: they keep different books on the same lanes (pipe_enter joins before it changes)
enum PipeKind { PIPE_NONE = 0, PIPE_STEPS_AND_RENDERS, PIPE_FUSED_OVERLAP, PIPE_ROLLOUT_CHUNKS };

// Pipelined mode (TBX_OPT_PIPELINE): random-rollout steps and batch renders of engines whose rasteriser reads
// step-written records run on internal streams, over double-buffered records, step outputs and frames.
struct StepRenderBooks {
    hipStream_t step_on = nullptr;                   // the last pipelined step ran on this stream ...
    hipStream_t step_user = nullptr;                 // ... and this caller's stream has been made to wait for it (compared, never used)
    hipStream_t render_on[2] = {nullptr, nullptr};   // the last render that READ records buffer p ran on this stream
    bool render_pending[2] = {false, false};
    bool user_frame_rec[2] = {false, false};
    bool step_outstanding = false;
    int live_reader = -1;         // >= 0: the render behind render_ev[live_reader] read LIVE state (records were not valid): the next step waits for it
    int frame_par = -1;           // frame buffer the last overlapped render wrote (-1: none since the pipeline was entered)
};

// Overlapped fused launches (TBX_OPT_FUSED_OVERLAP; fused_overlapped): consecutive tbx_render_step_synthetic
// launches alternate between the two lanes, the two output sets and the two frame buffers, and launch N+1 is ordered behind
// the STEP BLOCKS of launch N only -- a device counter they bump when their state, records and outputs are written, waited
// for by a one-wave kernel in front of launch N+1 (tbx_ticket_wait_kernel) -- not behind its rasteriser blocks.
struct FusedBooks {
    bool launch_rec[2] = {false, false};
    bool prev_overlapped = false;                    // the call before this one was an overlapped launch (else stream order holds)
    // The caller's stream joins LAZILY in this mode: it is made to wait for the launch that wrote a result when the caller asks
    // for the result's address (tbx_device_buffer -- required after every call, the addresses alternate) or makes a call of any
    // other kind.  A loop that only rolls queues nothing on the caller's stream: with a record gather on the device, a wait and
    // a fence per call on that stream turned a gain of 4-25 % into a loss of 10-100 % (profiles/r06_experiments.txt).
    bool user_waits[2] = {false, false};             // the caller's stream has been made to wait for launch_ev[k]
};

// Rollout chunks (tbx_rollout_synthetic; rollout_chunked): k frames per call.  ONE step launch on the step lane
// writes the k render records, the k step records and the state; the rasteriser launches (k, alternating between the two lanes, or
// one over the chunk's k x N frames on lane 0) depend on that step launch alone -- and the step launch of chunk c+1 runs beside them, a whole chunk ahead of its own
// rasterisers: no launch waits for a step that runs beside a rasteriser (what kept overlapped fused launches unstable).
struct ChunkBooks {
    bool step_rec[2] = {false, false}, raster_rec[2][2] = {{false, false}, {false, false}};
    bool user_waits[2] = {false, false};             // the caller's stream has been made to wait for chunk q (lazy join)
};

// what pipe_enter resets: everything the calls of one stay in the pipeline remember about each other
struct PipeBooks {
    PipeKind kind = PIPE_NONE;
    bool user_step_rec[2] = {false, false};          // (every form: TbxPipe::user_step_ev)
    bool reader_seen = false;                        // an address was handed out since the last call: the next call fences the caller's stream
    StepRenderBooks sr;
    FusedBooks fused;
    ChunkBooks chunk;
};

}  // namespace

// the resources, made once by pipe_prepare and kept until tbx_destroy, and the books
struct TbxPipe {
    hipStream_t lane[2] = {nullptr, nullptr};        // value 2: lane[0] is the step stream; value 3: step N and render N on lane[parity]
    hipStream_t step_lane = nullptr;
    hipEvent_t step_ev = nullptr;                    // behind the last pipelined step
    hipEvent_t render_ev[2] = {nullptr, nullptr};    // behind the last render that READ records buffer p
    // reader fences on the caller's stream: everything the caller had queued there when the step (render) call that
    // superseded buffer p's content was made -- the next writer of buffer p waits for it
    hipEvent_t user_step_ev[2] = {nullptr, nullptr}, user_frame_ev[2] = {nullptr, nullptr};
    hipEvent_t launch_ev[2] = {nullptr, nullptr};    // completion event of the last fused launch on lane k (it rides on the launch)
    hipEvent_t chunk_step_ev[2] = {nullptr, nullptr};        // behind the step launch of the last chunk of parity q
    hipEvent_t chunk_raster_ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [q][lane]: behind that chunk's last rasteriser launch on the lane
    unsigned long long* arrive = nullptr;            // device [2]: step blocks of overlapped launches that have finished, ever; launches
                                                     // whose RELEASE block has started (the block `lead` blocks before the end of the grid)
    unsigned long long arrive_want = 0;              // host: what the launches issued so far add up to
    unsigned long long release_want = 0;
    TbxDevBuf<uint8_t> frame[2];
    bool prepared = false;        // every resource above exists (set last by pipe_prepare)
    PipeBooks books;
};

// the one place that says which form is running
static PipeKind pipe_kind(const tbx_engine* e) { return e->pipe_active ? e->pipe->books.kind : PIPE_NONE; }

// ---- pipelined mode (TBX_OPT_PIPELINE; contract in include/toybox_amd.h)
//
// A step with in-kernel actions depends on nothing the previous frame's rasteriser produces, and for games whose rasteriser
// reads step-written records (GameOps::pipeline_ok) it disturbs nothing that rasteriser reads once there are two buffers of
// records and of step outputs: it runs on the engine's step stream BESIDE the render queued before it.  Measured on MI355X
// (scripts/interleave_probe.py): a 10 us step kernel serialised between two 1.19 ms Breakout render launches costs
// 0.04-0.22 ms depending on the box, run beside the render it costs 0.01-0.04 ms.  With value 3 consecutive renders into the
// engine-owned frame buffer alternate between two internal streams and two buffers as well, so that launch N+1 ramps up in
// the ramp-down of launch N.
//
// Streams.  Value 2: one internal step stream; renders stay on the caller's stream U.  Value 3: two internal streams S[0],
// S[1]; step N and the overlapped render N both go to S[p], p = the parity of the buffers step N writes -- so render N is
// behind its step, behind render N-2 (same frame buffer) and behind step N-2 / render N-2's reads of records p by stream order
// alone, and runs beside render N-1 on the other stream.  (Few streams on purpose: the runtime multiplexes streams onto a
// handful of hardware queues -- GPU_MAX_HW_QUEUES, 4 by default -- and two streams that share one queue do not overlap.)
//
// Who waits for whom beyond stream order (U = the stream the caller names):
//   step N   (writes records / outputs p)   <- step N-1 (the state; other stream in value 3), a render of records p that ran
//                                              elsewhere, U's readers of outputs p (fence recorded on U at step N-1's call),
//                                              the gather that read outputs p
//   render N on U (value 2, or out_dev given) <- nothing: U waits for every step
//   render N on S[p] (value 3)              <- U's readers of frame buffer p (fence recorded on U at render N-1's call)
//   U                                        <- every step and every overlapped render (so whatever the caller queues next
//                                              sees them, and U is the tail that calls of any other kind join)
int pipe_mode(const tbx_engine* e)
{
    const int v = e->opt[TBX_OPT_PIPELINE];
    if (v == 0 || e->gather_ring || !e->ops->pipeline_ok()) return 0;      // (the K-step record ring moves the one record pointer)
    if (v == 1) return e->ops->pipeline_auto(e->n, e->gather != nullptr);
    return v;
}

static int pipe_prepare(tbx_engine* e)
{
    if (!e->pipe && !(e->pipe = new (std::nothrow) TbxPipe())) return e->fail(TBX_E_NOMEM, "out of host memory");
    TbxPipe& p = *e->pipe;
    if (p.prepared) return TBX_OK;
    // every resource is made only while it is still missing, so that a call that failed half way can be repeated without
    // leaking what the first attempt got; `prepared` is set last
    const size_t N = (size_t)e->n;
    TbxStepOut& o = e->outs[1];
    if (!o.reward) { EHIP(hipMalloc((void**)&o.reward, N * sizeof(int32_t))); EHIP(hipMemset(o.reward, 0, N * sizeof(int32_t))); }
    if (!o.done) { EHIP(hipMalloc((void**)&o.done, N)); EHIP(hipMemset(o.done, 0, N)); }
    if (!o.lives) { EHIP(hipMalloc((void**)&o.lives, N * sizeof(int32_t))); EHIP(hipMemset(o.lives, 0, N * sizeof(int32_t))); }
    if (!o.score) { EHIP(hipMalloc((void**)&o.score, N * sizeof(int32_t))); EHIP(hipMemset(o.score, 0, N * sizeof(int32_t))); }
    if (!o.packed) { EHIP(hipMalloc((void**)&o.packed, N * sizeof(uint64_t))); EHIP(hipMemset(o.packed, 0, N * sizeof(uint64_t))); }
    if (!p.step_ev) EHIP(hipEventCreateWithFlags(&p.step_ev, hipEventDisableTiming));
    for (int k = 0; k < 2; k++) {
        if (!p.render_ev[k]) EHIP(hipEventCreateWithFlags(&p.render_ev[k], hipEventDisableTiming));
        if (!p.user_step_ev[k]) EHIP(hipEventCreateWithFlags(&p.user_step_ev[k], hipEventDisableTiming));
        if (!p.user_frame_ev[k]) EHIP(hipEventCreateWithFlags(&p.user_frame_ev[k], hipEventDisableTiming));
        if (!p.launch_ev[k]) EHIP(hipEventCreateWithFlags(&p.launch_ev[k], hipEventDisableTiming));
    }
    for (int q = 0; q < 2; q++) {
        if (!p.chunk_step_ev[q]) EHIP(hipEventCreateWithFlags(&p.chunk_step_ev[q], hipEventDisableTiming));
        for (int l = 0; l < 2; l++)
            if (!p.chunk_raster_ev[q][l]) EHIP(hipEventCreateWithFlags(&p.chunk_raster_ev[q][l], hipEventDisableTiming));
    }
    if (!p.arrive) {
        EHIP(hipMalloc((void**)&p.arrive, 2 * sizeof(unsigned long long)));
        EHIP(hipMemset(p.arrive, 0, 2 * sizeof(unsigned long long)));
        p.arrive_want = p.release_want = 0;
    }
    // The two internal streams are created with the highest priority.  Not for the priority's sake: the runtime multiplexes the
    // streams of a process onto a few hardware queues PER PRIORITY LEVEL (GPU_MAX_HW_QUEUES, 4 by default), two streams that
    // land on one queue do not overlap, and which streams share depends on the creation history of the whole process.  The
    // high-priority pool is the lanes' own (measured: with ordinary streams the overlapped modes were faster or slower than
    // the serial loop from one process to the next; scripts/pipeline_sweep.py).
    int lo = 0, hi = 0;
    EHIP(hipDeviceGetStreamPriorityRange(&lo, &hi));     // numerically hi <= lo
#ifdef TBX_DIAG
    if (getenv("TBX_LANE_PRIORITY")) hi = atoi(getenv("TBX_LANE_PRIORITY")) ? lo : hi;      // measurement builds: ordinary streams
#endif
    for (int k = 0; k < 2; k++)
        if (!p.lane[k]) EHIP(hipStreamCreateWithPriority(&p.lane[k], hipStreamNonBlocking, hi));
    if (!p.step_lane) EHIP(hipStreamCreateWithPriority(&p.step_lane, hipStreamNonBlocking, hi));   // (three of the priority level's four hardware queues)
    p.prepared = true;
    return TBX_OK;
}

// the first pipelined call after a call of any other kind: every internal stream behind all that came before
static int pipe_enter(tbx_engine* e, PipeKind kind)
{
    if (e->pending_kind) EHIP(tbx_finish_pending(e));           // (a host-delivery step between its begin and end calls)
    // pipelined steps / renders, overlapped fused launches and rollout chunks keep different books on the same lanes: a change of
    // kind joins first (tbx_use_stream makes the stream of the last call wait for every internal launch; the lanes re-enter behind it)
    if (e->pipe_active && pipe_kind(e) != kind) EHIP(tbx_use_stream(e, e->last_stream));
    if (e->pipe_active) return TBX_OK;
    if (e->serve_running) EHIP(tbx_serve_stop(e));
    int rc = pipe_prepare(e);
    if (rc) return rc;
    TbxPipe& p = *e->pipe;
    EHIP(tbx_wait_tail(e, p.lane[0]));
    EHIP(tbx_wait_tail(e, p.lane[1]));
    if (kind == PIPE_ROLLOUT_CHUNKS) EHIP(tbx_wait_tail(e, p.step_lane));
    p.books = PipeBooks{};
    p.books.kind = kind;
    // The caller may have queued readers of the current results before this call: it took their addresses while no form was running
    // (after tbx_sync, or behind a call of another kind), where pipe_reader_joins sees nothing, and after tbx_sync the lanes do not
    // go behind the caller's stream either.  So the first call of a stay fences that stream like a call that saw a reader -- one
    // event record per entry -- and the second call, which rewrites that output set and frame buffer, waits for the fence.
    p.books.reader_seen = true;
    e->pipe_active = true;
    return TBX_OK;
}

// The reader fence of output set `cur` ^ 1, which this call's launch on `writer` rewrites: readers of what it holds were queued on
// the caller's stream before the call before this one, which fenced them -- await that fence; then (fence_now) fence what the
// caller has queued so far, which may read set `cur`: the call after this one waits for it.
static hipError_t reader_fence(TbxPipe& p, hipStream_t writer, hipStream_t user, int cur, bool fence_now)
{
    PipeBooks& b = p.books;
    const int wp = cur ^ 1;
    if (b.user_step_rec[wp]) {
        hipError_t r = hipStreamWaitEvent(writer, p.user_step_ev[wp], 0);
        if (r != hipSuccess) return r;
        b.user_step_rec[wp] = false;
    }
    if (fence_now) {
        hipError_t r = hipEventRecord(p.user_step_ev[cur], user);
        if (r != hipSuccess) return r;
        b.user_step_rec[cur] = true;
        b.reader_seen = false;
    }
    return hipSuccess;
}

int pipe_step(tbx_engine* e, const ActionSource& src, uint32_t flags, hipStream_t user, int mode)
{
    int rc = pipe_enter(e, PIPE_STEPS_AND_RENDERS);
    if (rc) return rc;
    TbxPipe& p = *e->pipe;
    StepRenderBooks& b = p.books.sr;
    const int cur = e->out_par, wp = cur ^ 1;                  // this step writes output set wp ...
    const int rw = e->ops->records_parity() ^ 1;               // ... and records buffer rw
    hipStream_t ss = mode == 3 ? p.lane[wp] : p.lane[0];
    if (b.step_outstanding && b.step_on != ss) EHIP(hipStreamWaitEvent(ss, p.step_ev, 0));          // the state step N-1 left
    if (b.render_pending[rw]) {                                                                      // the reader of records rw
        if (b.render_on[rw] != ss) EHIP(hipStreamWaitEvent(ss, p.render_ev[rw], 0));
        b.render_pending[rw] = false;
    }
    // whatever the caller has queued so far may read the current outputs: the step after this one waits for it
    EHIP(reader_fence(p, ss, user, cur, true));
    // A render issued while the records did not reflect the state (after new_game / set_state / a single-env step) read LIVE
    // state -- the prep kernel that rebuilds the records, or a state-reading rasteriser -- on its own stream: this step, which
    // rewrites that state, goes behind it (it only waited for the reader of the OTHER records buffer).
    if (b.live_reader >= 0) {
        if (b.render_on[b.live_reader] != ss) EHIP(hipStreamWaitEvent(ss, p.render_ev[b.live_reader], 0));
        b.live_reader = -1;
    }
    tbx_set_out_parity(e, wp);
    hipError_t ge = tbx_gather_before_step(e, ss);
    rc = ge == hipSuccess ? e->ops->step_ahead(e, src, flags, ss) : hip_fail(e, "tbx_gather_before_step", ge);
    if (rc) {                                                  // nothing was launched: TBX_BUF_* keep naming the set that holds results
        tbx_set_out_parity(e, cur);
        return rc;
    }
    EHIP(hipEventRecord(p.step_ev, ss));
    EHIP(hipStreamWaitEvent(user, p.step_ev, 0));
    b.step_outstanding = true;
    b.step_on = ss;
    b.step_user = user;
    e->last_stream = user;
    e->has_last = true;
    return TBX_OK;
}

int pipe_render(tbx_engine* e, uint8_t* out_dev, int channels, hipStream_t user, int mode)
{
    int rc = pipe_enter(e, PIPE_STEPS_AND_RENDERS);
    if (rc) return rc;
    TbxPipe& p = *e->pipe;
    StepRenderBooks& b = p.books.sr;
    const int rp = e->ops->records_parity();
    const bool overlap = mode == 3 && out_dev == nullptr;
    const size_t bytes = (size_t)e->n * e->ops->height() * e->ops->width() * channels;
    hipStream_t rs = user;
    if (overlap) {
        const int fp = rp;                                     // frame buffer and stream follow the records' parity
        rs = p.lane[fp];
        EHIP(p.frame[fp].reserve(bytes, rs));
        if (b.step_outstanding && b.step_on != rs) EHIP(hipStreamWaitEvent(rs, p.step_ev, 0));
        // Readers of a frame are queued on U before the next render call.  Fence what is there now; the render into the OTHER
        // buffer waits for the fence of the call before (readers of what that buffer held), a second render into the SAME
        // buffer for the one just recorded.
        const int prev = b.frame_par < 0 ? fp ^ 1 : b.frame_par;
        EHIP(hipEventRecord(p.user_frame_ev[prev], user));
        b.user_frame_rec[prev] = true;
        if (b.user_frame_rec[fp]) { EHIP(hipStreamWaitEvent(rs, p.user_frame_ev[fp], 0)); b.user_frame_rec[fp] = false; }
        out_dev = p.frame[fp].p;
    } else {
        // on the caller's stream: it waits for the step unless it is the stream the step call named (pipe_step made that one wait)
        if (b.step_outstanding && b.step_user != user) EHIP(hipStreamWaitEvent(rs, p.step_ev, 0));
        if (!out_dev) {
            rc = ensure_frame(e, bytes);
            if (rc) return rc;
            out_dev = e->frame_own.p;
        }
    }
    if (((uintptr_t)out_dev & 15u) != 0) return e->fail(TBX_E_INVALID, "frame buffer must be 16-byte aligned");
    if (b.render_pending[rp] && b.render_on[rp] != rs) EHIP(hipStreamWaitEvent(rs, p.render_ev[rp], 0));   // (another render of these records)
    const bool reads_live = !e->ops->records_valid();          // the launch below starts from live state (pipe_step waits for it)
    rc = e->ops->render(e, out_dev, channels, 0, e->n, rs);
    if (rc) return rc;
    EHIP(hipEventRecord(p.render_ev[rp], rs));
    b.render_pending[rp] = true;
    b.render_on[rp] = rs;
    if (reads_live) b.live_reader = rp;
    if (overlap) {
        EHIP(hipStreamWaitEvent(user, p.render_ev[rp], 0));
        b.frame_par = rp;
        e->frame = p.frame[rp].p;
        e->frame_bytes = bytes;
    } else if (out_dev == e->frame_own.p) {
        e->frame = e->frame_own.p;
        e->frame_bytes = bytes;
    }
    e->last_stream = user;
    e->has_last = true;
    return TBX_OK;
}

// ---- overlapped fused launches (TBX_OPT_FUSED_OVERLAP; contract in include/toybox_amd.h)
//
// Launch N of a loop of tbx_render_step_synthetic calls = [step blocks: state t -> t+1, records R[b], outputs O[wp]] +
// [rasteriser blocks: R[a] -> frame F[wp]].  Launch N+1 needs the step blocks of launch N and nothing else of it, so it goes to
// the OTHER lane (a stream per parity, like value 3 of the pipelined mode) behind a one-wave kernel that waits until the device
// counter `arrive` says those blocks are through (they fence and bump it last).  The launch itself never waits: a grid that
// spins could fill the chip before the launch it waits for has been dispatched.  Hazards and who orders them:
//   state, O[wp] written by step N, read / rewritten by step N+1     the counter (+ an acquire fence at the head of every wave)
//   R[b] written by step N, read by rasteriser N+1                   the counter
//   R[a] read by rasteriser N, rewritten by step N+2 (three buffers) stream order: N and N+2 share a lane
//   F[wp], O[wp] written by N, rewritten by N+2                       stream order; their READERS on the caller's stream U by the
//                                                                    fence recorded on U at call N+1 (user_step_ev), awaited by N+2
//   the collective that reads O[wp] / a ring                          tbx_gather waits for both lanes' completion events;
//                                                                    tbx_gather_before_step makes the rewriting launch wait for it
//   U                                                                 waits for every launch's completion event (what the caller
//                                                                    queues next sees the results; calls of other kinds join through U)
// Measured (scripts/ubench/overlap_ticket.hip, a stand-in launch, ms per launch serial / completion-event dependency / this /
// hipStreamWaitValue64 on the counter): 4 096 envs 0.0920 / 0.0982 / 0.0887 / 0.0886, 8 192: 0.1854 / 0.1917 / 0.1794 / 0.1791,
// 65 536: 1.555 / 1.560 / 1.477 / 1.483 -- the wait kernel costs nothing against the command processor's own (beta) wait.
extern "C" __global__ void tbx_ticket_wait_kernel(const unsigned long long* arrive, unsigned long long want_steps, unsigned long long want_releases, uint32_t* err_flag)
{
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = wall_clock64();
    // (relaxed: what has to be seen behind the counter is read with agent-scope loads by the launch that follows)
    while (__hip_atomic_load(arrive + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want_releases ||
           __hip_atomic_load(arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want_steps) {
        __builtin_amdgcn_s_sleep(2);
        if (wall_clock64() - t0 > 300000000ull) { atomicOr(err_flag, 4u); return; }   // 3 s of the 100 MHz clock: report, never hang
    }
}

bool fused_overlap_on(const tbx_engine* e, const uint8_t* out_dev, int channels)
{
    const int v = e->opt[TBX_OPT_FUSED_OVERLAP];
    if (v == 2 || out_dev != nullptr || !e->ops->render_step_fused(channels)) return false;
    return v == 1 || e->ops->fused_overlap_auto(e->n, !e->gather ? 0 : e->gather_ring ? 2 : 1);
}

int fused_overlapped(tbx_engine* e, int channels, const ActionSource& src, uint32_t flags, hipStream_t user)
{
    int rc = pipe_enter(e, PIPE_FUSED_OVERLAP);
    if (rc) return rc;
    TbxPipe& p = *e->pipe;
    FusedBooks& b = p.books.fused;
    const int cur = e->out_par, wp = cur ^ 1;                  // this launch writes output set wp and frame buffer wp, on lane wp
#ifdef TBX_DIAG
    const int diag = getenv("TBX_OVERLAP_DIAG") ? atoi(getenv("TBX_OVERLAP_DIAG")) : 0;
#else
    const int diag = 0;
#endif
    hipStream_t ls = p.lane[OVL_DIAG(diag, 8) ? 0 : wp];
    const int fb = OVL_DIAG(diag, 32) ? 0 : wp;
    const size_t bytes = (size_t)e->n * e->ops->height() * e->ops->width() * channels;
    EHIP(p.frame[fb].reserve(bytes, ls));
    // Readers of what call N-2 left in set / frame wp were queued on U before call N-1, which fenced them; this call fences the
    // readers of call N-1's results for call N+1 -- if there can be any: U joined lazily (pipe_reader_joins), and a caller
    // that took no address since the last call has queued no reader.
    EHIP(reader_fence(p, ls, user, cur, p.books.reader_seen || OVL_DIAG(diag, 16)));
    uint64_t* const ring_slot = e->gather_ring ? e->packed : nullptr;      // (a K-step ring owns the record pointer)
    tbx_set_out_parity(e, wp);
    if (ring_slot) { e->packed = ring_slot; e->ops->rebind_outputs(e); }
    auto undo = [&]() { tbx_set_out_parity(e, cur); if (ring_slot) { e->packed = ring_slot; e->ops->rebind_outputs(e); } };
    hipError_t ge = tbx_gather_before_step(e, ls);
    if (ge != hipSuccess) { undo(); return hip_fail(e, "tbx_gather_before_step", ge); }
    if (b.prev_overlapped && !OVL_DIAG(diag, 64)) {
        hipLaunchKernelGGL(tbx_ticket_wait_kernel, dim3(1), dim3(64), 0, ls, p.arrive, p.arrive_want, p.release_want, e->err_flag);
        ge = hipGetLastError();
        if (ge != hipSuccess) { undo(); return hip_fail(e, "tbx_ticket_wait_kernel", ge); }
    }
    TbxOverlapLaunch ov{p.arrive, p.launch_ev[wp], e->opt[TBX_OPT_FUSED_OVERLAP_LEAD], 0, diag};
    rc = e->ops->render_step(e, p.frame[fb].p, channels, src, flags, ls, &ov);
    if (rc) { undo(); return rc; }                             // nothing was launched: TBX_BUF_* keep naming the set that holds results
    p.arrive_want += (unsigned long long)ov.step_blocks;
    p.release_want += 1;
    b.prev_overlapped = true;
    b.launch_rec[wp] = true;
    if (OVL_DIAG(diag, 128)) EHIP(hipEventRecord(p.launch_ev[wp], ls));
    b.user_waits[wp] = false;
    if (OVL_DIAG(diag, 16)) { EHIP(hipStreamWaitEvent(user, p.launch_ev[wp], 0)); b.user_waits[wp] = true; }    // (DIAG: the eager join of the first build)
    e->frame = p.frame[fb].p;
    e->frame_bytes = bytes;
    e->step_carries_order_ev = false;
    e->last_stream = user;
    e->has_last = true;
    return TBX_OK;
}

// ---- rollout chunks (tbx_rollout_synthetic; contract in include/toybox_amd.h)
//
// Chunk c (parity q = c & 1) of k frames:
//   step lane   T_c: ONE launch steps every env k frames with the state in registers; it writes the k render records R[q][0..k-1]
//               (record j = the state before frame j), the k step records (straight into a ring of the gather, or an engine-owned
//               [k][N] array) and the state.  It is ordered behind T_{c-1} by the lane, behind the rasterisers of chunk c-2 (they read
//               R[q]), behind the collective that last read the ring, behind the caller's readers of output set q.
//   lanes 0, 1  the rasteriser launches R[q][j] -> F[q][j]: k plain ones, launch j on lane j & 1, or ONE over the chunk's k x N frames
//               on lane 0 (GameOps::rollout_render_span; below).  They wait for T_c and for nothing else -- and T_{c+1} has the whole
//               length of these launches to finish beside them.  No launch ever waits for a step that is
//               running beside a rasteriser (a Breakout step kernel that takes 10 us alone takes 100-250 us there -- what made the
//               device-side ticket of overlapped fused launches wait for most of the launch before it).
//   collective  (K-step ring, K = k) behind T_c alone: it runs beside the chunk's rasterisers.
//   caller      joins lazily (tbx_device_buffer), as with overlapped fused launches.
bool rollout_chunks_on(const tbx_engine* e, int channels)
{
    const int v = e->opt[TBX_OPT_ROLLOUT_CHUNKS];
    if (v == 2 || !e->ops->rollout_ok(channels)) return false;
    if (e->gather && !e->gather_ring) return false;              // one collective per step: k collectives cannot ride on one launch
    return v == 1 || v >= 3 || e->ops->rollout_auto(e->n, !e->gather ? 0 : e->gather_ring ? 2 : 1);
}

int rollout_chunked(tbx_engine* e, int channels, const ActionSource& src, uint32_t flags, int k, hipStream_t user)
{
    int rc = pipe_enter(e, PIPE_ROLLOUT_CHUNKS);
    if (rc) return rc;
    TbxPipe& p = *e->pipe;
    ChunkBooks& b = p.books.chunk;
    TbxRolloutResult& res = e->rollout;
    const int cur = e->out_par, q = cur ^ 1;                   // this chunk: output set q, record buffer q, frame chunk q
    hipStream_t ss = p.step_lane;
    const size_t fb = (size_t)e->n * e->ops->height() * e->ops->width() * channels;
    rc = chunk_buffers(e, q, k, fb, !e->gather_ring, p.lane[0], p.lane[1]);
    if (rc) return rc;
    uint64_t* packed = res.packed[q].p;
    size_t stride = (size_t)e->n;
    if (e->gather_ring) {
        rc = tbx_gather_ring_open(e, ss, k, &packed, &stride);
        if (rc) return rc;
    }
    // T_c behind the rasterisers of chunk c - 2, which read the record buffer it rewrites
    for (int l = 0; l < 2; l++)
        if (b.raster_rec[q][l]) EHIP(hipStreamWaitEvent(ss, p.chunk_raster_ev[q][l], 0));
    // ... and behind the caller's readers of what chunk c - 2 left in output set q (fenced by call c - 1); the same fence holds the
    // rasterisers below back from the frames those readers may still read.  This call fences the readers of chunk c - 1, if the
    // caller took an address since (lazy join: no address, no reader)
    const bool fenced = p.books.user_step_rec[q];
    EHIP(reader_fence(p, ss, user, cur, p.books.reader_seen));
    tbx_set_out_parity(e, q);
    e->packed = packed + (size_t)(k - 1) * stride;              // TBX_BUF_PACKED: the record of the chunk's last step
    e->ops->rebind_outputs(e);
    rc = e->ops->rollout_step(e, src, flags, k, q, packed, stride, ss);
    if (rc) { tbx_set_out_parity(e, cur); return rc; }
    EHIP(hipEventRecord(p.chunk_step_ev[q], ss));
    b.step_rec[q] = true;
    bool lane_used[2] = {false, false};
    auto lane_for = [&](int l) -> int {
        if (!lane_used[l]) {
            EHIP(hipStreamWaitEvent(p.lane[l], p.chunk_step_ev[q], 0));
            if (fenced) EHIP(hipStreamWaitEvent(p.lane[l], p.user_step_ev[q], 0));
            lane_used[l] = true;
        }
        return TBX_OK;
    };
    const int form = e->opt[TBX_OPT_ROLLOUT_CHUNKS];
    const bool span = e->ops->rollout_span_ok() && (form == 4 || (form != 3 && e->ops->rollout_span_auto(e->n, !e->gather ? 0 : 2)));
    if (span) {
        // The chunk's frames in ONE rasteriser launch (k x n frames; at most 65 536 frames per launch), chunk behind chunk on ONE internal
        // stream: rasteriser launches back to back as in a render-only loop, k times as long as a frame's, the next chunk's step launch
        // beside them on the step lane.  Nothing runs beside a rasteriser launch but that step launch, so the rate does not depend on where
        // the frame buffers lie (two rasteriser launches side by side: 0.151-0.164 ms per step at 8 192 envs from process to process,
        // this form 0.1533-0.1536 in every one; profiles/r06_experiments.txt item 6).
        const int l = 0;
        // is the previous chunk's launch still running on that stream?  Then this one starts like a launch of a render-only loop
        bool behind = b.raster_rec[cur][l] && hipEventQuery(p.chunk_raster_ev[cur][l]) == hipErrorNotReady;
        (void)hipGetLastError();                                // (hipErrorNotReady is an answer, not an error to keep)
        rc = lane_for(l);
        if (rc) return rc;
        const int per = std::max(1, std::min(k, 65536 / std::max(1, e->n)));
        for (int j0 = 0; j0 < k; j0 += per) {
            rc = e->ops->rollout_render_span(e, res.frames[q].p + (size_t)j0 * fb, channels, q, j0, std::min(per, k - j0), behind, p.lane[l]);
            if (rc) return rc;
            behind = true;
        }
    } else {
        for (int j = 0; j < k; j++) {
            const int l = j & 1;
            rc = lane_for(l);
            if (rc) return rc;
            rc = e->ops->rollout_render(e, res.frames[q].p + (size_t)j * fb, channels, q, j, p.lane[l]);
            if (rc) return rc;
        }
    }
    for (int l = 0; l < 2; l++) {
        b.raster_rec[q][l] = lane_used[l];
        if (lane_used[l]) EHIP(hipEventRecord(p.chunk_raster_ev[q][l], p.lane[l]));
    }
    if (e->gather_ring) {
        rc = tbx_gather_ring_filled(e, p.chunk_step_ev[q]);
        if (rc) return rc;
    }
    b.user_waits[q] = false;
    res.cur = q; res.k = k; res.channels = channels;
    res.packed_base = packed; res.packed_stride = stride;
    e->frame = res.frames[q].p + (size_t)(k - 1) * fb;          // TBX_BUF_FRAME: the chunk's last frame
    e->frame_bytes = fb;
    e->step_carries_order_ev = false;
    e->last_stream = user;
    e->has_last = true;
    return TBX_OK;
}

// ---- what the rest of the engine needs of a running form

hipError_t pipe_leave(tbx_engine* e, hipStream_t s)
{
    const TbxPipe& p = *e->pipe;
    const PipeBooks& b = p.books;
    hipError_t r = hipSuccess;
    auto join = [&](bool outstanding, hipEvent_t ev) { if (outstanding && r == hipSuccess) r = hipStreamWaitEvent(s, ev, 0); };
    switch (b.kind) {
    case PIPE_STEPS_AND_RENDERS:
        // leaving the pipelined mode: a render that ran on another caller stream than the one the last pipelined call named
        // (mode 2, or out_dev given: render on U1, then a step naming U2) is not behind last_stream -- join it here
        for (int k = 0; k < 2; k++) join(b.sr.render_pending[k] && b.sr.render_on[k] && b.sr.render_on[k] != s, p.render_ev[k]);
        break;
    case PIPE_FUSED_OVERLAP:
        // ... and overlapped fused launches, which the caller's stream joins lazily (FusedBooks::user_waits): both lanes
        for (int k = 0; k < 2; k++) join(b.fused.launch_rec[k] && p.lane[k] != s, p.launch_ev[k]);
        break;
    case PIPE_ROLLOUT_CHUNKS:
        // ... and rollout chunks: the step lane and the rasterisers of both parities
        for (int q = 0; q < 2; q++) {
            join(b.chunk.step_rec[q], p.chunk_step_ev[q]);
            for (int l = 0; l < 2; l++) join(b.chunk.raster_rec[q][l], p.chunk_raster_ev[q][l]);
        }
        break;
    case PIPE_NONE: break;
    }
    return r;
}

int pipe_reader_joins(tbx_engine* e, bool frames)
{
    TbxPipe& p = *e->pipe;
    PipeBooks& b = p.books;
    if (b.kind == PIPE_FUSED_OVERLAP) {
        const int k = e->out_par;
        if (b.fused.launch_rec[k] && !b.fused.user_waits[k]) {
            EHIP(hipSetDevice(e->device));
            EHIP(hipStreamWaitEvent(e->last_stream, p.launch_ev[k], 0));
            b.fused.user_waits[k] = true;
        }
        b.reader_seen = true;
    } else if (b.kind == PIPE_ROLLOUT_CHUNKS) {
        const int q = e->rollout.cur;
        EHIP(hipSetDevice(e->device));
        if (b.chunk.step_rec[q] && !b.chunk.user_waits[q]) EHIP(hipStreamWaitEvent(e->last_stream, p.chunk_step_ev[q], 0));
        if (frames)
            for (int l = 0; l < 2; l++)
                if (b.chunk.raster_rec[q][l]) EHIP(hipStreamWaitEvent(e->last_stream, p.chunk_raster_ev[q][l], 0));
        b.chunk.user_waits[q] = true;
        b.reader_seen = true;
    }
    return TBX_OK;
}

// Overlapped fused launches: the completion events of both lanes -- the last launch and the one before it, which may still be
// painting but whose step blocks the last launch waited for; pipelined mode: the step stream's event; otherwise the tail of the handle.
hipError_t pipe_wait_for_steps(tbx_engine* e, hipStream_t gs)
{
    const PipeKind kind = pipe_kind(e);
    if (kind == PIPE_FUSED_OVERLAP) {
        const TbxPipe& p = *e->pipe;
        for (int k = 0; k < 2; k++)
            if (p.books.fused.launch_rec[k]) {
                hipError_t r = hipStreamWaitEvent(gs, p.launch_ev[k], 0);
                if (r != hipSuccess) return r;
            }
        return hipSuccess;
    }
    if (kind == PIPE_STEPS_AND_RENDERS && e->pipe->books.sr.step_outstanding) return hipStreamWaitEvent(gs, e->pipe->step_ev, 0);
    return tbx_wait_tail(e, gs, true);
}

void pipe_drain(tbx_engine* e)
{
    if (!e->pipe) return;
    for (int k = 0; k < 2; k++)
        if (e->pipe->lane[k]) hipStreamSynchronize(e->pipe->lane[k]);
    if (e->pipe->step_lane) hipStreamSynchronize(e->pipe->step_lane);
}

void pipe_free(tbx_engine* e)
{
    if (!e->pipe) return;
    TbxPipe& p = *e->pipe;
    if (p.step_ev) hipEventDestroy(p.step_ev);
    for (int k = 0; k < 2; k++) {
        p.frame[k].release();
        if (p.render_ev[k]) hipEventDestroy(p.render_ev[k]);
        if (p.user_step_ev[k]) hipEventDestroy(p.user_step_ev[k]);
        if (p.user_frame_ev[k]) hipEventDestroy(p.user_frame_ev[k]);
        if (p.launch_ev[k]) hipEventDestroy(p.launch_ev[k]);
        if (p.chunk_step_ev[k]) hipEventDestroy(p.chunk_step_ev[k]);
        for (int l = 0; l < 2; l++)
            if (p.chunk_raster_ev[k][l]) hipEventDestroy(p.chunk_raster_ev[k][l]);
    }
    hipFree(p.arrive);
    for (int k = 0; k < 2; k++)
        if (p.lane[k]) hipStreamDestroy(p.lane[k]);
    if (p.step_lane) { hipStreamSynchronize(p.step_lane); hipStreamDestroy(p.step_lane); }
    delete e->pipe;
    e->pipe = nullptr;
}
