// engine_host.hpp -- host-side helpers shared by engine.hip and pipeline.hip
#pragma once

#include "tbx_common.hpp"

#define CHECK_ENGINE(e) \
    if (!(e)) return TBX_E_INVALID

inline int hip_fail(tbx_engine* e, const char* what, hipError_t err)
{
    return e->fail(TBX_E_NO_DEVICE, std::string(what) + ": " + hipGetErrorString(err));
}

#define EHIP(call)                                        \
    do {                                                  \
        hipError_t _e = (call);                           \
        if (_e != hipSuccess) return hip_fail(e, #call, _e); \
    } while (0)

// engine.hip
int ensure_frame(tbx_engine* e, size_t bytes);     // TBX_BUF_FRAME names the engine-owned frame buffer, `bytes` large
int chunk_buffers(tbx_engine* e, int q, int k, size_t frame_bytes, bool want_packed, hipStream_t sync_a, hipStream_t sync_b);
