// pipeline.hpp -- the pipelined step / render mode and the overlapped loop forms on top of it (pipeline.hip): what the rest of
// the engine calls.  Their state (TbxPipe) is the module's own; tbx_engine holds the pointer and `pipe_active`.
#pragma once

#include "tbx_common.hpp"

// which form a call takes (the options, the game's abilities and the engine's choice), and the forms themselves
int pipe_mode(const tbx_engine* e);
int pipe_step(tbx_engine* e, const ActionSource& src, uint32_t flags, hipStream_t user, int mode);
int pipe_render(tbx_engine* e, uint8_t* out_dev, int channels, hipStream_t user, int mode);
bool fused_overlap_on(const tbx_engine* e, const uint8_t* out_dev, int channels);
int fused_overlapped(tbx_engine* e, int channels, const ActionSource& src, uint32_t flags, hipStream_t user);
bool rollout_chunks_on(const tbx_engine* e, int channels);
int rollout_chunked(tbx_engine* e, int channels, const ActionSource& src, uint32_t flags, int k, hipStream_t user);

// tbx_use_stream while tbx_engine::pipe_active: stream s waits for every internal launch that is not behind the stream of the last call
hipError_t pipe_leave(tbx_engine* e, hipStream_t s);
// tbx_device_buffer while tbx_engine::pipe_active: the caller asks where a result of the last call lies -- the stream that call
// named now waits for the launch that wrote it (frames: for the rasterisers of the chunk as well)
int pipe_reader_joins(tbx_engine* e, bool frames);
// the communication stream behind the step(s) whose records a collective reads (gather.hip)
hipError_t pipe_wait_for_steps(tbx_engine* e, hipStream_t gs);
// tbx_destroy: the internal streams run dry (before anything they use is freed); events, buffers and streams go.  Without a pipe: nothing
void pipe_drain(tbx_engine* e);
void pipe_free(tbx_engine* e);
