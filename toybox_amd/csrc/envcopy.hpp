// envcopy.hpp -- whole envs moved on the device (envcopy.hip): the fork and the checkpoints, what the rest of the engine calls.
// Their state (TbxEnvCopy: the fork's scratch copy, the checkpoint store) is the module's own; tbx_engine holds the pointer.
#pragma once

#include "tbx_common.hpp"

// TBX_EDIT_COPY_ENV on stream s; direct: one pass, which fork_check_host (the host form: it sees the rows) has found safe
int fork_check_host(tbx_engine* e, const double* args, int n_args, int per_env, const uint8_t* mask_host, bool& direct);
int fork_envs(tbx_engine* e, const TbxEditArgs& a, const uint8_t* mask_dev, bool direct, hipStream_t s);
// TBX_EDIT_CHECKPOINT_SLOTS (the caller has drained the stream), _SAVE / _RESTORE on stream s (check: the host form),
// TBX_QUERY_CHECKPOINT_VALID
int checkpoint_slots(tbx_engine* e, const double* args, int n_args, int per_env, const uint8_t* mask_host);
int checkpoint_copy(tbx_engine* e, bool save, const TbxEditArgs& a, const uint8_t* mask_dev, bool check, hipStream_t s);
int checkpoint_valid(tbx_engine* e, const TbxEditArgs& a, double* out_dev, hipStream_t s);
// tbx_destroy: the scratch copy and the store go.  Without either: nothing
void envcopy_free(tbx_engine* e);
