// hold_stream.hip -- test tool: hold a stream back for a known, bounded time (tests/held_stream.py builds and loads it).
//
// tbx_test_hold(stream, microseconds) queues ONE block of 64 threads on `stream`.  Lane 0 reads the 100 MHz wall clock (100 ticks
// per microsecond, as scripts/ubench/anyorder.hip measures it), naps with s_sleep between reads and returns when the time is up.
// Whatever is queued behind it on the stream waits; whatever is queued elsewhere is free to overtake.  The kernel reads no host
// memory and waits for nothing: it is a delay, not a gate, and it always ends by itself -- the duration is clamped ON THE DEVICE
// to 250 000 us, and the loop is also bounded by a count of naps in case the clock should ever stand still.

#include <hip/hip_runtime.h>
#include <stdint.h>

#define TBX_TEST_HOLD_MAX_US 250000u
// The nap bound is a backstop, not the timer.  s_sleep(16) asks for 16 x 64 clocks, ABOUT 0.5 us at the shader clock -- an estimate,
// not a measurement: were a nap much shorter, 4 000 000 of them could end a long hold early.  Every case that holds a stream asserts
// that the hold lasted at least 0.8 of what it asked for, by events around it, so a hold that the bound cut short fails its case.
#define TBX_TEST_HOLD_MAX_NAPS 4000000u

extern "C" __global__ void tbx_test_hold_kernel(unsigned microseconds)
{
    if (threadIdx.x != 0) return;
    if (microseconds > TBX_TEST_HOLD_MAX_US) microseconds = TBX_TEST_HOLD_MAX_US;
    const uint64_t ticks = (uint64_t)microseconds * 100u;
    const uint64_t t0 = wall_clock64();
    for (unsigned naps = 0; naps < TBX_TEST_HOLD_MAX_NAPS && wall_clock64() - t0 < ticks; naps++) __builtin_amdgcn_s_sleep(16);
}

extern "C" int tbx_test_hold(void* stream, unsigned microseconds)
{
    hipLaunchKernelGGL(tbx_test_hold_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, microseconds);
    return (int)hipGetLastError();
}
