"""A held stream (test tool): tests/hold_stream.hip built on first use, and the bookkeeping around it.

hold(stream, us) queues a kernel that keeps `stream` busy for `us` microseconds (at most 250 000: the device code clamps) and does
nothing else.  What is queued behind it waits, what is queued on other streams may overtake: an ordering that the engine owes and
forgot shows as wrong bytes at any batch size.  The kernel is a delay, not a gate -- it always ends by itself.

    with Held(stream, us) as h:        # start event, the hold, an event right behind the hold
        ...                            # queue work
        alive = h.in_flight()          # was the hold still running when this line was reached?
    h.observed_ms()                    # after the stream has been waited for: how long the hold lasted, by the two events
"""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

from toybox_amd import hip

HIP_ERROR_NOT_READY = 600                                    # hipErrorNotReady
MAX_HOLD_US = 250000                                         # the clamp of tests/hold_stream.hip

_lib = None
_dir = None


def library():
    """the hold library: hipcc --offload-arch=gfx950 -shared -fPIC into a temporary directory, once per process"""
    global _lib, _dir
    if _lib is None:
        hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        _dir = tempfile.TemporaryDirectory(prefix="tbx_hold_")
        so = os.path.join(_dir.name, "libtbx_hold.so")
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hold_stream.hip")
        subprocess.run([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so, src], check=True)
        _lib = C.CDLL(so)
        _lib.tbx_test_hold.restype = C.c_int
        _lib.tbx_test_hold.argtypes = [C.c_void_p, C.c_uint]
    return _lib


def _handle(stream):
    return stream.handle if isinstance(stream, hip.Stream) else C.c_void_p(int(stream or 0))


def hold(stream, us):
    """keep `stream` (a hip.Stream or a raw handle) busy for `us` microseconds"""
    us = int(us)
    assert 0 < us <= MAX_HOLD_US, "a hold lasts 1 .. %d us, not %d" % (MAX_HOLD_US, us)
    hip.check(library().tbx_test_hold(_handle(stream), us), "tbx_test_hold")


def in_flight(event):
    """hipEventQuery: True while what the event was recorded behind has not finished"""
    rt = hip.runtime()
    rc = rt.hipEventQuery(event.handle)
    if rc == HIP_ERROR_NOT_READY:
        rt.hipGetLastError()                                 # (an answer, not an error to keep)
        return True
    hip.check(rc, "hipEventQuery")
    return False


class Held:
    """Context manager: on entry an event, the hold and a second event go onto `stream`.  in_flight() tells whether the hold was
    still running at the line that asks; observed_ms(), once the stream has drained, how long it lasted.  Leaving the block waits
    for nothing."""

    def __init__(self, stream, us):
        self.stream, self.us = stream, int(us)
        self.start, self.end = hip.Event(), hip.Event()

    def __enter__(self):
        self.start.record(self.stream)
        hold(self.stream, self.us)
        self.end.record(self.stream)
        return self

    def __exit__(self, *exc):
        return False

    def in_flight(self):
        return in_flight(self.end)

    def observed_ms(self):
        self.end.synchronize()
        return self.start.elapsed_ms(self.end)

    def close(self):
        self.start.close()
        self.end.close()
