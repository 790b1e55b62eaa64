#!/usr/bin/env python3
"""What a checkpoint costs next to a fork (TBX_EDIT_CHECKPOINT_SAVE / _RESTORE against TBX_EDIT_COPY_ENV, include/toybox_amd.h):
one process, Breakout, 65 536 envs, without the agent layer and with it (rolled stack), HIP events around single repetitions,
20 of them after 3 warm-ups:

  (a) a whole-batch SAVE into slot 0 followed by a whole-batch RESTORE from it (device forms, one pass each);
  (b) one fork with the reversal map (device form: a gather into the scratch copy, then a scatter) -- the same bytes, moved
      twice over as well.

Expectation: (a) <= 1.15 x (b); the margin is the per-env cell lookup and the valid bytes.

    python scripts/checkpoint_rate.py [--out profiles/checkpoints.md] [--envs 65536]

Needs a GPU; prints the markdown it writes.  Exit status 1 when (a) misses the expectation."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fork_rate import fork_bytes, make  # noqa: E402
from toybox_amd import _abi, hip  # noqa: E402

WARMUPS, REPEATS, MARGIN = 3, 20, 1.15


def timed(stream, body):
    """ms of every one of REPEATS runs of body() on `stream`, after WARMUPS untimed ones"""
    a, b = hip.Event(), hip.Event()
    out = []
    for r in range(WARMUPS + REPEATS):
        a.record(stream)
        body()
        b.record(stream)
        b.synchronize()
        if r >= WARMUPS:
            out.append(a.elapsed_ms(b))
    return np.asarray(out)


def measure(n, layer):
    e = make("breakout", n, layer)
    e.checkpoint_slots(1)
    rows = np.ascontiguousarray(np.arange(n, dtype=np.float64)[::-1].reshape(n, 1))
    d_rows = hip.malloc(rows.nbytes)
    hip.memcpy_htod(d_rows, rows, rows.nbytes)
    s = hip.Stream()
    try:
        def save_restore():
            e.edit_device(_abi.EDIT_CHECKPOINT_SAVE, [0], stream=s.ptr)
            e.edit_device(_abi.EDIT_CHECKPOINT_RESTORE, [0], stream=s.ptr)

        def fork():
            e.edit_device(_abi.EDIT_COPY_ENV, stream=s.ptr, per_env_ptr=d_rows, n_args=1)

        ta, tb = timed(s, save_restore), timed(s, fork)
        assert (e.checkpoint_valid(0) == 1).all()
    finally:
        s.synchronize()
        e.sync()                                             # the engine forgets the stream before it is destroyed (toybox_amd.h)
        hip.free(d_rows)
        s.close()
    box = e.device_identity()
    e.close()
    return ta, tb, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoints.md"))
    ap.add_argument("--envs", type=int, default=65536)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("checkpoint_rate.py measures on a GPU; none found")
    n = args.envs
    rows, missed, box = [], [], None
    for layer in ("raw", "stack"):
        ta, tb, box = measure(n, layer)
        cell = fork_bytes("breakout", layer)
        moved = 2.0 * cell * n                               # every byte of every env twice: save + restore, gather + scatter
        a, b = float(np.median(ta)), float(np.median(tb))
        if a > MARGIN * b:
            missed.append(layer)
        rows.append("| %s | %d | %d | %.4f / %.4f / %.4f | %.0f | %.4f / %.4f / %.4f | %.0f | %.2f |" % (
            layer, n, cell, a, ta.min(), ta.max(), 2 * moved / a / 1e6, b, tb.min(), tb.max(), 2 * moved / b / 1e6, a / b))
        print(rows[-1], flush=True)
    lines = ["# Checkpoint rate (scripts/checkpoint_rate.py)", "",
             "Box: %s (%s, %d CUs), one process.  Breakout, ms per repetition as median / min / max of %d repetitions after %d warm-ups "
             "(HIP events on the caller's stream).  (a) = one whole-batch TBX_EDIT_CHECKPOINT_SAVE + one whole-batch "
             "TBX_EDIT_CHECKPOINT_RESTORE, device forms; (b) = one TBX_EDIT_COPY_ENV with the reversal map, device form (gather into the "
             "scratch copy + scatter).  Both move every byte of every env twice; GB/s counts each move as a read and a write "
             "(4 x bytes per cell x envs per repetition).  Bytes per cell: the arrays the fork plan lists, without the 256-byte "
             "alignment of each array's plane." % (box["name"] or "device %d at %s" % (box["ordinal"], box["pci"]), box["arch"], box["compute_units"], REPEATS, WARMUPS), "",
             "| layer | envs | bytes / cell | (a) save + restore ms | (a) GB/s | (b) fork ms | (b) GB/s | (a) / (b) |",
             "|---|---|---|---|---|---|---|---|"] + rows
    lines += ["", "Expectation (a) <= %.2f x (b): %s" % (MARGIN, "met in every row" if not missed else "MISSED for " + ", ".join(missed))]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
