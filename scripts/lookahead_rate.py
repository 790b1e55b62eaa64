#!/usr/bin/env python3
"""What TBX_QUERY_LOOKAHEAD_ALL costs next to the composition that answers the same question without it (include/toybox_amd.h).
One process; Breakout, SpaceInvaders and Amidar at 4 096 and 65 536 envs, horizons of 16 and 64 frames, agent layer off.

  (A) the composition: one whole-batch TBX_EDIT_CHECKPOINT_SAVE, then per legal action H x tbx_step_device with a constant action
      row (no auto-reset), a device-side copy of the score and lives outputs aside, and one whole-batch
      TBX_EDIT_CHECKPOINT_RESTORE -- all device forms on one caller's stream.  (It reads the end state only: the per-frame
      fields of the query -- return, first lost life, frames run -- would need a read per frame on top.)
  (B) one tbx_reduce_device(TBX_QUERY_LOOKAHEAD_ALL) with hold = H and rest = -1 replaced by the same held action: {H, H}.

The two arms are interleaved in one process, REGIONS regions each after one warm-up, timed with HIP events on the caller's
stream; the median region is reported as ms per call and as env-frames/s (N x n_legal x H frames per call -- an upper count for
envs whose game ends early, the same for both arms).  Beside them: the batch step kernel's own rate on the same engine (H plain
tbx_step_synthetic launches, N x H frames) as the ceiling a frame costs when nothing else is paid, and --bench-line, the
flagship line of bench.py from the same session, quoted as it is.

    python scripts/lookahead_rate.py [--out profiles/lookahead.md] [--bench-line FILE]

Needs a GPU; prints the markdown it writes and keeps the file's "## Kernel resources" section, which is written by hand from the
compiler's resource remarks (make -C toybox_amd/csrc resources).  No ratio is expected in advance: the figures are the result."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fork_rate import make  # noqa: E402
from toybox_amd import _abi, hip  # noqa: E402

REGIONS = 5
KEEP = "## Kernel resources"
GAMES, SIZES, HORIZONS = ("breakout", "space_invaders", "amidar"), (4096, 65536), (16, 64)


def region_ms(stream, body, calls):
    a, b = hip.Event(), hip.Event()
    a.record(stream)
    for _ in range(calls):
        body()
    b.record(stream)
    b.synchronize()
    return a.elapsed_ms(b) / calls


def measure(game, n):
    e = make(game, n, "raw")
    for t in range(16, 400):                                 # mid-game states: balls in play, formations on the move, games ending
        e.step_synthetic(1337, t, auto_reset=True)
    e.checkpoint_slots(1)
    legal = e.legal_actions
    s = hip.Stream()
    rows = [hip.malloc(4 * n) for _ in legal]
    for p, a in zip(rows, legal):
        hip.memcpy_htod(p, np.full(n, a, np.int32), 4 * n)
    aside = hip.malloc(8 * n * len(legal))
    out = hip.malloc(8 * 5 * n * len(legal))
    results = []
    try:
        for h in HORIZONS:
            def composition():
                e.edit_device(_abi.EDIT_CHECKPOINT_SAVE, [0], stream=s.ptr)
                for k, p in enumerate(rows):
                    for _ in range(h):
                        e.step_device(p, auto_reset=False, stream=s.ptr)
                    for j, which in enumerate((_abi.BUF_SCORE, _abi.BUF_LIVES)):
                        src, nbytes = e.device_buffer(which)
                        hip.memcpy_dtod_async(aside + 4 * n * (2 * k + j), src, nbytes, s)
                    e.edit_device(_abi.EDIT_CHECKPOINT_RESTORE, [0], stream=s.ptr)

            def query():
                e.reduce_device(_abi.QUERY_LOOKAHEAD_ALL, out, [h, h], stream=s.ptr)

            def steps():
                for t in range(h):
                    e.step_synthetic(1337, 400 + t, auto_reset=True, stream=s.ptr)

            calls_b = 4 if n <= 4096 else 1
            region_ms(s, composition, 1), region_ms(s, query, 1)          # warm-ups
            ta, tb = [], []
            for _ in range(REGIONS):
                ta.append(region_ms(s, composition, 1))
                tb.append(region_ms(s, query, calls_b))
            e.edit_device(_abi.EDIT_CHECKPOINT_SAVE, [0], stream=s.ptr)
            region_ms(s, steps, 1)
            tc = [region_ms(s, steps, 1) for _ in range(REGIONS)]
            e.edit_device(_abi.EDIT_CHECKPOINT_RESTORE, [0], stream=s.ptr)
            results.append((h, len(legal), np.asarray(ta), np.asarray(tb), np.asarray(tc)))
    finally:
        s.synchronize()
        e.sync()
        for p in rows + [aside, out]:
            hip.free(p)
        s.close()
    box = e.device_identity()
    e.close()
    return results, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookahead.md"))
    ap.add_argument("--bench-line", default=None, help="file whose last JSON line is bench.py's result of the same session")
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("lookahead_rate.py measures on a GPU; none found")
    rows, slower, box = [], [], None
    for game in GAMES:
        for n in SIZES:
            res, box = measure(game, n)
            for h, a_count, ta, tb, tc in res:
                frames = n * a_count * h
                a, b, c = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
                if b > a:
                    slower.append("%s %d envs H=%d" % (game, n, h))
                rows.append("| %s | %d | %d | %d | %.3f (%.3f - %.3f) | %.0f | %.3f (%.3f - %.3f) | %.0f | %.2f | %.0f |" % (
                    game, n, h, a_count, a, ta.min(), ta.max(), frames / a / 1e3, b, tb.min(), tb.max(), frames / b / 1e3, a / b, n * h / c / 1e3))
                print(rows[-1], flush=True)
    bench = "not given"
    if args.bench_line and os.path.exists(args.bench_line):
        for line in open(args.bench_line):
            line = line.strip()
            if line.startswith("{"):
                try:
                    j = json.loads(line)
                    bench = "%s: %.2f M %s (%.4f ms per step)" % (j.get("metric"), j["value"] / 1e6, j.get("unit"), j.get("ms_per_step", float("nan")))
                except (ValueError, KeyError):
                    pass
    lines = ["# Lookahead rate (scripts/lookahead_rate.py)", "",
             "Box: %s (%s, %d CUs), one process, agent layer off.  ms per call as the median (min - max) of %d interleaved regions after one "
             "warm-up, HIP events on the caller's stream.  (A) = the composition the engine offered before: TBX_EDIT_CHECKPOINT_SAVE, then per "
             "legal action H x tbx_step_device with a constant action row, a device-side copy of the score and lives outputs, "
             "TBX_EDIT_CHECKPOINT_RESTORE -- device forms.  (B) = one tbx_reduce_device(TBX_QUERY_LOOKAHEAD_ALL) {H, hold = H}.  "
             "M env-frames/s counts N x n_legal x H frames per call for both arms.  Step ceiling: H plain tbx_step_synthetic launches (auto-reset on) on the "
             "same engine, N x H frames.  bench.py line of the session -- %s." % (
                 box["name"] or "device %d at %s" % (box["ordinal"], box["pci"]), box["arch"], box["compute_units"], REGIONS, bench), "",
             "| game | envs | H | actions | (A) ms | (A) M env-frames/s | (B) ms | (B) M env-frames/s | (A) / (B) | step ceiling M env-frames/s |",
             "|---|---|---|---|---|---|---|---|---|---|"] + rows
    lines += ["", "The query is slower than the composition in: %s." % (", ".join(slower) if slower else "no row")]
    if os.path.exists(args.out):
        old = open(args.out).read()
        if KEEP in old:
            lines += ["", old[old.index(KEEP):].rstrip()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
