"""The whole-output frame checker of tests/support.py (FrameChecker + orc_render_envs), on the CPU: it must pass equal frames, fail on
any single wrong byte wherever it lies relative to its slices, and name that byte; the oracle's env-range painter must equal its
one-env painter.  The GPU frame tests (tests/test_gpu_frames.py and others) rely on both."""
import re

import numpy as np
import pytest

from support import FrameChecker, oracle_frames, oracle_render_envs, synthetic_actions
from toybox_amd import Engine, ToyboxAmdError

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]


def _rolled(game, n, oracle_lib, steps=30):
    o = Engine(game, n, lib=oracle_lib)
    o.seed(77)
    o.new_game()
    for t in range(steps):
        o.step(synthetic_actions(game, n, t), auto_reset=True)
    return o


@pytest.mark.parametrize("game", GAMES)
def test_render_envs_equals_render_env(game, oracle_lib):
    n = 19
    o = _rolled(game, n, oracle_lib)
    H, W = o.height, o.width
    for channels in (1, 3, 4):
        one = np.stack([o.render_env(i, channels) for i in range(n)])
        assert np.array_equal(o.render(channels), one), channels
        for first, count in ((0, n), (0, 1), (5, 7), (n - 1, 1), (3, n - 3), (4, 0)):
            out = np.full((max(count, 1), H, W, channels), 0xA5, np.uint8)
            oracle_render_envs(o, first, count, out, channels)
            assert np.array_equal(out[:count], one[first:first + count]), (channels, first, count)
    out = np.empty((n + 1, H, W, 3), np.uint8)
    for first, count in ((-1, 2), (0, n + 1), (n, 1), (2, -1)):
        with pytest.raises(ToyboxAmdError):
            oracle_render_envs(o, first, count, out, 3)
    with pytest.raises(ToyboxAmdError):
        oracle_render_envs(o, 0, 1, out, 2)
    o.close()


def _report(err):
    m = re.search(r"frame j=(\d+) env i=(\d+) y=(\d+) x=(\d+) channel (\d+) \(got (\d+), want (\d+)\); (\d+) frames of (\d+), (\d+) envs",
                  str(err.value))
    assert m, str(err.value)
    return tuple(int(v) for v in m.groups())


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_frame_checker_finds_every_flipped_byte(channels, oracle_lib):
    n, per = 23, 4                                     # slices of 4 frames: 0-3, 4-7, ..., 20-22
    o = _rolled("breakout", n, oracle_lib)
    H, W = o.height, o.width
    shape = (H, W, channels)
    chk = FrameChecker(shape, slice_bytes=per * H * W * channels)
    assert chk.per == per
    frames = o.render(channels)

    def source(arr):
        def fill(lo, hi, out):
            out[:hi - lo] = arr[lo:hi]
        return fill

    chk.compare(source(frames), oracle_frames(o, channels), n, what="equal")
    chk.compare(oracle_frames(o, channels), oracle_frames(o, channels), n, what="itself")
    last = (H - 1, W - 1, channels - 1)
    for f, (y, x, c) in ((0, (0, 0, 0)), (per - 1, last), (per, (0, 0, 0)), (n - 1, last), (2 * per + 1, (H // 2, W // 3, channels // 2))):
        bad = frames.copy()
        bad[f, y, x, c] ^= 0x5A
        with pytest.raises(AssertionError) as err:
            chk.compare(source(bad), oracle_frames(o, channels), n, what="flip")
        assert _report(err) == (0, f, y, x, c, int(bad[f, y, x, c]), int(frames[f, y, x, c]), 1, n, 1)
        # numbered as frames frame0 .. of a chunk of steps of n envs: (step, env) of the frame
        with pytest.raises(AssertionError) as err:
            chk.compare(source(bad), oracle_frames(o, channels), n, n=n, frame0=3 * n)
        assert _report(err)[:2] == (3, f)
        with pytest.raises(AssertionError) as err:
            chk.compare(source(bad), oracle_frames(o, channels), n, n=10, frame0=5)
        assert _report(err)[:2] == ((5 + f) // 10, (5 + f) % 10)
    # several wrong frames: the first one is named, all are counted
    bad = frames.copy()
    bad[n - 1, 0, 0, 0] ^= 1
    bad[per + 2, H - 1, 0, 0] ^= 1
    bad[per + 2, 0, W - 1, 0] ^= 1
    with pytest.raises(AssertionError) as err:
        chk.compare(source(bad), oracle_frames(o, channels), n)
    assert _report(err) == (0, per + 2, 0, W - 1, 0, int(bad[per + 2, 0, W - 1, 0]), int(frames[per + 2, 0, W - 1, 0]), 2, n, 2)
    o.close()
