"""A fork and a save-then-restore of the same map are the same operation (TBX_EDIT_COPY_ENV against TBX_EDIT_CHECKPOINT_SAVE +
_RESTORE, include/toybox_amd.h): both move one row of every per-env array to every selected env, by the copy kernels of
toybox_amd/csrc/envcopy.hip.  Two device engines are prepared identically (tests/fork_replay.py: the same seeds, edits and
steps); A gets fork(src, mask, salt), B checkpoint_slots(1), a whole-batch save into slot 0 and restore(0, rows=src, mask, salt)
at once.  Every state byte and the simulator RNG must be equal afterwards, and so must every output of the steps that follow,
played with the same action rows.  The row entries of B's unselected envs name a row outside the batch: the mask must keep them
from being read.  49 cases, 8 s together on an MI355X (the 8 200-env case 1.5 s)."""
import numpy as np
import pytest

from checkpoint_replay import restore_map
from fork_replay import Agent, Raw, assert_rows_equal, assert_snapshot_equal, fork_maps, snapshot
from test_gpu_checkpoint import _restore, _save
from test_gpu_fork import _device_fork

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
MAPS = ["masked_identity", "one_to_all", "reversal", "swap_pairs", "random_repeats", "some_self"]
SALTED = ("one_to_all", "random_repeats")                   # per-env salts, zeros (no salt for that env) among them
RAW_CASES = [(m, "host") for m in MAPS] + [("random_repeats", "device"), ("reversal", "device")]


def _salts(n):
    s = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(2 ** 32)
    s[np.arange(n) % 4 == 1] = 0
    return s


def _fork_and_restore(a, b, name, form, seed):
    """engine a forked, engine b saved and restored, through map `name` of fork_maps"""
    n = a.n_envs
    src, mask = fork_maps(n, seed=seed)[name]
    salt = _salts(n) if name in SALTED else None
    if form == "host":
        a.fork(src, mask=mask, salt=salt)
    else:
        _device_fork(a, src, mask, salt=salt)
    rows = src if mask is None else restore_map(n, src, mask)[0]
    b.checkpoint_slots(1)
    _save(b, form, 0)
    _restore(b, form, 0, rows=rows, mask=mask, salt=salt)


def _raw_case(game, n, name, form, hip_lib, t0=60, t1=84):
    case = Raw(game, n)
    a, b = case.make(hip_lib), case.make(hip_lib)
    what = "%s n=%d map %s %s" % (game, n, name, form)
    assert_rows_equal(case.run(b, 0, t0), case.run(a, 0, t0), what + ": the two engines before the copy")
    _fork_and_restore(a, b, name, form, seed=n)
    assert_snapshot_equal(snapshot(b), snapshot(a), what + " right after")
    assert_rows_equal(case.run(b, t0, t1), case.run(a, t0, t1), what + " after")     # (the same action rows: actions(t))
    assert np.array_equal(b.render(1), a.render(1)), what + ": gray frames at the end"
    assert_snapshot_equal(snapshot(b), snapshot(a), what + " at the end")
    a.close(); b.close()


@pytest.mark.parametrize("name,form", RAW_CASES)
@pytest.mark.parametrize("game", GAMES)
def test_raw_fork_equals_save_and_restore(game, name, form, hip_lib):
    """700 envs (no multiple of 256 or of 4, several blocks of both copy kernels), 60 frames before and 24 after: direct and
    two-pass forks, masks, self-copies, per-env salts on two maps; the device forms on a stream of the caller's"""
    _raw_case(game, 700, name, form, hip_lib)


@pytest.mark.parametrize("name", ["swap_pairs", "random_repeats"])
@pytest.mark.parametrize("new_plane", [0, 2])
@pytest.mark.parametrize("game", GAMES)
def test_agent_fork_equals_save_and_restore(game, new_plane, name, hip_lib):
    """24 envs with every wrapper on, copied after 41 agent steps (the plane ring's head is not 0): the observation right after
    and 20 agent steps"""
    case = Agent(game, 24, new_plane=new_plane)
    a, b = case.make(hip_lib), case.make(hip_lib)
    what = "%s new_plane=%d map %s" % (game, new_plane, name)
    assert_rows_equal(case.run(b, 0, 41), case.run(a, 0, 41), what + ": the two engines before the copy")
    if new_plane == 2:
        assert a.agent_ring_head() != 0, "the ring's head is 0: the case does not test what it is meant to"
    _fork_and_restore(a, b, name, "host", seed=5)
    assert np.array_equal(case.observation(b), case.observation(a)), what + ": observations right after"
    assert_snapshot_equal(snapshot(b), snapshot(a), what + " right after")
    assert_rows_equal(case.run(b, 41, 61), case.run(a, 41, 61), what + " after")
    assert_snapshot_equal(snapshot(b), snapshot(a), what + " at the end")
    a.close(); b.close()


def test_strided_rows_grid_fork_equals_save_and_restore(hip_lib):
    """the first size at which the rows kernel's grid (2 048 blocks of 4 waves = 8 192 env rows) strides; device forms"""
    _raw_case("breakout", 8200, "reversal", "device", hip_lib)
