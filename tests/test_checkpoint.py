"""Checkpoints (TBX_EDIT_CHECKPOINT_*, TBX_QUERY_CHECKPOINT_VALID), the part that needs no GPU: the constants, the argument
shaping of Engine.checkpoint_*, and the yardstick of tests/test_gpu_checkpoint.py under test itself -- over the CPU checker
alone, a replay engine made with `eff` and run to the save step t_s holds the original batch's rows `eff` as they were at t_s
(tests/checkpoint_replay.py), whatever the original batch did afterwards."""
import os
import re

import numpy as np
import pytest

from checkpoint_replay import Twin, mixed_actions, pick_rows, replay_to, restore_map
from conftest import ROOT
from fork_replay import Agent, Raw, assert_snapshot_equal, fork_maps, snapshot
from test_gpu_fork import _pick_moment
from toybox_amd import Engine, ToyboxAmdError, _abi
from toybox_amd.engine import checkpoint_args

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
HEADER = open(os.path.join(ROOT, "include", "toybox_amd.h")).read()


def test_header_and_python_agree_on_the_constants():
    want = {"TBX_EDIT_CHECKPOINT_SLOTS": (_abi.EDIT_CHECKPOINT_SLOTS, 41), "TBX_EDIT_CHECKPOINT_SAVE": (_abi.EDIT_CHECKPOINT_SAVE, 42),
            "TBX_EDIT_CHECKPOINT_RESTORE": (_abi.EDIT_CHECKPOINT_RESTORE, 43), "TBX_QUERY_CHECKPOINT_VALID": (_abi.QUERY_CHECKPOINT_VALID, 140)}
    for name, (py, value) in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, HEADER)
        assert m and int(m.group(1)) == py == value, name


def test_the_header_gives_the_width_of_the_query():
    m = re.search(r"#define\s+TBX_QUERY_CHECKPOINT_VALID\s+140\s+/\*\s*\{slot\[, row\]\}\s*->\s*(\d+)(.*?)\*/", HEADER, re.S)
    assert m and int(m.group(1)) == 1 and "tbx_reduce_width" in m.group(2)


def test_the_abi_has_no_new_symbols_and_keeps_its_version():
    assert len(re.findall(r"\btbx_\w*checkpoint\w*\s*\(", HEADER)) == 0, "checkpoints go through tbx_edit / tbx_reduce"
    assert re.search(r"#define\s+TBX_ABI_VERSION\s+1\b", HEADER)


def test_the_checker_has_no_checkpoints(oracle_lib):
    """the expected values of the checkpoint tests cannot come from the checker's own: it answers "unknown edit" / "unknown query" """
    with Engine("breakout", 4, lib=oracle_lib) as e:
        for call in (lambda: e.checkpoint_slots(1), lambda: e.checkpoint_save(0), lambda: e.checkpoint_restore(0), lambda: e.checkpoint_valid(0)):
            with pytest.raises(ToyboxAmdError) as ei:
                call()
            assert ei.value.code == _abi.E_INVALID


# ---------------------------------------------------------------- the argument shaping

def test_args_scalar_forms():
    assert checkpoint_args(8, 3) == [3.0]
    assert checkpoint_args(8, 3, rows=5) == [3.0, 5.0]
    assert checkpoint_args(8, 3, rows=5, salt=9) == [3.0, 5.0, 9.0]
    assert checkpoint_args(8, 3, salt=9) == [3.0, -1.0, 9.0], "a salt without rows: the row column says 'own row'"


def test_args_per_env_forms():
    n = 6
    a = checkpoint_args(n, 1, rows=np.arange(n)[::-1])
    assert a.shape == (n, 2) and a.dtype == np.float64
    assert np.array_equal(a[:, 0], np.ones(n)) and np.array_equal(a[:, 1], np.arange(n)[::-1])
    a = checkpoint_args(n, np.arange(n) % 2)
    assert a.shape == (n, 1) and np.array_equal(a[:, 0], np.arange(n) % 2)
    a = checkpoint_args(n, np.arange(n) % 2, salt=7)
    assert a.shape == (n, 3) and np.array_equal(a[:, 1], np.full(n, -1.0)) and np.array_equal(a[:, 2], np.full(n, 7.0))
    a = checkpoint_args(n, 0, rows=2, salt=np.arange(n))
    assert a.shape == (n, 3) and np.array_equal(a[:, 1], np.full(n, 2.0)) and np.array_equal(a[:, 2], np.arange(n))


@pytest.mark.parametrize("bad", [dict(slot=np.zeros(5)), dict(slot=0, rows=np.zeros(7)), dict(slot=0, rows=None, salt=np.zeros((6, 1))),
                                 dict(slot=np.zeros(6), rows=np.zeros(5))])
def test_args_wrong_length_raises(bad):
    with pytest.raises(ValueError):
        checkpoint_args(6, **bad)


def test_the_adapters_select_envs_like_fork(monkeypatch):
    """save_checkpoint / restore_checkpoint hand Engine the mask _fork_map makes of `envs` (None, a boolean mask, indices)"""
    from toybox_amd.envs import vec_env

    class FakeEngine:
        def checkpoint_save(self, slot, mask=None):
            self.saved = (slot, mask)

    n = 6
    for cls in (vec_env.ToyboxVecEnv, vec_env.ToyboxPreprocVecEnv):
        v = object.__new__(cls)
        v.num_envs, v._in_flight, v._pending, v.engine = n, None, None, FakeEngine()
        for envs in (None, [1, 4], np.arange(n) % 2 == 0):
            calls = []
            real = vec_env._fork_map
            monkeypatch.setattr(vec_env, "_fork_map", lambda *a: calls.append(a) or real(*a))
            v.save_checkpoint(2, envs=envs)
            monkeypatch.setattr(vec_env, "_fork_map", real)
            assert len(calls) == 1 and calls[0][0] == n and calls[0][2] is envs
            assert v.engine.saved[0] == 2 and np.array_equal(v.engine.saved[1], real(n, 0, envs)[1])


# ---------------------------------------------------------------- the replay identity across time, on the checker alone

def _identity(case, lib, eff, t_s, t_on, run_kw=None):
    """the original batch at t_s and the replay made with eff at t_s; the original then plays on to t_on (the identity must not
    care: the replay is a fresh engine)"""
    o = case.make(lib)
    case.run(o, 0, t_s)
    at = snapshot(o)
    obs = case.observation(o) if hasattr(case, "observation") else o.render(3)
    case.run(o, t_s, t_on)
    o2 = replay_to(case, lib, eff, t_s)
    assert_snapshot_equal(snapshot(o2), at, "replay at step %d" % t_s, eff)
    got = case.observation(o2) if hasattr(case, "observation") else o2.render(3)
    assert np.array_equal(got, obs[eff])
    return o, o2


@pytest.mark.parametrize("game", GAMES)
def test_replay_across_time_raw(game, oracle_lib):
    """the twin of the raw-layer cases: 48 envs saved at frame 120, the batch at 160, the masked random map with repeats; then
    Twin(replay, original) steps as one batch whose rows come from the right engine"""
    n, t_s, t_r = 48, 120, 160
    case = Raw(game, n)
    src, mask = fork_maps(n, seed=11)["random_repeats"]
    rows, eff = restore_map(n, src, mask)
    assert (rows[~mask] >= n).all() and np.array_equal(eff[~mask], np.arange(n)[~mask])
    o, o2 = _identity(case, oracle_lib, eff, t_s, t_r)
    x = Twin(o2, o, mask)
    a = case.actions(t_r)
    r = x.step(a)
    o3 = replay_to(case, oracle_lib, eff, t_s)
    assert np.array_equal(r[3][mask], o3.step(a, auto_reset=True)[3][mask])
    o.close(); o2.close(); o3.close()


@pytest.mark.parametrize("game", GAMES)
def test_replay_across_time_two_slots_and_reversal(game, oracle_lib):
    """the twin of the two-slot case (rows reversed, saves at 20 and 35, n = 32) and of the 8 200-env case's times (20, 30)"""
    n = 32
    case = Raw(game, n)
    rev = n - 1 - np.arange(n)
    for t_s in (20, 35):
        o, o2 = _identity(case, oracle_lib, rev, t_s, 50)
        o.close(); o2.close()


AGENT_FORMS = {"rolled": {}, "new_plane_1": {"new_plane": 1}, "ring": {"new_plane": 2}, "stack_fill": {"stack_fill": 1}}


@pytest.mark.parametrize("form", list(AGENT_FORMS))
@pytest.mark.parametrize("game", GAMES)
def test_replay_across_time_agent(game, form, oracle_lib):
    """the twin of the agent-layer cases: 24 envs saved at agent step 40, the batch at 63 (the ring form: the two engines' ring
    heads stand 23 = 3 mod 4 slots apart, and the observation is read through each engine's own head); the 60 steps of mixed
    action rows that follow cross a `done` and (Amidar aside) an ended episode"""
    n, t_s, t_r = 24, 40, 63
    case = Agent(game, n, **AGENT_FORMS[form])
    src = fork_maps(n, seed=5)["random_repeats"][0]
    sel = np.arange(n) % 3 != 0
    rows, eff = restore_map(n, src, sel)
    o, o2 = _identity(case, oracle_lib, eff, t_s, t_r)
    if form == "ring":
        assert (o.agent_ring_head() - o2.agent_ring_head()) % 4 == 3
    want = Twin(o2, o, sel).agent_rows(case, [mixed_actions(case, sel, eff, t_s, t_r, k) for k in range(60)])
    ended, done = np.stack([r[3] for r in want]), np.stack([r[2] for r in want])
    assert done.any() and (ended.any() or game == "amidar")
    o.close(); o2.close()


@pytest.mark.parametrize("moment", ["life", "game"])
@pytest.mark.parametrize("game", GAMES)
def test_replay_across_time_agent_moments(game, moment, oracle_lib):
    """the twin of the moment cases: the saved row is the env that lost a life / whose game ended at the save step"""
    if game == "gridworld" and moment == "life":
        moment = "game"
    n = 24
    case = Agent(game, n, **({"new_plane": 2} if moment == "game" else {}))
    o = case.make(oracle_lib)
    t_s, star = _pick_moment(case.run(o, 0, 130), moment, 40)
    o.close()
    rows, eff = restore_map(n, np.full(n, star), np.arange(n) % 3 == 1)
    o, o2 = _identity(case, oracle_lib, eff, t_s, t_s + 30)
    o.close(); o2.close()


def test_pick_rows():
    sel = np.array([True, False, True])
    a, b = np.arange(6).reshape(3, 2), -np.arange(6).reshape(3, 2)
    assert np.array_equal(pick_rows(sel, a, b), [[0, 1], [-2, -3], [4, 5]])
    assert np.array_equal(pick_rows(sel, [1, 2, 3], [7, 8, 9]), [1, 8, 3])
