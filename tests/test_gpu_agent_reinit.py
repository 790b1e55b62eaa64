"""tbx_agent_init a second and a third time on a live engine, held to the CPU oracle.

A re-init frees every array of the agent layer and makes it anew under another config (other observation form, stack depth, frame
skip and output size), while the game's snapshot slots stay from the first call.  Three phases on ONE engine of 65 envs (two waves
and a partial block) per game, each agent_init -> agent_reset -> STEPS[game][phase] agent steps of random legal actions:

1. the rolled stack: stack 4, 84 x 84, skip 4;
2. the ring of planes (new_plane = 2): stack 2, skip 2, a second size from the per-game table of include/toybox_amd.h;
3. the rolled stack with its newest plane beside it (new_plane = 1): stack 4, 84 x 84, skip 4;

every wrapper the game supports on in all three.  After every call: the observation (or the ring and its head, or the plane),
reward, done and the episode records; at the end of each phase every byte tbx_get_states reports of all 65 envs.

The test without the gpu mark is the twin: the same calls on the checker alone, and the conditions that keep the comparison from
being vacuous -- some env reports done in every phase, and the three phases' observations have the shapes they were configured for.
"""
import os

import numpy as np
import pytest

from fork_replay import states_bytes
from support import LEGAL, read_buffer
from toybox_amd import Engine, _abi

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
N = 65
SECOND_SIZE = {"breakout": (53, 47), "space_invaders": (45, 64), "amidar": (50, 40), "gridworld": (32, 40)}   # (out_h, out_w)
# Agent steps per phase.  From a fresh reset 12 steps end no life in any of the games, so each phase runs until the checker alone has
# seen an env report done, and a little longer (first done at step 18 / 39 / 18 in Breakout, 48 / 98 / 46 in SpaceInvaders, 65-73 /
# 149-158 / 65-79 in Amidar, 25-32 / 20-49 / 23-29 in GridWorld over three seeds and more with other action draws; phase 2 repeats an action twice, not four times)
STEPS = {"breakout": (20, 42, 20), "space_invaders": (50, 102, 50), "amidar": (80, 164, 80), "gridworld": (48, 96, 48)}


def phases(game):
    h2, w2 = SECOND_SIZE[game]
    wrappers = dict(clip_reward=True, episodic_life=True, fire_reset=1 in LEGAL[game], noop_max=30, noop_seed=11)
    return [dict(new_plane=0, stack=4, skip=4, out_h=84, out_w=84, **wrappers),
            dict(new_plane=2, stack=2, skip=2, out_h=h2, out_w=w2, **wrappers),
            dict(new_plane=1, stack=4, skip=4, out_h=84, out_w=84, **wrappers)]


def observation(e, cfg, obs):
    """what the engine holds as the observation under cfg, by name"""
    shape = (N, cfg["out_h"], cfg["out_w"])
    if cfg["new_plane"] == 2:
        assert obs is None
        return {"ring": read_buffer(e, _abi.BUF_AGENT_RING, (cfg["stack"],) + shape), "head": np.int64(e.agent_ring_head())}
    out = {"obs": obs.copy()}
    if cfg["new_plane"] == 1:
        out["plane"] = read_buffer(e, _abi.BUF_AGENT_PLANE, shape)
    return out


def run(libs, game, seed, check):
    """the three phases on one engine per library of `libs`, in lockstep; check(what, [outputs of engine 0, of engine 1, ...]) after
    every call, outputs = {name: array} of everything that is compared"""
    rng = np.random.default_rng(seed)
    legal = np.asarray(LEGAL[game], np.int32)
    engines = [Engine(game, N, lib=lib) for lib in libs]
    try:
        for e in engines:
            e.seed(seed)
            e.new_game()
        for p, cfg in enumerate(phases(game)):
            for e in engines:
                e.agent_init(**cfg)
            check("phase %d reset" % p, [observation(e, cfg, e.agent_reset()) for e in engines])
            for t in range(STEPS[game][p]):
                actions = legal[rng.integers(0, len(legal), N)]
                outs = []
                for e in engines:
                    obs, reward, done = e.agent_step(actions)
                    ep_done, ep_return, ep_length = e.agent_episodes()
                    outs.append(dict(observation(e, cfg, obs), reward=reward, done=done, ep_done=ep_done,
                                     ep_return=np.where(ep_done, ep_return, 0), ep_length=np.where(ep_done, ep_length, 0)))
                check("phase %d step %d" % (p, t), outs)            # (the episode records are valid where ep_done is set)
            check("phase %d states" % p, [{"states": states_bytes(e)} for e in engines])
    finally:
        for e in engines:
            e.close()


@pytest.fixture
def fuzz_seed():
    seed = int(os.environ.get("TBX_FUZZ_SEED", 2024))
    print("TBX_FUZZ_SEED=%d" % seed)                # (captured output is shown for a failing test only)
    return seed


@pytest.mark.parametrize("game", GAMES)
def test_reinit_sequence_reaches_done_in_every_phase(oracle_lib, game, fuzz_seed):
    dones, shapes = [0, 0, 0], [None, None, None]

    def check(what, outs):
        p = int(what.split()[1])
        if "done" in outs[0]:
            dones[p] += int(outs[0]["done"].sum())
            shapes[p] = {name: outs[0][name].shape for name in ("obs", "plane", "ring") if name in outs[0]}

    run([oracle_lib], game, fuzz_seed, check)
    assert all(dones), "%s: envs that reported done, by phase: %r" % (game, dones)
    h2, w2 = SECOND_SIZE[game]
    assert (h2, w2) != (84, 84)
    assert shapes == [{"obs": (N, 84, 84, 4)}, {"ring": (2, N, h2, w2)}, {"obs": (N, 84, 84, 4), "plane": (N, 84, 84)}]


@pytest.mark.gpu
@pytest.mark.parametrize("game", GAMES)
def test_gpu_agent_reinit_matches_oracle(hip_lib, oracle_lib, game, fuzz_seed):
    def check(what, outs):
        got, want = outs
        assert sorted(got) == sorted(want), what
        for name in want:
            if not np.array_equal(got[name], want[name]):
                bad = np.argwhere(np.asarray(got[name]) != np.asarray(want[name]))
                raise AssertionError("%s %s: %s differs in %d places, first at %r" % (game, what, name, len(bad), tuple(bad[0])))

    run([hip_lib, oracle_lib], game, fuzz_seed, check)
