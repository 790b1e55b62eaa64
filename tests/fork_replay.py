"""The yardstick of the fork tests (TBX_EDIT_COPY_ENV, include/toybox_amd.h): REPLAY.

The CPU checker cannot fork, and it has no setter for prev_score or for the agent layer's state.  What a fork must produce is
therefore built without one: an engine whose env i is created the way env src[i] was (its seed, its no-op count, the same edits
with their masks permuted) and driven with env src[i]'s actions has, after the same number of steps, env src[i]'s whole state
in slot i -- game, simulator RNG, prev_score, wrapper stack and frame stack.  Envs never interact, so this is an identity of the
checker (tests/test_fork.py checks it where no GPU is), and a forked device engine must continue exactly like it.

Raw(...) / Agent(...) describe one such run: make(lib, src) builds the engine (src None: the original batch), run(e, t0, t1, src)
drives it and returns every output of every step, snapshot(e) what an env is made of."""
import numpy as np

from support import LEGAL, read_buffer, stack_from_ring, synthetic_actions
from toybox_amd import Engine, _abi


def states_bytes(e, first=0, count=None):
    """uint8[count, record size]: every byte tbx_get_states reports"""
    arr = e.get_states(first, count)
    return np.frombuffer(arr, np.uint8).reshape(len(arr), -1).copy()


def sim_rngs(e, envs=None):
    envs = range(e.n_envs) if envs is None else envs
    return np.asarray([e.get_sim_rng(int(i)) for i in envs], np.uint64)


def fork_maps(n, seed=0):
    """name -> (src int[N], mask bool[N] or None): the maps of the issue"""
    rng = np.random.default_rng(seed)
    ar = np.arange(n)
    swap = ar ^ 1
    swap[swap >= n] = n - 1
    maps = {
        "masked_identity": (ar.copy(), ar % 2 == 0),
        "one_to_all": (np.full(n, n // 3), None),
        "reversal": (ar[::-1].copy(), None),
        "swap_pairs": (swap, None),
        "random_repeats": (rng.integers(0, n, n), rng.random(n) < 0.7),
        "some_self": (np.where(ar % 3 == 0, ar, rng.integers(0, n, n)), None),
    }
    return maps


def effective(src, mask):
    """the map a fork realises: unselected envs stay themselves"""
    src = np.asarray(src, np.int64)
    return src if mask is None else np.where(mask, src, np.arange(len(src)))


class Raw:
    """the raw layer: seeds, lives edited to 1 in two thirds of the envs, synthetic actions, auto-reset on"""

    def __init__(self, game, n, seed=1234, action_seed=1337, lives_one=True):
        self.game, self.n, self.action_seed, self.lives_one = game, n, action_seed, lives_one
        self.seeds = (seed + 7 * np.arange(n)).astype(np.uint32)
        self.lives_mask = np.arange(n) % 3 != 0

    def make(self, lib, src=None):
        src = np.arange(self.n) if src is None else np.asarray(src)
        e = Engine(self.game, self.n, lib=lib)
        e.seed_array(self.seeds[src])
        e.new_game()
        if self.lives_one and self.game != "gridworld":
            e.edit(_abi.EDIT_SET_LIVES, [1], mask=self.lives_mask[src])
        return e

    def actions(self, t, src=None):
        a = synthetic_actions(self.game, self.n, t, seed=self.action_seed)
        return a if src is None else a[np.asarray(src)]

    def run(self, e, t0, t1, src=None, frames=0):
        """steps t0 .. t1-1; -> list of (reward, done, lives, score[, frame]) per step"""
        out = []
        for t in range(t0, t1):
            r = e.step(self.actions(t, src), auto_reset=True)
            out.append(tuple(np.asarray(x).copy() for x in r) + ((e.render(frames),) if frames else ()))
        return out


class Agent:
    """the agent layer: every wrapper on, per-env no-op overrides, lives edited to 1 in half the envs after the reset"""

    def __init__(self, game, n, seed=99, action_seed=7, new_plane=0, stack_fill=0, size=84):
        self.game, self.n, self.action_seed = game, n, action_seed
        self.new_plane, self.stack_fill, self.size = new_plane, stack_fill, size
        self.seeds = (seed + 11 * np.arange(n)).astype(np.uint32)
        self.counts = (1 + (5 * np.arange(n) + 3) % 30).astype(np.int32)
        self.lives_mask = np.arange(n) % 2 == 0
        self.fire = 1 in LEGAL[game]

    def make(self, lib, src=None, options=()):
        src = np.arange(self.n) if src is None else np.asarray(src)
        e = Engine(self.game, self.n, lib=lib)
        for opt, val in options:
            e.set_option(opt, val)
        e.seed_array(self.seeds[src])
        e.new_game()
        e.agent_init(skip=4, out_h=self.size, out_w=self.size, stack=4, clip_reward=False, episodic_life=True, fire_reset=self.fire,
                     noop_max=30, noop_seed=5, stack_fill=self.stack_fill, new_plane=self.new_plane)
        e.agent_set_noops(self.counts[src])
        e.agent_reset()
        if self.game != "gridworld":
            e.edit(_abi.EDIT_SET_LIVES, [1], mask=self.lives_mask[src])
        return e

    def own_slots(self, e):
        """after the replay the slots' own configuration again (a fork does not move it)"""
        e.agent_set_noops(self.counts)

    def actions(self, t, src=None):
        a = synthetic_actions(self.game, self.n, t, seed=self.action_seed)
        return a if src is None else a[np.asarray(src)]

    def observation(self, e):
        """uint8[N, h, w, stack] of the current observation, whatever form the device keeps it in"""
        n, s = self.n, self.size
        if self.new_plane == 2:
            return stack_from_ring(read_buffer(e, _abi.BUF_AGENT_RING, (4, n, s, s)), e.agent_ring_head())
        return read_buffer(e, _abi.BUF_AGENT_OBS, (n, s, s, 4))

    def run(self, e, t0, t1, src=None):
        """agent steps t0 .. t1-1; -> rows as rows() returns them"""
        return self.rows(e, (self.actions(t, src) for t in range(t0, t1)))

    def rows(self, e, actions):
        """one agent step per action row given; -> list of (obs, reward, done, ep_done, ep_return, ep_length[, plane]) per step"""
        out = []
        for a in actions:
            _, reward, done = e.agent_step(a)
            ended, ret, length = e.agent_episodes()
            row = (self.observation(e), reward.copy(), done.copy(), ended.copy(), np.where(ended, ret, 0), np.where(ended, length, 0))
            if self.new_plane == 1:
                row += (read_buffer(e, _abi.BUF_AGENT_PLANE, (self.n, self.size, self.size)),)
            out.append(row)
        return out


def snapshot(e):
    return states_bytes(e), sim_rngs(e)


def assert_rows_equal(got, want, what, src=None):
    """two run() results; src: `want` is the ORIGINAL batch, row i of `got` must equal its row src[i]"""
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        for k, (x, y) in enumerate(zip(g, w)):
            y = y if src is None else y[np.asarray(src)]
            if not np.array_equal(x, y):
                bad = np.flatnonzero((np.asarray(x) != np.asarray(y)).reshape(len(x), -1).any(axis=1))
                raise AssertionError("%s: output %d differs at step %d in %d envs, first %s" % (what, k, t, len(bad), bad[:8]))


def assert_snapshot_equal(got, want, what, src=None):
    for name, x, y in zip(("state records", "simulator RNG"), got, want):
        y = y if src is None else y[np.asarray(src)]
        if not np.array_equal(x, y):
            bad = np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))
            raise AssertionError("%s: %s differ in %d envs, first %s" % (what, name, len(bad), bad[:8]))
