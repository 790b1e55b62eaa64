"""The yardstick of the checkpoint tests (TBX_EDIT_CHECKPOINT_*, include/toybox_amd.h): REPLAY ACROSS TIME.

The CPU checker has no checkpoints and needs none.  After a restore at step t_r of cells saved at step t_s, a restored env i must
be, bit for bit, env r = row_i of the original batch as it was at t_s -- which is slot i of a checker engine made with
case.make(lib, eff) (tests/fork_replay.py: env i created the way env eff[i] was) and driven 0 .. t_s with actions(t, eff).  An env
that was not selected must be env i of the original batch at t_r.  Envs never interact, so both are identities of the checker
(tests/test_checkpoint.py checks them where no GPU is).  Twin puts the two checker engines together, row by row, into the batch
the device engine must equal from the restore on; from there every engine plays the action rows the test assembles."""
import numpy as np

from fork_replay import sim_rngs, states_bytes


def pick_rows(sel, a, b):
    """row i of a where sel[i], else of b"""
    a, b = np.asarray(a), np.asarray(b)
    return np.where(np.asarray(sel).reshape((-1,) + (1,) * (a.ndim - 1)), a, b)


class Solo:
    """one checker engine behind Twin's interface"""

    def __init__(self, engine):
        self.e = engine

    def step(self, actions):
        return tuple(np.asarray(x).copy() for x in self.e.step(actions, auto_reset=True))

    def render(self, channels):
        return self.e.render(channels)

    def snapshot(self):
        return states_bytes(self.e), sim_rngs(self.e)


class Twin:
    """the expected batch after a restore: env i is engine `restored`'s where sel[i], engine `others`' elsewhere"""

    def __init__(self, restored, others, sel):
        self.a, self.b, self.sel = restored, others, np.asarray(sel, bool)

    def pick(self, x, y):
        return pick_rows(self.sel, x, y)

    def step(self, actions):
        ra, rb = self.a.step(actions, auto_reset=True), self.b.step(actions, auto_reset=True)
        return tuple(self.pick(x, y) for x, y in zip(ra, rb))

    def render(self, channels):
        return self.pick(self.a.render(channels), self.b.render(channels))

    def snapshot(self):
        return self.pick(states_bytes(self.a), states_bytes(self.b)), self.pick(sim_rngs(self.a), sim_rngs(self.b))

    # ---- the agent layer (case: fork_replay.Agent)
    def observation(self, case):
        return self.pick(case.observation(self.a), case.observation(self.b))

    def agent_rows(self, case, actions):
        """one agent step of both engines per action row; -> rows as Agent.rows returns them"""
        ra, rb = case.rows(self.a, actions), case.rows(self.b, actions)
        return [tuple(self.pick(x, y) for x, y in zip(p, q)) for p, q in zip(ra, rb)]


def restore_map(n, src, sel):
    """(rows int[N], eff int[N]) of a restore of the envs sel from rows src: an unselected env's row entry is a row outside the
    batch (the mask must keep it from being read), and it stays itself"""
    sel = np.asarray(sel, bool)
    rows = np.where(sel, np.asarray(src, np.int64), n + 5)
    return rows, np.where(sel, np.asarray(src, np.int64), np.arange(n))


def mixed_actions(case, sel, eff, t_s, t_r, k):
    """the action row k steps after the restore: restored envs play actions(t_s + k, eff), the others actions(t_r + k)"""
    return np.where(sel, case.actions(t_s + k, eff), case.actions(t_r + k)).astype(np.int32)


def replay_to(case, lib, eff, t_s, run=None):
    """the checker engine whose slot i is env eff[i] of the original batch at step t_s"""
    e = case.make(lib, eff)
    (run or case.run)(e, 0, t_s, eff)
    if hasattr(case, "own_slots"):
        case.own_slots(e)
    return e
