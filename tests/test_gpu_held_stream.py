"""The program-order promise and the reader promise of include/toybox_amd.h under a HELD stream.

    1. Calls on one handle take effect in program order, whatever streams they name.
    2. A result in an engine-owned buffer stays valid for whatever the caller has queued on the stream of the call that produced
       it, until the caller's next call on the handle.

At 65 and 257 envs every kernel ends before the host has queued the next call, so on an idle GPU a forgotten join or a missing
fence cannot produce a wrong byte.  Here the stream of call A is held back by a delay kernel (tests/held_stream.py) for four times
as long as the host needs to issue the script: everything queued behind A waits, everything queued elsewhere is free to overtake,
and an ordering the engine owes and forgot shows as wrong bytes, deterministically.

Every case is one ordered script on one device engine and on its oracle twin, run twice on the same engines: pass 1 without a
hold (it warms every lazy allocation and times how long the host takes to issue the script), pass 2 with the stream held for
max(5 ms, 4 x that time) -- the 4 is the margin for host jitter.  Both passes are compared with the oracle, exactly.  Where the
script's last call is asynchronous the case asserts, after that call has returned, that the hold is still running: a case whose
hold has ended proves nothing and FAILS as vacuous.  A hold beyond the tool's 250 ms cap fails too (split the case).

The streams s1 (held) and s2 are a pair for which test_a_held_stream_is_overtaken has SEEN s2 overtake a held s1: the runtime
multiplexes streams onto a few hardware queues, and two streams that share one serialise.  The engine's internal streams cannot be
chosen this way: should one of them share the held queue, a bug stays hidden behind it -- but no correct engine fails for it.

test_the_edges_cannot_pass_vacuously (no GPU) runs every script on two oracle engines, one with call A and one without (a reader
case: one with the reader in its place and one with the reader after B), and asserts that what the case compares differs between
the two in at least half the envs -- else a B that overtook A would go unnoticed.  Per result the shares are printed.  The
overlapped forms' step outputs (reward, done, lives, score of consecutive frames) are sparse by the games' nature and an edit between
two overlapped calls would leave the form: there the frames carry the share, the step outputs are compared all the same.

The checker library has neither TBX_EDIT_COPY_ENV, the checkpoint edits nor any lookahead or planner query: edge c builds its twin
by host writes and tests/lookahead_replay.py, the planner edges e, f, g and the TBX_BUF_PLAN_* readers from the Python replays of
tests/tree_act_replay.py and tests/act_replay.py on the twin's records.
GridWorld has no field edits, so the edges whose A or B is TBX_EDIT_SET_LIVES / _SCORE run on the other three games.
"""
import ctypes as C
import gc
import time

import numpy as np
import pytest

import tree_replay as TR
from support import DONOR_FRAMES, LEGAL, donor_records, synthetic_actions, write_mid_game_states
from toybox_amd import Engine, _abi
from fork_replay import sim_rngs
from lookahead_replay import FIELDS as LOOKAHEAD_FIELDS, expected as lookahead_expected
from act_replay import EVOLVE as ACT_EVOLVE, expected_act
from tree_act_replay import TreeActReplay
from toybox_amd.engine import checkpoint_args, lookahead_args, tree_store_units

GAMES = ("breakout", "space_invaders", "amidar", "gridworld")
SIZES = (65, 257)                                            # a partial wavefront; more than one block
SEED = 1337
MIN_HOLD_US, MARGIN = 5000, 4
STEP_IDS = (("reward", _abi.BUF_REWARD, np.int32), ("done", _abi.BUF_DONE, np.uint8), ("lives", _abi.BUF_LIVES, np.int32),
            ("score", _abi.BUF_SCORE, np.int32), ("packed", _abi.BUF_PACKED, np.uint64))
AGENT_IDS = (("obs", _abi.BUF_AGENT_OBS, np.uint8), ("plane", _abi.BUF_AGENT_PLANE, np.uint8), ("reward", _abi.BUF_AGENT_REWARD, np.float32),
             ("done", _abi.BUF_AGENT_DONE, np.uint8), ("ep_done", _abi.BUF_AGENT_EP_DONE, np.uint8),
             ("ep_return", _abi.BUF_AGENT_EP_RETURN, np.float32), ("ep_length", _abi.BUF_AGENT_EP_LENGTH, np.int32))
AGENT = dict(skip=4, out_h=84, out_w=84, stack=4, clip_reward=False, episodic_life=False, fire_reset=False, noop_max=0, new_plane=1)


@pytest.fixture(scope="module")
def donors(oracle_lib):
    """the mid-game donor records of tests/support.py, computed once per game and never written to"""
    keep = {}

    def get(game):
        if game not in keep:
            keep[game] = donor_records(game, oracle_lib, donors=257) if DONOR_FRAMES[game] else None
            if keep[game] is not None:
                keep[game].flags.writeable = False
        return keep[game]
    return get


# ---------------------------------------------------------------- one engine of a case and the memory its calls name

class Side:
    """the device engine or its oracle twin (the `_pair` of the other GPU tests: same seed, same start states), the two streams,
    and memory for the calls' pointer arguments -- HBM on the device, numpy arrays for the checker, which takes host pointers in
    the "_device" forms and has nothing in flight"""

    def __init__(self, lib, game, n, records, streams=None, agent=None, opts=(), active=None):
        self.is_hip = not hasattr(lib, "orc_splitmix64")
        self.game, self.n, self.lib = game, n, lib
        self.e = e = Engine(game, n, lib=lib)
        e.seed(11)
        e.new_game()
        if records is None:                                  # (GridWorld has no donors: a few frames, so that no two envs stand alike)
            for w in range(12):
                e.step(synthetic_actions(game, n, w, seed=3), auto_reset=True)
        if agent:
            e.agent_init(**agent)
            e.agent_reset()
        write_mid_game_states([e], n, records)
        for opt, val in opts:                                # (the oracle stores launch-time options without effect)
            e.set_option(opt, val)
        self.active = dict(active or {}) if self.is_hip else {}
        self.check_active()
        if self.is_hip:
            self.S1, self.S2 = streams
            self.s1, self.s2 = self.S1.ptr, self.S2.ptr
        else:
            self.S1 = self.S2 = None
            self.s1 = self.s2 = 0
        self.H, self.W = e.height, e.width
        self._mem, self._named = {}, {}

    def check_active(self):
        """the form the case means to exercise is the one the engine runs (TBX_OPT_*_ACTIVE; a host query, nothing is queued):
        asked when the options are set and again behind the script's last call, so that no case falls back to stream order midway"""
        for opt, val in self.active.items():
            assert self.e.get_option(opt) == val, "option %d reads %d, the case needs %d" % (opt, self.e.get_option(opt), val)

    def alloc(self, nbytes, name=None):
        """zeroed memory of the side's kind; with a name the same block on every later call (pass 2 allocates nothing)"""
        if name is not None and name in self._named:
            assert self._named[name][1] >= nbytes
            return self._named[name][0]
        p = self.put(np.zeros(max(int(nbytes), 8), np.uint8))
        if name is not None:
            self._named[name] = (p, nbytes)
        return p

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        if self.is_hip:
            from toybox_amd import hip
            p = hip.malloc(arr.nbytes)
            hip.memcpy_htod(p, arr, arr.nbytes)
            self._mem[p] = None
        else:
            arr = arr.copy()
            p = arr.ctypes.data
            self._mem[p] = arr
        return p

    def fetch(self, ptr, shape, dtype):
        """what lies at ptr, once everything queued has finished"""
        out = np.empty(shape, dtype)
        if self.is_hip:
            from toybox_amd import hip
            hip.memcpy_dtoh(out, ptr, out.nbytes)
        else:
            C.memmove(out.ctypes.data, ptr, out.nbytes)
        return out

    def copy(self, dst, src, nbytes, stream):
        """a device-to-device copy queued on `stream` (the checker: done here)"""
        if self.is_hip:
            from toybox_amd import hip
            hip.memcpy_dtod_async(dst, src, nbytes, stream)
        else:
            C.memmove(dst, src, nbytes)

    def snapshot(self, which, stream, tag=""):
        """tbx_device_buffer now, then a copy of the buffer into the test's own memory queued on `stream` -> (ptr, bytes)"""
        p, nbytes = self.e.device_buffer(which)
        assert p and nbytes, which
        dst = self.alloc(nbytes, "snap %d %s" % (which, tag))
        self.copy(dst, p, nbytes, stream)
        return dst, nbytes

    def buffer(self, which, dtype):
        """an engine-owned buffer as it is once everything queued has finished"""
        p, nbytes = self.e.device_buffer(which)
        return self.fetch(p, (nbytes // np.dtype(dtype).itemsize,), dtype)

    def finish(self):
        if self.is_hip:
            self.S1.synchronize()
            self.S2.synchronize()
        self.e.sync()

    def close(self):
        self.e.close()
        if self.is_hip:
            from toybox_amd import hip
            for p in self._mem:
                hip.free(p)
        self._mem.clear()


def no_hold():
    pass


def states(side):
    return side.e.get_states_np().copy()


def step_outputs(side, res, prefix=""):
    for name, which, dt in STEP_IDS:
        res[prefix + name] = side.buffer(which, dt)


# ---------------------------------------------------------------- the edges
# An edge: games, b_async (the script's last call returns before its work has run), side keywords, setup(side) -> ctx,
# script(side, ctx, p, hold, with_a): pass p's calls in program order, hold() at the point where s1 is to be held (A follows it;
# in a reader case the readers do), and results(side, ctx) -> {name: array or list with one entry per env}, read after everything
# has finished.  key: the results that carry the differs-with-and-without-A share.

class Edge:
    games = GAMES
    b_async = True
    key = None

    def side_keywords(self, game):
        return {}

    def setup(self, s):
        return {}


class StepThenQuery(Edge):
    """(a) step_synthetic on s1 | reduce_device of a state query on s2: the query answers the state after the step"""
    name = "a-step-query"
    games = ("breakout", "space_invaders", "amidar")
    QUERY = {"breakout": _abi.QUERY_BRK_BALLS, "space_invaders": _abi.QUERY_SI_SHIP, "amidar": _abi.QUERY_AMI_PLAYER_TILE}
    STEPS = {"breakout": 1, "space_invaders": 4, "amidar": 12}     # frames until the queried field has moved in half the envs

    def setup(self, s):
        self.width = s.e.reduce_width(self.QUERY[s.game])
        return dict(out=s.alloc(s.n * self.width * 8))

    def script(self, s, c, p, hold, with_a=True):
        hold()
        if with_a:
            for i in range(self.STEPS[s.game]):
                s.e.step_synthetic(SEED, 40 * p + i, auto_reset=True, stream=s.s1)
        s.e.reduce_device(self.QUERY[s.game], c["out"], stream=s.s2)

    def results(self, s, c):
        return dict(rows=s.fetch(c["out"], (s.n, self.width), np.float64))


class EditThenStep(Edge):
    """(b) edit_device SET_LIVES (a shared row) and SET_SCORE (per-env device rows) on s1 | step_device on s2"""
    name = "b-edit-step"
    games = GAMES[:3]                                        # (GridWorld has no field edits)

    def setup(self, s):
        return dict(acts=[s.put(synthetic_actions(s.game, s.n, 100 + p, seed=5)) for p in range(2)],
                    rows=[s.put((1000.0 * (p + 1) + 7 * np.arange(s.n, dtype=np.float64)).reshape(s.n, 1)) for p in range(2)])

    def script(self, s, c, p, hold, with_a=True):
        hold()
        if with_a:
            s.e.edit_device(_abi.EDIT_SET_LIVES, [7 + p], stream=s.s1)
            s.e.edit_device(_abi.EDIT_SET_SCORE, stream=s.s1, per_env_ptr=c["rows"][p], n_args=1)
        s.e.step_device(c["acts"][p], auto_reset=True, stream=s.s2)

    def results(self, s, c):
        res = dict(states=states(s))
        step_outputs(s, res)
        return res

    key = ("lives", "score", "packed", "states")


class CopyThenRender(Edge):
    """(c) edit_device COPY_ENV, CHECKPOINT_SAVE, CHECKPOINT_RESTORE from other rows on s1 | render_device into a caller's buffer
    and reduce_device(LOOKAHEAD_ALL) on s2.  The checker library has neither the env copies nor the lookahead: its twin takes A's
    effect through host state and RNG writes (env i ends as env src[n - 1 - i] was: copied, saved, restored from the mirrored row;
    no step has run since the states were written, so prev_score is the score on both sides), and the lookahead rows are
    tests/lookahead_replay.py played on clones of the twin."""
    name = "c-copy-render"

    def schedule(self, game):
        return dict(frames=2 * TR.HOLD[game], hold=TR.HOLD[game], rest=-1, seed=9, t=3)

    def setup(self, s):
        n, L = s.n, len(LEGAL[s.game])
        self.src = (np.arange(n) * 7 + 3) % n
        if not s.is_hip:
            return {}
        s.e.checkpoint_slots(1)
        rows = checkpoint_args(n, 0, rows=(n - 1 - np.arange(n)))
        self.la = lookahead_args(n, **self.schedule(s.game))[0]
        return dict(src=s.put(self.src.astype(np.float64).reshape(n, 1)), rows=s.put(rows), n_rows=rows.shape[1], frame=s.alloc(n * s.H * s.W * 3),
                    la=s.alloc(n * L * 5 * 8))

    def script(self, s, c, p, hold, with_a=True):
        hold()
        if s.is_hip:
            if with_a:
                s.e.edit_device(_abi.EDIT_COPY_ENV, stream=s.s1, per_env_ptr=c["src"], n_args=1)
                s.e.edit_device(_abi.EDIT_CHECKPOINT_SAVE, [0], stream=s.s1)
                s.e.edit_device(_abi.EDIT_CHECKPOINT_RESTORE, stream=s.s1, per_env_ptr=c["rows"], n_args=c["n_rows"])
            s.e.render_device(c["frame"], 3, stream=s.s2)
            s.e.reduce_device(_abi.QUERY_LOOKAHEAD_ALL, c["la"], self.la, stream=s.s2)
            return
        if with_a:
            m = self.src[s.n - 1 - np.arange(s.n)]
            rec, rngs = s.e.get_states_np().copy(), sim_rngs(s.e)
            s.e.set_states_np(0, rec[m])
            for i in range(s.n):
                s.e.set_sim_rng((int(rngs[m[i]][0]), int(rngs[m[i]][1])), env=i)
        c["frames"] = np.stack([s.e.render_env(i, 3) for i in range(s.n)])
        exp = lookahead_expected(s.lib, s.game, s.e.get_states(), sim_rngs(s.e), self.schedule(s.game), all_actions=True)
        c["rows"] = np.stack([exp[k].astype(np.float64) for k in LOOKAHEAD_FIELDS], axis=2).reshape(s.n, -1)

    def results(self, s, c):
        if not s.is_hip:
            return dict(frames=c["frames"], lookahead=c["rows"], states=states(s))
        return dict(frames=s.fetch(c["frame"], (s.n, s.H, s.W, 3), np.uint8), lookahead=s.fetch(c["la"], (s.n, len(LEGAL[s.game]) * 5), np.float64),
                    states=states(s))

    key = ("frames", "states")


class StepThenFusedAndRollout(Edge):
    """(d) step_device on s1 | render_step_synthetic and rollout_synthetic(k = 2) on s2"""
    name = "d-step-rollout"
    STEPS = {"breakout": 1, "space_invaders": 1, "amidar": 1, "gridworld": 2}

    def setup(self, s):
        for w in range(2):                                   # chunks and fused launches alternate between two sets of buffers: both grow here, none in pass 2
            s.e.render_step_synthetic(SEED, 500 + 3 * w, 0, 3, auto_reset=True, stream=s.s2)
            s.e.rollout_synthetic(SEED, 501 + 3 * w, 2, channels=3, auto_reset=True, stream=s.s2)
        return dict(acts=[[s.put(synthetic_actions(s.game, s.n, 200 + 8 * p + i, seed=5)) for i in range(self.STEPS[s.game])] for p in range(2)])

    def script(self, s, c, p, hold, with_a=True):
        hold()
        if with_a:
            for a in c["acts"][p]:
                s.e.step_device(a, auto_reset=True, stream=s.s1)
        s.e.render_step_synthetic(SEED, 10 + 3 * p, 0, 3, auto_reset=True, stream=s.s2)
        c["frame"] = s.snapshot(_abi.BUF_FRAME, s.S2)
        s.e.rollout_synthetic(SEED, 11 + 3 * p, 2, channels=3, auto_reset=True, stream=s.s2)

    def results(self, s, c):
        n, fb = s.n, s.H * s.W * 3
        assert c["frame"][1] == n * fb
        res = dict(frame=s.fetch(c["frame"][0], (n, fb), np.uint8),
                   rollout_frames=np.moveaxis(s.buffer(_abi.BUF_ROLLOUT_FRAMES, np.uint8).reshape(2, n, fb), 0, 1),
                   rollout_packed=s.buffer(_abi.BUF_ROLLOUT_PACKED, np.uint64).reshape(2, n).T, states=states(s))
        step_outputs(s, res)
        return res

    key = ("frame", "rollout_frames", "states")


# ---- the planner edges.  The checker library answers none of the planner queries: the twin's side of these calls is the Python
# replay of the query (tests/tree_act_replay.py, tests/act_replay.py) on the twin's records, and the twin keeps the store, the
# action buffer and the carry that the device keeps in TBX_BUF_PLAN_*.  A step from TBX_BUF_PLAN_ACTION is one frame of the twin
# under the replay's actions.

def tree_case(game, simulations, t):
    hold = TR.HOLD[game]
    return dict(frames=3 * hold, hold=hold, depth=3, simulations=simulations, explore=TR.EXPLORE[game], rest=-1, seed=9, t=t)


def tree_keywords(case, reuse):
    """the product's keywords of a replay case"""
    return dict(case, rest=None, reuse=reuse)


def twin_tree_call(s, case, reuse):
    r = s.tree.call(s.lib, s.e.get_states(), sim_rngs(s.e), case, int(reuse))
    s.plan_action = r["action"]
    return r["out"]


class TreeActLoop(Edge):
    """(e) reduce_device(LOOKAHEAD_TREE_ACT, reuse = 1) on s1 | step_device(actions = TBX_BUF_PLAN_ACTION) on s2, the query again
    on s1 -- three periods; rows, the action buffer and the store, unit by unit"""
    name = "e-tree-act"

    def sims(self, game):
        return len(LEGAL[game]) + 2

    def setup(self, s):
        if s.is_hip:
            return dict(out=[s.alloc(s.n * 14 * 8) for _ in range(3)])
        s.tree = TreeActReplay(s.game, s.n)
        return dict(rows=[None] * 3)

    def script(self, s, c, p, hold, with_a=True):
        # every pass starts from a host-form call under the OTHER objective: TBX_BUF_PLAN_ACTION holds the survival pick and the
        # store is dead for a reuse under this one -- so without A period 1 plays that pick and finds no tree to start from
        prime = dict(tree_case(s.game, self.sims(s.game), 90 + p), objective=1)
        if s.is_hip:
            s.e.lookahead_tree_act(**dict(tree_keywords(prime, False), objective="survival"))
        else:
            twin_tree_call(s, prime, False)
        case = tree_case(s.game, self.sims(s.game), 10 * p)
        hold()
        for period in range(3):
            at = dict(case, t=10 * p + period)
            if s.is_hip:
                if period:
                    s.e.step_device(s.e.plan_action_ptr, auto_reset=True, stream=s.s2)
                if period or with_a:
                    s.e.lookahead_tree_act_device(c["out"][period], stream=s.s1, **tree_keywords(at, True))
                    c["store%d" % period] = s.snapshot(_abi.BUF_PLAN_TREE, s.S1, tag=str(period))      # the store of every period
            else:
                if period:
                    s.e.step(s.plan_action, auto_reset=True)
                if period or with_a:
                    c["rows"][period] = twin_tree_call(s, at, True)
                    c["store%d" % period] = s.tree.units()

    def rows(self, s, c, k):
        return s.fetch(c["out"][k], (s.n, 14), np.float64) if s.is_hip else c["rows"][k]

    def results(self, s, c):
        res = {"rows%d" % k: self.rows(s, c, k) for k in (1, 2)}
        res.update({"store%d" % k: self.store(s, c, k) for k in (1, 2)})
        res["action"] = s.buffer(_abi.BUF_PLAN_ACTION, np.int32) if s.is_hip else s.plan_action
        res["states"] = states(s)
        return res

    def store(self, s, c, k):
        if not s.is_hip:
            return c["store%d" % k]
        ptr, nbytes = c["store%d" % k]
        return tree_store_units(s.game, s.fetch(ptr, (nbytes,), np.uint8), s.n, self.sims(s.game))

    def results_with_a(self, s, c):
        return dict(rows0=self.rows(s, c, 0), store0=self.store(s, c, 0))

    key = ("store1",)


class TreeDrop(Edge):
    """(f) tree_drop_device(mask_dev) on s1 | LOOKAHEAD_TREE_ACT with reuse = 1 on s2: dropped envs start empty"""
    name = "f-tree-drop"

    def sims(self, game):
        return 2 * len(LEGAL[game])

    def setup(self, s):
        mask = np.arange(s.n) % 4 != 1
        case = tree_case(s.game, self.sims(s.game), 4)
        if s.is_hip:
            s.e.lookahead_tree_act(**tree_keywords(case, False))
            return dict(out=s.alloc(s.n * 14 * 8), mask=s.put(mask.astype(np.uint8)))
        s.tree = TreeActReplay(s.game, s.n)
        twin_tree_call(s, case, False)
        return dict(mask=mask)

    def script(self, s, c, p, hold, with_a=True):
        case = tree_case(s.game, self.sims(s.game), 4)
        hold()
        if s.is_hip:
            if with_a:
                s.e.tree_drop_device(c["mask"], stream=s.s1)
            s.e.lookahead_tree_act_device(c["out"], stream=s.s2, **tree_keywords(case, True))
            return
        if with_a:
            assert s.tree.drop(c["mask"])
        c["rows"] = twin_tree_call(s, case, True)

    def results(self, s, c):
        if s.is_hip:
            return dict(rows=s.fetch(c["out"], (s.n, 14), np.float64), action=s.buffer(_abi.BUF_PLAN_ACTION, np.int32),
                        store=tree_store_units(s.game, s.buffer(_abi.BUF_PLAN_TREE, np.uint8), s.n, self.sims(s.game)))
        return dict(rows=c["rows"], action=s.plan_action, store=s.tree.units())

    key = ("rows", "store")


def act_case(game, t, seed=9):
    hold = TR.HOLD[game]
    return dict(frames=3 * hold, hold=hold, depth=3, objective=0, rest=-1, seed=seed, t=t, population=4, generations=1, elite=2, mutation=128, plan_seed=seed)


def act_keywords(case):
    """the product's keywords of a replay case"""
    return dict(case, rest=None, objective="return")


def twin_act_call(s, case):
    out, s.plan_action, s.plan_carry, _ = expected_act(s.lib, s.game, s.e.get_states(), sim_rngs(s.e), ACT_EVOLVE, case, carry=getattr(s, "plan_carry", None))
    return out


class ActLoop(Edge):
    """(g) lookahead_act_device (query 159, the evolution) on s1 | step_device(TBX_BUF_PLAN_ACTION) on s2, 159 with init = -2 on s1"""
    name = "g-act-carry"

    def setup(self, s):
        if s.is_hip:
            s.e.lookahead_act("evolve", **act_keywords(act_case(s.game, 90, seed=1)))
            return dict(out=[s.alloc(s.n * 11 * 8) for _ in range(2)])
        twin_act_call(s, act_case(s.game, 90, seed=1))
        return dict(rows=[None, None])

    def script(self, s, c, p, hold, with_a=True):
        # the second call is the carried plan itself (one member, no generation): its row differs wherever the carry does
        first, second = act_case(s.game, 10 * p, seed=9 + p), dict(act_case(s.game, 10 * p + 1), init=-2, population=1, generations=0, elite=1)
        hold()
        if s.is_hip:
            if with_a:
                s.e.lookahead_act_device("evolve", c["out"][0], stream=s.s1, **act_keywords(first))
            s.e.step_device(s.e.plan_action_ptr, auto_reset=True, stream=s.s2)
            s.e.lookahead_act_device("evolve", c["out"][1], stream=s.s1, **act_keywords(second))
            return
        if with_a:
            c["rows"][0] = twin_act_call(s, first)
        s.e.step(s.plan_action, auto_reset=True)
        c["rows"][1] = twin_act_call(s, second)

    def results(self, s, c):
        if s.is_hip:
            return dict(rows1=s.fetch(c["out"][1], (s.n, 11), np.float64), action=s.buffer(_abi.BUF_PLAN_ACTION, np.int32),
                        carry=s.buffer(_abi.BUF_PLAN_CARRY, np.uint32), states=states(s))
        return dict(rows1=c["rows"][1], action=s.plan_action, carry=s.plan_carry, states=states(s))

    def results_with_a(self, s, c):
        return dict(rows0=s.fetch(c["out"][0], (s.n, 11), np.float64) if s.is_hip else c["rows"][0])

    key = ("rows1", "carry", "states")


class PlanReaders(Edge):
    """lookahead_act_device on s1, readers of TBX_BUF_PLAN_ACTION and TBX_BUF_PLAN_CARRY | the query at another time, under another
    seed, on s2.  with_a = False (the CPU check): the readers come after B."""
    name = "r-plan-action"
    IDS = (("action", _abi.BUF_PLAN_ACTION, np.int32), ("carry", _abi.BUF_PLAN_CARRY, np.uint32))

    def setup(self, s):
        if s.is_hip:
            s.e.lookahead_act("evolve", **act_keywords(act_case(s.game, 90, seed=1)))
            return dict(out=[s.alloc(s.n * 11 * 8) for _ in range(2)])
        twin_act_call(s, act_case(s.game, 90, seed=1))
        return {}

    def read(self, s, c, stream):
        if s.is_hip:
            c["snaps"] = {name: s.snapshot(which, stream) + (dt,) for name, which, dt in self.IDS}
        else:
            c["read"] = dict(action=s.plan_action.copy(), carry=s.plan_carry.copy())

    def script(self, s, c, p, hold, with_a=True):
        calls = (act_case(s.game, 10 * p), act_case(s.game, 10 * p + 5, seed=77))
        if s.is_hip:
            s.e.lookahead_act_device("evolve", c["out"][0], stream=s.s1, **act_keywords(calls[0]))
        else:
            twin_act_call(s, calls[0])
        hold()
        if with_a:
            self.read(s, c, s.S1)
        if s.is_hip:
            s.e.lookahead_act_device("evolve", c["out"][1], stream=s.s2, **act_keywords(calls[1]))
        else:
            twin_act_call(s, calls[1])
        if not with_a:
            self.read(s, c, s.S2)

    def results(self, s, c):
        if s.is_hip:
            return {name: s.fetch(ptr, (s.n,), dt) for name, (ptr, nbytes, dt) in c["snaps"].items()}
        return c["read"]

    key = ("action", "carry")


class AgentSteps(Edge):
    """(h) agent_step_device on s1 | edit_device(SET_LIVES) on s2, agent_step_synthetic on s1"""
    name = "h-agent"
    games = GAMES[:3]

    def side_keywords(self, game):
        return dict(agent=AGENT)

    def setup(self, s):
        return dict(acts=[s.put(synthetic_actions(s.game, s.n, 300 + p, seed=5)) for p in range(2)])

    def script(self, s, c, p, hold, with_a=True):
        hold()
        if with_a:
            s.e.agent_step_device(c["acts"][p], stream=s.s1)
        s.e.edit_device(_abi.EDIT_SET_LIVES, [7 + p], stream=s.s2)
        s.e.agent_step_synthetic(SEED, 20 + p, stream=s.s1)

    def results(self, s, c):
        res = {name: s.buffer(which, dt).reshape(s.n, -1) for name, which, dt in AGENT_IDS}
        res["states"] = states(s)
        return res

    key = ("obs", "plane", "states")


class HostForms(Edge):
    """(i) step_synthetic on s1 | a host-pointer form -- get_states, reduce, scalars, render_env, or sync and a raw copy of
    TBX_BUF_PACKED -- reads the values after the step; one case per form, since the first of them drains the hold"""
    b_async = False
    STEPS = {"breakout": 1, "space_invaders": 4, "amidar": 12, "gridworld": 2}
    QUERY = dict(StepThenQuery.QUERY)

    def __init__(self, form):
        self.form, self.name = form, "i-host-" + form
        if form == "reduce":
            self.games = StepThenQuery.games
        elif form in ("scalars", "sync_copy"):
            self.games = GAMES[:3]                           # (no edit of GridWorld moves lives or score within two frames)

    def script(self, s, c, p, hold, with_a=True):
        e = s.e
        hold()
        if with_a:
            if s.game != "gridworld":
                e.edit_device(_abi.EDIT_SET_LIVES, [7 + p], stream=s.s1)
            for i in range(self.STEPS[s.game]):
                e.step_synthetic(SEED, 40 * p + i, auto_reset=True, stream=s.s1)
        if self.form == "get_states":
            c["got"] = dict(states=states(s))
        elif self.form == "reduce":
            c["got"] = dict(rows=e.reduce(self.QUERY[s.game]))
        elif self.form == "scalars":
            sc = e.scalars()
            c["got"] = dict(score=np.asarray(sc[0]), lives=np.asarray(sc[1]))
        elif self.form == "render_env":
            c["got"] = dict(frames=np.stack([e.render_env(i, 3) for i in range(s.n)]))
        else:
            e.sync()
            c["got"] = dict(lives=s.buffer(_abi.BUF_LIVES, np.int32), packed=s.buffer(_abi.BUF_PACKED, np.uint64))

    def results(self, s, c):
        return c["got"]


class GatherBehindStep(Edge):
    """(j) SET_LIVES in every env, K x step_synthetic and gather into a caller's block on s1 | SET_LIVES in the odd envs, K steps
    and a gather on s2: each gathered block equals the own records of its K steps (one rank; K = 1, and a K = 2 ring).  B's block
    carries A's lives in the even envs -- more than half -- and B's own in the odd ones, where a step of B that overtook A's
    gather would show in A's block."""
    games = ("breakout", "amidar")

    def __init__(self, every):
        self.every, self.name = every, "j-gather-K%d" % every

    def setup(self, s):
        s.e.set_option(_abi.OPT_GATHER_EVERY, self.every)
        s.e.gather_init(1, 0, s.e.gather_unique_id(), records_per_rank=s.n)
        return dict(out=[s.alloc(self.every * s.n * 8) for _ in range(2)], odd=s.put((np.arange(s.n) % 2 == 1).astype(np.uint8)))

    def script(self, s, c, p, hold, with_a=True):
        hold()
        for k, stream, lives, mask in ((0, s.s1, 7 + p, 0), (1, s.s2, 3 + p, c["odd"])):
            if k == 0 and not with_a:
                continue
            s.e.edit_device(_abi.EDIT_SET_LIVES, [lives], mask_ptr=mask, stream=stream)
            for i in range(self.every):
                s.e.step_synthetic(SEED, 50 * p + 10 * k + i, auto_reset=True, stream=stream)
            s.e.gather(c["out"][k], stream=stream)

    def results(self, s, c):
        return dict(block_b=s.fetch(c["out"][1], (self.every, s.n), np.uint64).T, states=states(s))

    def results_with_a(self, s, c):
        return dict(block_a=s.fetch(c["out"][0], (self.every, s.n), np.uint64).T)

    key = ("block_b",)


# ---- reader cases: the second promise.  A on s1; s1 is held; copies of the buffers A produced go onto s1 into the test's own
# memory; B rewrites those buffers.  The copies must hold A's values.  with_a = False (the CPU check): the copies are taken after B.

class Readers(Edge):
    def results(self, s, c):
        return {name: s.fetch(ptr, (s.n, nbytes // (s.n * np.dtype(dt).itemsize)), dt) for name, (ptr, nbytes, dt) in c["snaps"].items()}

    def read(self, s, c, ids, stream):
        c["snaps"] = {}
        for name, which, dt in ids:
            p, nbytes = s.snapshot(which, stream)
            c["snaps"][name] = (p, nbytes, dt)


class StepOutputReaders(Readers):
    """step_synthetic + render_device(NULL) on s1, readers of TBX_BUF_REWARD .. TBX_BUF_PACKED and TBX_BUF_FRAME | SET_LIVES,
    SET_SCORE, step_synthetic, render_device(NULL) on s2 -- stream order, no overlapped form"""
    name = "r-step-outputs"
    games = GAMES[:3]
    IDS = STEP_IDS + (("frame", _abi.BUF_FRAME, np.uint8),)

    def side_keywords(self, game):
        return dict(opts=[(_abi.OPT_PIPELINE, 0), (_abi.OPT_FUSED_OVERLAP, _abi.FUSED_OVERLAP_OFF), (_abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_OFF)],
                    active={_abi.OPT_PIPELINE_ACTIVE: 0, _abi.OPT_FUSED_OVERLAP_ACTIVE: 0, _abi.OPT_ROLLOUT_CHUNKS_ACTIVE: 0})

    def setup(self, s):
        return dict(rows=[s.put((5000.0 * (p + 1) + 3 * np.arange(s.n, dtype=np.float64)).reshape(s.n, 1)) for p in range(2)])

    def script(self, s, c, p, hold, with_a=True):
        e = s.e
        e.step_synthetic(SEED, 8 * p, auto_reset=True, stream=s.s1)
        e.render_device(0, 3, stream=s.s1)
        hold()
        if with_a:
            self.read(s, c, self.IDS, s.S1)
        e.edit_device(_abi.EDIT_SET_LIVES, [7 + p], stream=s.s2)
        e.edit_device(_abi.EDIT_SET_SCORE, stream=s.s2, per_env_ptr=c["rows"][p], n_args=1)
        for i in range(3):
            e.step_synthetic(SEED, 8 * p + 1 + i, auto_reset=True, stream=s.s2)
        e.render_device(0, 3, stream=s.s2)
        if not with_a:
            self.read(s, c, self.IDS, s.S2)

    key = ("lives", "score", "packed", "frame")


class RolloutReaders(Readers):
    """rollout_synthetic(k = 2) as single calls on s1, readers of TBX_BUF_ROLLOUT_FRAMES / _PACKED | the next two chunks on s2"""
    name = "r-rollout-fallback"
    IDS = (("rollout_frames", _abi.BUF_ROLLOUT_FRAMES, np.uint8), ("rollout_packed", _abi.BUF_ROLLOUT_PACKED, np.uint64))

    def side_keywords(self, game):
        return dict(opts=[(_abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_OFF)], active={_abi.OPT_ROLLOUT_CHUNKS_ACTIVE: 0})

    def script(self, s, c, p, hold, with_a=True):
        s.e.rollout_synthetic(SEED, 20 * p, 2, channels=3, auto_reset=True, stream=s.s1)
        hold()
        if with_a:
            self.read(s, c, self.IDS, s.S1)
        for i in (1, 2):
            s.e.rollout_synthetic(SEED, 20 * p + 4 * i, 2, channels=3, auto_reset=True, stream=s.s2)
        if not with_a:
            self.read(s, c, self.IDS, s.S2)

    def results(self, s, c):
        n = s.n
        p, nbytes, _ = c["snaps"]["rollout_frames"]
        q, qbytes, _ = c["snaps"]["rollout_packed"]
        return dict(rollout_frames=np.moveaxis(s.fetch(p, (2, n, nbytes // (2 * n)), np.uint8), 0, 1), rollout_packed=s.fetch(q, (2, n), np.uint64).T)

    key = ("rollout_frames",)


class AgentReaders(Readers):
    """agent_step_device on s1, readers of TBX_BUF_AGENT_OBS / _PLANE / _REWARD (and the rest) | agent_step_synthetic x 2 on s2"""
    name = "r-agent"
    IDS = AGENT_IDS

    def side_keywords(self, game):
        return dict(agent=AGENT)

    def setup(self, s):
        return dict(acts=[s.put(synthetic_actions(s.game, s.n, 300 + p, seed=5)) for p in range(2)])

    def script(self, s, c, p, hold, with_a=True):
        s.e.agent_step_device(c["acts"][p], stream=s.s1)
        hold()
        if with_a:
            self.read(s, c, self.IDS, s.S1)
        for i in range(2):
            s.e.agent_step_synthetic(SEED, 20 + 4 * p + i, stream=s.s2)
        if not with_a:
            self.read(s, c, self.IDS, s.S2)

    key = ("obs", "plane")


class FormReaders(Readers):
    """The reader cases under an overlapped form, by the reader rule the header gives those forms: tbx_device_buffer is asked AFTER
    the call, readers go on the call's own stream, and so do the next calls -- their launches run on the engine's internal
    lanes, which a hold on the caller's stream does not stop.  form: "pipeline2" / "pipeline3" (step_synthetic + render_device),
    "fused" (render_step_synthetic), "chunks" (rollout_synthetic, k = 2).
    entry = True is the scenario of ADVICE.md (round 6, first item): the producing call, tbx_sync, THEN the addresses, the hold, the
    readers, three overlapped calls -- the pipeline is entered anew with a reader already queued on the caller's stream."""
    games = ("breakout", "space_invaders")

    FORMS = {"pipeline2": ([(_abi.OPT_PIPELINE, 2), (_abi.OPT_FUSED_OVERLAP, 2), (_abi.OPT_ROLLOUT_CHUNKS, 2)], {_abi.OPT_PIPELINE_ACTIVE: 2}),
             "pipeline3": ([(_abi.OPT_PIPELINE, 3), (_abi.OPT_FUSED_OVERLAP, 2), (_abi.OPT_ROLLOUT_CHUNKS, 2)], {_abi.OPT_PIPELINE_ACTIVE: 3}),
             "fused": ([(_abi.OPT_FUSED_OVERLAP, 1), (_abi.OPT_ROLLOUT_CHUNKS, 2)], {_abi.OPT_FUSED_OVERLAP_ACTIVE: 1, _abi.OPT_PIPELINE_ACTIVE: 0}),
             "chunks": ([(_abi.OPT_ROLLOUT_CHUNKS, _abi.ROLLOUT_CHUNKS_PER_FRAME), (_abi.OPT_FUSED_OVERLAP, 2)], {_abi.OPT_ROLLOUT_CHUNKS_ACTIVE: 1})}

    def __init__(self, form, entry=False):
        self.form, self.entry = form, entry
        self.name = ("r-entry-" if entry else "r-form-") + form
        if form == "fused":
            self.games = ("breakout",)                       # (the one game with a fused launch to overlap)
        self.ids = STEP_IDS + (("frame", _abi.BUF_FRAME, np.uint8),)
        if form == "chunks":
            self.ids += RolloutReaders.IDS
        self.key = ("frame",)

    def side_keywords(self, game):
        opts, active = self.FORMS[self.form]
        return dict(opts=opts, active=active)

    def call(self, s, t):
        e = s.e
        if self.form in ("pipeline2", "pipeline3"):
            e.step_synthetic(SEED, t, auto_reset=True, stream=s.s1)
            e.render_device(0, 3, stream=s.s1)
        elif self.form == "fused":
            e.render_step_synthetic(SEED, t, 0, 3, auto_reset=True, stream=s.s1)
        else:
            e.rollout_synthetic(SEED, 2 * t, 2, channels=3, auto_reset=True, stream=s.s1)

    def script(self, s, c, p, hold, with_a=True):
        for i in range(2):                                   # the form is running when the producing call is made
            self.call(s, 10 * p + i)
        if self.entry:
            s.e.sync()
        hold()
        if with_a:
            self.read(s, c, self.ids, s.S1)
        for i in range(3):
            self.call(s, 10 * p + 2 + i)
        if not with_a:
            self.read(s, c, self.ids, s.S1)

    def results(self, s, c):
        res = {}
        for name, (ptr, nbytes, dt) in c["snaps"].items():
            if name.startswith("rollout"):
                res[name] = np.moveaxis(s.fetch(ptr, (2, s.n, nbytes // (2 * s.n * np.dtype(dt).itemsize)), dt), 0, 1)
            else:
                res[name] = s.fetch(ptr, (s.n, nbytes // (s.n * np.dtype(dt).itemsize)), dt)
        return res


EDGES = ([StepThenQuery(), EditThenStep(), CopyThenRender(), StepThenFusedAndRollout(), TreeActLoop(), TreeDrop(), ActLoop(), AgentSteps()]
         + [HostForms(f) for f in ("get_states", "reduce", "scalars", "render_env", "sync_copy")] + [GatherBehindStep(1), GatherBehindStep(2)]
         + [StepOutputReaders(), RolloutReaders(), AgentReaders(), PlanReaders()]
         + [FormReaders(f) for f in ("pipeline2", "pipeline3", "fused", "chunks")] + [FormReaders(f, entry=True) for f in ("pipeline2", "pipeline3", "fused", "chunks")])
CASES = [(edge, game) for edge in EDGES for game in edge.games]
CASE_IDS = ["%s-%s" % (edge.name, game) for edge, game in CASES]


# ---------------------------------------------------------------- comparing

def env_rows(value, n):
    """one comparable row per env: bytes of an array with n leading entries, or the entries of a list"""
    if isinstance(value, list):
        assert len(value) == n
        return value
    a = np.ascontiguousarray(value)
    assert a.shape[0] == n, a.shape
    return a.reshape(n, -1).view(np.uint8) if a.size else a.reshape(n, 0)


def differing_envs(got, want, n):
    g, w = env_rows(got, n), env_rows(want, n)
    if isinstance(g, list):
        return np.array([g[i] != w[i] for i in range(n)])
    assert g.shape == w.shape, (g.shape, w.shape)
    return (g != w).any(axis=1)


def assert_same(got, want, n, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    bad = []
    for name in got:
        d = differing_envs(got[name], want[name], n)
        if d.any():
            bad.append("%s: %s differs from the oracle in %d of %d envs, first env %d" % (what, name, int(d.sum()), n, int(np.flatnonzero(d)[0])))
    assert not bad, "\n".join(bad)


def all_results(edge, s, c, with_a=True):
    res = edge.results(s, c)
    if with_a and hasattr(edge, "results_with_a"):
        res.update(edge.results_with_a(s, c))
    return res


# ---------------------------------------------------------------- the CPU check: no edge can pass vacuously

@pytest.mark.parametrize("edge,game", CASES, ids=CASE_IDS)
def test_the_edges_cannot_pass_vacuously(edge, game, oracle_lib, donors):
    """On two oracle engines, one with A and one without (reader cases: the reader in its place / after B), what the case compares
    differs in at least half the envs: a B that overtook A, or a reader that saw B's bytes, cannot equal the oracle by accident."""
    n = SIZES[0]
    for p in range(2):                                       # pass 2 starts where pass 1 -- the whole script, A included -- leaves both engines
        sides = [Side(oracle_lib, game, n, donors(game), **edge.side_keywords(game)) for _ in range(2)]
        try:
            ctx = [edge.setup(s) for s in sides]
            for s, c, with_a in zip(sides, ctx, (True, False)):
                for q in range(p):
                    edge.script(s, c, q, no_hold)
                edge.script(s, c, p, no_hold, with_a=with_a)
            res = [all_results(edge, s, c, with_a=False) for s, c in zip(sides, ctx)]
            shares = {name: int(differing_envs(res[0][name], res[1][name], n).sum()) for name in res[0]}
            print("VACUITY %s %s pass %d: envs of %d that differ: %s" % (edge.name, game, p + 1, n, shares))
            keys = edge.key or tuple(res[0])
            union = np.zeros(n, bool)
            for name in keys:
                union |= differing_envs(res[0][name], res[1][name], n)
            assert 2 * int(union.sum()) >= n, "%s %s pass %d: only %d of %d envs differ in %r" % (edge.name, game, p + 1, int(union.sum()), n, keys)
        finally:
            for s in sides:
                s.close()


# ---------------------------------------------------------------- the GPU side

@pytest.fixture(scope="module")
def overtaking_pair(hip_lib):
    """(s1, s2, tried): up to 8 streams; the first pair for which a device-to-device copy on s2 completed while the event behind a
    hold on s1 still answered hipErrorNotReady -- two streams on different hardware queues.  (None, None, tried) if there is none."""
    from held_stream import Held
    from toybox_amd import hip
    streams, bufs, done = [], [], None
    try:
        streams = [hip.Stream() for _ in range(8)]
        bufs = [hip.malloc(1 << 16), hip.malloc(1 << 16)]
        done = hip.Event()
        found, tried = (None, None), 0
        for i in range(len(streams)):
            for j in range(len(streams)):
                if i == j or found[0] is not None:
                    continue
                tried += 1
                h = Held(streams[i], 20000)
                try:
                    with h:
                        hip.memcpy_dtod_async(bufs[1], bufs[0], 1 << 16, streams[j])
                        done.record(streams[j])
                        done.synchronize()
                        overtaken = h.in_flight()
                    h.observed_ms()
                finally:
                    h.close()
                if overtaken:
                    found = (streams[i], streams[j])
        hip.synchronize()
        yield found + (tried,)
    finally:
        hip.synchronize()
        for b in bufs:
            hip.free(b)
        if done is not None:
            done.close()
        for s in streams:
            s.close()


@pytest.mark.gpu
def test_a_held_stream_is_overtaken(overtaking_pair):
    """The hold has teeth: there is a pair of streams of which one overtakes the other while it is held, and a hold lasts at least
    0.8 of what was asked for, by events around it."""
    from held_stream import Held
    s1, s2, tried = overtaking_pair
    assert s1 is not None, "no pair among 8 streams (%d tried) on which a copy overtook a 20 ms hold: every stream shares one hardware queue" % tried
    for us in (5000, 40000):
        with Held(s1, us) as h:
            pass
        ms = h.observed_ms()
        h.close()
        print("HOLD asked %d us observed %.0f us (pair found after %d tries)" % (us, ms * 1000, tried))
        assert ms * 1000 >= 0.8 * us, "a hold of %d us lasted %.0f us" % (us, ms * 1000)
        assert ms * 1000 <= 2 * us + 2000, "a hold of %d us lasted %.0f us" % (us, ms * 1000)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("edge,game", CASES, ids=CASE_IDS)
def test_program_order_under_a_held_stream(edge, game, n, hip_lib, oracle_lib, donors, overtaking_pair):
    """One edge on the device engine and its oracle twin: pass 1 without a hold, pass 2 with s1 held (module docstring).  The
    r-entry cases are the ones that need pipe_enter to fence the caller's stream on the first call of a stay."""
    from held_stream import MAX_HOLD_US, Held
    s1, s2, _ = overtaking_pair
    assert s1 is not None, "no overtaking pair of streams: see test_a_held_stream_is_overtaken"
    kw = edge.side_keywords(game)
    g = Side(hip_lib, game, n, donors(game), streams=(s1, s2), **kw)
    o = Side(oracle_lib, game, n, donors(game), **kw)
    what = "%s %s %d envs" % (edge.name, game, n)
    held = []
    try:
        # the twin first, both passes: the checker's OpenMP workers spin for a while behind every parallel loop, and a host that
        # issues pass 2 beside sixteen spinning threads is not the host pass 1 timed
        co = edge.setup(o)
        want = []
        for p in range(2):
            edge.script(o, co, p, no_hold)
            want.append(all_results(edge, o, co))
        cg = edge.setup(g)
        g.finish()
        t0 = time.perf_counter()                             # pass 1: no hold; every lazy allocation happens here
        edge.script(g, cg, 0, no_hold)
        issue_us = (time.perf_counter() - t0) * 1e6
        g.check_active()
        g.finish()
        assert_same(all_results(edge, g, cg), want[0], n, what + ", pass 1 (no hold)")
        us = max(MIN_HOLD_US, int(MARGIN * issue_us))
        assert us <= MAX_HOLD_US, "%s: the script took %.0f us to issue; a hold of %d us is beyond the cap -- split the case" % (what, issue_us, us)
        began = []

        def start_hold():
            held.append(Held(g.S1, us).__enter__())
            began.append(time.perf_counter())
        gc.collect()
        gc.disable()                                         # (no collector pause between the hold and the question whether it still runs)
        try:
            edge.script(g, cg, 1, start_hold)                # pass 2: s1 held
            alive = held[0].in_flight()                      # ... and still held now that the last call has returned?
            behind_us = (time.perf_counter() - began[0]) * 1e6
            g.check_active()
        finally:
            gc.enable()
        g.finish()
        observed_us = held[0].observed_ms() * 1000
        print("HELD %s | issue %.0f us | asked %d us | observed %.0f us | calls behind the hold issued in %.0f us | %s" % (
              what, issue_us, us, observed_us, behind_us, "still held after the last call" if alive else "hold over" if edge.b_async else "drained by the host form"))
        assert observed_us >= 0.8 * us, "%s: a hold of %d us lasted %.0f us" % (what, us, observed_us)
        if edge.b_async:
            assert alive, "%s: VACUOUS -- the %d us hold had ended when the last call returned, %.0f us after it was queued" % (what, us, behind_us)
        assert_same(all_results(edge, g, cg), want[1], n, what + ", pass 2 (s1 held)")
    finally:
        for h in held:
            h.close()
        g.close()
        o.close()
