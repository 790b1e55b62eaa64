"""Batched env with the VecEnv contract of the reference's vendored baselines
(/root/reference/baselines/baselines/common/vec_env/__init__.py:26-131): reset() -> obs[N,...];
step_async(actions[N]); step_wait() -> (obs, rews float32, dones bool, infos); a done env is reset and
the returned obs is the reset obs (dummy_vec_env.py:51-54, subproc_vec_env.py:11-15).  The N worker
processes + pipes of SubprocVecEnv collapse into one device batch: one step kernel + one render kernel."""
import time

import numpy as np

from .. import _abi
from ..engine import Engine
from ..games import codec
from ..toybox import _make_engine
from .base import hash_seed
from .spaces import Box, Discrete


class LazyInfos:
    """The per-env info dicts of a VecEnv step as a read-only sequence that builds a dict only when one is asked for:
    65 536 Python dicts per step would cost more host time than the whole device step.  Indexing, iteration and len()
    behave like the list of dicts baselines expects (`for info in infos: info.get('episode')`)."""

    def __init__(self, n, columns=None, extras=None):
        self._n = int(n)
        self._columns = columns or {}        # key -> array[N]
        self._extras = extras or {}          # env index -> dict of additional keys

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(self._n))]
        i = int(i)
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        d = {k: v[i].item() for k, v in self._columns.items()}
        d.update(self._extras.get(i, ()))
        return d

    def __iter__(self):
        return (self[i] for i in range(self._n))

    def with_key(self, key):
        """{env index: value} of the envs whose info carries `key` -- e.g. infos.with_key('episode') -- without walking N dicts"""
        if key in self._columns:
            return {i: self._columns[key][i].item() for i in range(self._n)}
        return {i: d[key] for i, d in self._extras.items() if key in d}


def _pool_size(obs_pool, reuse_obs_buffer):
    """obs_pool with the older reuse_obs_buffer spelling folded in (True: one array, False: a fresh array per call)"""
    if reuse_obs_buffer is not None:
        return 1 if reuse_obs_buffer else 0
    p = int(obs_pool)
    if p < 0:
        raise ValueError("obs_pool must be >= 0")
    return p


def _lookahead(env, frames, hold, first, rest, all_actions, seed, t):
    """Engine.lookahead / lookahead_all for an adapter: action indices -> ALE ids going in, nothing to map coming out (the
    candidates of lookahead_all are in action-index order: the action set is the engine's legal set, sorted as it already is)"""
    def ale(a):
        if a is None:
            return None
        a = np.asarray(a, np.int64)
        if a.min() < 0 or a.max() >= len(env._action_set):
            raise AssertionError("action index out of range")
        return env._lut[a] if a.ndim else int(env._lut[a])
    if all_actions:
        return env.engine.lookahead_all(frames, hold=hold, rest=ale(rest), seed=seed, t=t)
    return env.engine.lookahead(frames, hold=hold, first=ale(first), rest=ale(rest), seed=seed, t=t)


def _ale(env, a):
    if a is None:
        return None
    a = np.asarray(a, np.int64)
    if a.size and (a.min() < 0 or a.max() >= len(env._action_set)):
        raise AssertionError("action index out of range")
    return env._lut[a] if a.ndim else int(env._lut[a])


def _lookahead_plan(env, frames, hold, plan, rest, seed, t):
    """Engine.lookahead_plan for an adapter: plan [depth] or [num_envs, depth] action indices -> ALE ids"""
    return env.engine.lookahead_plan(frames, _ale(env, np.asarray(plan, np.int64)), hold=hold, rest=_ale(env, rest), seed=seed, t=t)


def _search(env, frames, hold, depth, objective, rest, seed, t):
    """Engine.lookahead_search for an adapter: `plan` comes back as action indices (the digits of the code: the action set is the
    engine's legal set in its order), and the winner among an env's rows under the same objective -- ties to the smaller code --
    is added as best_action [num_envs] and best_plan [num_envs, depth]"""
    out = env.engine.lookahead_search(frames, int(depth), hold=hold, objective=objective, rest=_ale(env, rest), seed=seed, t=t)
    return _with_best(env, out, depth, objective)


def _beam(env, frames, hold, depth, width, objective, rest, seed, t):
    """Engine.lookahead_beam for an adapter: as _search, with the beam's width"""
    out = env.engine.lookahead_beam(frames, int(depth), int(width), hold=hold, objective=objective, rest=_ale(env, rest), seed=seed, t=t)
    return _with_best(env, out, depth, objective)


def _evolve(env, frames, hold, depth, population, generations, elite, mutation, plan_seed, init_plan, objective, rest, seed, t):
    """Engine.lookahead_evolve for an adapter: as _beam; init_plan [depth] or [num_envs, depth] action indices becomes the code"""
    init = None
    if init_plan is not None:
        p = np.asarray(init_plan, np.int64)
        if p.ndim not in (1, 2) or p.shape[-1] != int(depth) or (p.ndim == 2 and p.shape[0] != env.num_envs):
            raise ValueError("init_plan is [depth] or [num_envs, depth] action indices with depth %d, got shape %r" % (int(depth), p.shape))
        _ale(env, p)                                         # (range check; the action set is the legal set in its order: an index is a digit)
        L = np.uint64(len(env._action_set))
        code = np.zeros(p.shape[:-1], np.uint64)
        for k in range(p.shape[-1] - 1, -1, -1):
            code = code * L + p[..., k].astype(np.uint64)
        init = code.astype(np.float64) if p.ndim == 2 else int(code)
    out = env.engine.lookahead_evolve(frames, int(depth), int(population), int(generations), elite=elite, mutation=mutation, plan_seed=plan_seed, init=init,
                                      hold=hold, objective=objective, rest=_ale(env, rest), seed=seed, t=t)
    return _with_best(env, out, depth, objective)


def _with_best(env, out, depth, objective):
    """the rows of a search or a beam: plan as action indices, best_action and best_plan added (one lexsort per call)"""
    from ..engine import plan_digits
    out["plan"] = plan_digits(len(env._action_set), out["code"], int(depth))
    loss = np.where(out["life_lost_at"] < 0, 1 << 30, out["life_lost_at"])
    keys = (out["ret"], out["lives"], loss) if objective in ("return", 0) else (out["lives"], loss, out["ret"])
    # np.lexsort: the last key is the primary one; ascending, so larger-is-better keys are negated
    order = np.lexsort((out["code"].astype(np.int64),) + tuple(-np.asarray(k, np.float64) for k in reversed(keys)), axis=1)
    out["best_action"] = order[:, 0].astype(np.int64)
    out["best_plan"] = out["plan"][np.arange(out["plan"].shape[0]), out["best_action"]]
    return out


def sample_best_action(out, objective="return"):
    """The winner among an env's rows of a sampled lookahead (arrays [num_envs, n_actions]) -> int64 [num_envs].  "return": the
    largest ret_sum, then the smallest lost, then the largest safe_frames_sum, then the smallest index; "survival": the smallest
    lost, then the largest safe_frames_sum, then the largest ret_sum, then the smallest index."""
    if objective not in ("return", "survival"):
        raise ValueError("objective is 'return' or 'survival', got %r" % (objective,))
    ret, lost, safe = (np.asarray(out[k], np.int64) for k in ("ret_sum", "lost", "safe_frames_sum"))
    keys = (-ret, lost, -safe) if objective == "return" else (lost, -safe, -ret)
    index = np.broadcast_to(np.arange(ret.shape[1]), ret.shape)
    # np.lexsort: the last key is the primary one, ascending
    return np.lexsort((index,) + tuple(reversed(keys)), axis=1)[:, 0].astype(np.int64)


def _samples(env, frames, hold, samples, rest, seed, t, salt, objective):
    """Engine.lookahead_samples for an adapter: `rest` an action index going in; the rows are in action-index order (the action
    set is the engine's legal set in its order); the means and the winner (sample_best_action) are added"""
    if objective not in ("return", "survival"):
        raise ValueError("objective is 'return' or 'survival', got %r" % (objective,))
    out = env.engine.lookahead_samples(frames, int(samples), hold=hold, salt=salt, rest=_ale(env, rest), seed=seed, t=t)
    played = np.maximum(out["samples"], 1).astype(np.float64)
    out["ret_mean"] = out["ret_sum"] / played
    out["lost_frac"] = out["lost"] / played
    out["ended_frac"] = out["ended"] / played
    out["best_action"] = sample_best_action(out, objective)
    return out


def _search_samples(env, frames, hold, depth, samples, objective, rest, seed, t, salt):
    """Engine.lookahead_search_samples for an adapter: `rest` an action index going in, `plan` action indices coming out (the
    digits of the code); the means are added as _samples adds them, best_action is sample_best_action over the rows and best_plan
    that row's plan"""
    if objective not in ("return", "survival"):
        raise ValueError("objective is 'return' or 'survival', got %r" % (objective,))
    out = env.engine.lookahead_search_samples(frames, int(depth), int(samples), hold=hold, objective=objective, salt=salt, rest=_ale(env, rest), seed=seed, t=t)
    return _with_sample_best(env, out, depth, objective)


def _with_sample_best(env, out, depth, objective):
    """the rows of a search or a beam over samples: plan as action indices; the means, best_action and best_plan added"""
    from ..engine import plan_digits
    out["plan"] = plan_digits(len(env._action_set), out["code"], int(depth))
    played = np.maximum(out["samples"], 1).astype(np.float64)
    out["ret_mean"] = out["ret_sum"] / played
    out["lost_frac"] = out["lost"] / played
    out["ended_frac"] = out["ended"] / played
    out["best_action"] = sample_best_action(out, objective)
    out["best_plan"] = out["plan"][np.arange(out["plan"].shape[0]), out["best_action"]]
    return out


def _beam_samples(env, frames, hold, depth, width, samples, objective, rest, seed, t, salt):
    """Engine.lookahead_beam_samples for an adapter: as _search_samples, with the beam's width"""
    if objective not in ("return", "survival"):
        raise ValueError("objective is 'return' or 'survival', got %r" % (objective,))
    out = env.engine.lookahead_beam_samples(frames, int(depth), int(width), int(samples), hold=hold, objective=objective, salt=salt, rest=_ale(env, rest), seed=seed, t=t)
    return _with_sample_best(env, out, depth, objective)


def _tree(env, frames, hold, depth, simulations, explore, objective, rest, seed, t, salt):
    """Engine.lookahead_tree for an adapter: `rest` an action index going in; the rows are in action-index order.  best_action is
    sample_best_action over the root sums, best_plan [num_envs, depth] the digits of that row's principal variation, -1 beyond
    its pv_depth"""
    from ..engine import plan_digits
    if objective not in ("return", "survival"):
        raise ValueError("objective is 'return' or 'survival', got %r" % (objective,))
    out = env.engine.lookahead_tree(frames, int(depth), int(simulations), explore=explore, salt=salt, hold=hold, objective=objective, rest=_ale(env, rest), seed=seed, t=t)
    out["best_action"] = sample_best_action(out, objective)
    rows = np.arange(out["code"].shape[0])
    plan = plan_digits(len(env._action_set), out["code"][rows, out["best_action"]], int(depth))
    plan[np.arange(int(depth))[None, :] >= out["pv_depth"][rows, out["best_action"]][:, None]] = -1
    out["best_plan"] = plan
    return out


class _PlanLoop:
    """What plan_step / plan_rollout of an adapter keep on the device: a stream of their own, the rows of the last rollout's
    TBX_QUERY_LOOKAHEAD_ACT calls [k][N][11] (planner "tree": TBX_QUERY_LOOKAHEAD_TREE_ACT, [k][N][14]) and its per-step rewards and
    dones, copied device-to-device behind every step"""

    def __init__(self, env):
        from .. import hip
        self.hip, self.env = hip, env
        self.stream = hip.Stream()
        self.bufs = {}                 # name -> (device address, bytes)
        self.rows = None               # (k, planner id) of the last rollout
        self.planned = False

    def buf(self, name, nbytes):
        p, b = self.bufs.get(name, (0, 0))
        if b < nbytes:
            self.stream.synchronize()
            self.hip.free(p)
            p, b = self.hip.malloc(nbytes), nbytes
            self.bufs[name] = (p, b)
        return p

    def host(self, name, shape, dtype):
        out = np.empty(shape, dtype)
        self.hip.memcpy_dtoh(out, self.bufs[name][0], out.nbytes)
        return out

    def args(self, planner, frames, hold, depth, objective, rest, seed, t, kw):
        """the argument row of one period: the adapter's defaults for the evolution filled in, init 'carry' once a plan is there"""
        from ..engine import act_args, act_planner
        pid, kw = act_planner(planner), dict(kw)
        if pid == _abi.QUERY_LOOKAHEAD_EVOLVE:
            kw.setdefault("population", 16)
            kw.setdefault("generations", 2)
            if kw.get("elite") is None:
                kw["elite"] = max(1, int(kw["population"]) // 4)
            if kw.get("mutation") is None:
                kw["mutation"] = max(1, round(256 / max(int(depth) - 1, 1)))
            if kw.get("init") is None:
                kw["init"] = "carry" if self.planned else -1
        return pid, act_args(self.env.game, pid, frames=frames, hold=hold, depth=int(depth), objective=objective, rest=_ale(self.env, rest), seed=seed, t=t, **kw)

    def tree_args(self, frames, hold, depth, objective, rest, seed, t, kw):
        """planner "tree": the row of TBX_QUERY_LOOKAHEAD_TREE_ACT; keywords simulations (default 16), explore, salt, reuse (default True)"""
        from ..engine import tree_act_args
        kw = dict(kw)
        row = tree_act_args(self.env.game, frames, int(depth), kw.pop("simulations", 16), kw.pop("explore", 0), kw.pop("salt", 0), kw.pop("reuse", True), hold=hold,
                            objective=objective, rest=_ale(self.env, rest), seed=seed, t=t)
        if kw:
            raise TypeError("planner 'tree' takes simulations, explore, salt and reuse, got %r" % (sorted(kw),))
        return row

    def run(self, k, planner, frames, hold, depth, objective, rest, seed, t, kw, step, reward_id, reward_bytes, done_id, sub, drop_id=None):
        """k periods queued back to back on the stream: the query, then step(action pointer, stream) `sub` times, the reward and
        done buffers copied behind each; ONE synchronisation at the end.  -> (reward [k, sub, N], done [k, sub, N]).  Planner
        "tree" with reuse: TBX_EDIT_TREE_DROP is queued behind every step with the buffer drop_id as its mask -- the carried trees
        of a game that ended do not steer the new one."""
        env, eng, hip, n = self.env, self.env.engine, self.hip, self.env.num_envs
        tree = planner == "tree" or planner == _abi.QUERY_LOOKAHEAD_TREE_ACT
        width = 14 if tree else 11
        rows = self.buf("rows", 8 * width * n * k)
        rew, don = self.buf("reward", reward_bytes * n * k * sub), self.buf("done", n * k * sub)
        for i in range(k):
            if tree:
                pid, args = _abi.QUERY_LOOKAHEAD_TREE_ACT, self.tree_args(frames, hold, depth, objective, rest, seed, int(t) + i, kw)
                eng.reduce_device(pid, rows + 8 * width * n * i, args, stream=self.stream.ptr)
            else:
                pid, args = self.args(planner, frames, hold, depth, objective, rest, seed, int(t) + i, kw)
                eng.reduce_device(_abi.QUERY_LOOKAHEAD_ACT, rows + 8 * 11 * n * i, args, stream=self.stream.ptr)
                self.planned = True
            action = eng.plan_action_ptr                 # (made by the engine's first such query; its address stays)
            for j in range(sub):
                step(action, self.stream.ptr)
                at = i * sub + j
                hip.memcpy_dtod_async(rew + reward_bytes * n * at, eng.device_buffer(reward_id)[0], reward_bytes * n, self.stream)
                hip.memcpy_dtod_async(don + n * at, eng.device_buffer(done_id)[0], n, self.stream)
                if tree and args[12]:
                    eng.edit_device(_abi.EDIT_TREE_DROP, (), mask_ptr=eng.device_buffer(drop_id)[0], stream=self.stream.ptr)
        self.stream.synchronize()
        self.rows = (k, pid, width)
        return self.host("reward", (k, sub, n), np.float32 if reward_id == _abi.BUF_AGENT_REWARD else np.int32), self.host("done", (k, sub, n), np.uint8)

    def actions(self):
        if self.rows is None:
            raise RuntimeError("plan_actions before the first plan_step / plan_rollout")
        k, _, width = self.rows
        return self.host("rows", (k, self.env.num_envs, width), np.float64)[..., 1].astype(np.int64)

    def close(self):
        self.stream.synchronize()
        for p, _ in self.bufs.values():
            self.hip.free(p)
        self.bufs = {}
        self.stream.close()


def _fork_map(n, src, envs):
    """(src int[N], selected bool[N]) of a fork: src an int (one source fanned out) or one index per env; envs None (every
    env), a boolean mask or indices.  Unselected envs name themselves."""
    sel = np.zeros(n, bool)
    if envs is None:
        sel[:] = True
    else:
        sel[envs] = True
    s = np.arange(n, dtype=np.int64)
    full = np.broadcast_to(np.asarray(src, np.int64), (n,)) if np.ndim(src) <= 1 else None
    if full is None:
        raise ValueError("src must be an int or one index per env")
    s[sel] = full[sel]
    if s.min() < 0 or s.max() >= n:
        raise ValueError("fork: a source outside 0 .. %d" % (n - 1))
    return s, sel


class ToyboxVecEnv:
    CACHE_TERMINAL_STATE_UP_TO = 64      # cache_terminal_state=None: on up to this many envs

    def __init__(self, game, num_envs, grayscale=True, alpha=False, seed=None, cache_terminal_state=None, engine=None,
                 obs_pool=2, reuse_obs_buffer=None):
        """cache_terminal_state: ToyboxBaseEnv.step always attaches info["cached_state"] = the state JSON on the step that ends
        a game (envs/atari/base.py:128-130).  Here that needs the finished envs' state records on the host BEFORE they are reset,
        which takes the step out of the asynchronous path (step, read-back, new_game, render as four synchronous calls).  None
        (default): on for batches of up to CACHE_TERMINAL_STATE_UP_TO envs -- the sizes the reference's own vector envs run
        (run.py: nenv = the CPU count) -- and off above, where the batch step with in-kernel auto-reset is the point; True /
        False force it.  INTEGRATION.md section 3, row V.
        obs_pool: the observations that reset() / step() return are page-locked host arrays handed out in rotation, so an
        observation stays valid until obs_pool - 1 further steps have been taken (default 2: the reference's learners copy on
        receipt -- `self.obs[:] = self.env.step(...)`, baselines/ppo2/ppo2.py:110 -- and the copy from the device runs at the PCIe
        link's rate, asynchronously between step_async and step_wait).  obs_pool = 0 is the contract as the reference's VecEnvs
        spell it, a fresh pageable array per call: a staged copy plus page faults, several times slower
        (bench.py --protocol host times both).  reuse_obs_buffer=True/False is the older spelling of obs_pool = 1 / 0."""
        self.game = {"spaceinvaders": "space_invaders"}.get(game, game)
        self.num_envs = int(num_envs)
        self.engine = engine if engine is not None else _make_engine(self.game, self.num_envs)
        self._channels = 1 if grayscale else 4 if alpha else 3
        shape = (self.num_envs, self.engine.height, self.engine.width, self._channels)
        self._obs_shape = shape
        self._pool = [self.engine.host_array(shape) for _ in range(_pool_size(obs_pool, reuse_obs_buffer))]
        self._turn = 0
        # step outputs staged in page-locked memory; what step_wait returns are fresh copies (rollout buffers keep references:
        # `mb_rewards.append(rewards)`, ppo2.py:113)
        n = self.num_envs
        self._st = {"reward": self.engine.host_array((n,), np.int32), "done": self.engine.host_array((n,), np.uint8),
                    "lives": self.engine.host_array((n,), np.int32), "score": self.engine.host_array((n,), np.int32)}
        self._action_set = sorted(self.engine.legal_actions)
        self._lut = np.asarray(self._action_set, dtype=np.int32)
        self.action_space = Discrete(len(self._action_set))
        self.observation_space = Box(0, 255, (self.engine.height, self.engine.width, self._channels), "uint8")
        self.cache_terminal_state = self.num_envs <= self.CACHE_TERMINAL_STATE_UP_TO if cache_terminal_state is None else bool(cache_terminal_state)
        self._codec = codec(self.game)
        self._pending = None
        self._in_flight = None
        self._plan = None                   # plan_step / plan_rollout: made by the first call
        self.closed = False
        if seed is not None:
            self.seed(seed)

    # ------------------------------------------------------------------ seeding
    def seed(self, seed):
        """env i gets the reference's per-env derivation (cmd_util.py:31: seed + rank), each pushed through
        ToyboxBaseEnv.seed's hash (envs/atari/base.py:84-98); returns [[seed1, seed2], ...]."""
        out = [[int(seed) + i, hash_seed(int(seed) + i + 1) % 2 ** 31] for i in range(self.num_envs)]
        self.engine.seed_array([s2 for _, s2 in out])      # one upload + one launch, not N
        self.engine.new_game()
        return out

    # ------------------------------------------------------------------ VecEnv
    def _next_obs_array(self):
        if not self._pool:
            return np.empty(self._obs_shape, np.uint8)
        a = self._pool[self._turn % len(self._pool)]
        self._turn += 1
        return a

    def _frames(self):
        return self.engine.render(self._channels, out=self._next_obs_array())

    def reset(self):
        if self._in_flight is not None:          # a step between step_async and step_wait: it ends first (its results are dropped)
            self.step_wait()
        self._pending = None
        self.engine.new_game()
        return self._frames()

    def step_async(self, actions):
        """Queues the whole step -- actions to the device, the batch step with auto-reset, the rasteriser, the copy of every
        frame and of the step outputs to host memory -- and returns; step_wait() collects
        (vec_env/__init__.py:67-87, subproc_vec_env.py:63-74)."""
        a = np.asarray(actions)
        if a.shape != (self.num_envs,):
            raise ValueError("actions must have shape (%d,)" % self.num_envs)
        if a.min() < 0 or a.max() >= len(self._action_set):
            raise AssertionError("action index out of range")   # assert action_index < len(action_set) (base.py:123)
        ale = self._lut[a.astype(np.int64)]
        if self.cache_terminal_state:
            self._pending = ale                                  # (needs the states of finished games before they are reset)
            return
        obs = self._next_obs_array()
        st = self._st
        self.engine.step_begin(ale, auto_reset=True, reward=st["reward"], done=st["done"], lives=st["lives"], score=st["score"],
                               frame=obs, channels=self._channels)
        self._in_flight = obs

    def step_wait(self):
        if self._in_flight is not None:
            obs, self._in_flight = self._in_flight, None
            self.engine.step_end()
            st = self._st
            reward, lives, score = st["reward"].copy(), st["lives"].copy(), st["score"].copy()
            done = st["done"].astype(bool)
            infos = LazyInfos(self.num_envs, {"lives": lives, "score": np.where(done, 0, score)}, {})
            return obs, reward.astype(np.float32), done, infos
        assert self._pending is not None, "step_wait without step_async"
        actions, self._pending = self._pending, None
        extras = {}
        reward, done, lives, score = self.engine.step(actions, auto_reset=False)
        idx = np.nonzero(done)[0]
        for i in idx:
            extras[int(i)] = {"cached_state": self._codec.state_to_json(self.engine.get_state(int(i)))}
        if len(idx):
            self.engine.new_game(done.astype(np.uint8))
        obs = self._frames()
        infos = LazyInfos(self.num_envs, {"lives": lives, "score": np.where(done, 0, score)}, extras)
        return obs, reward.astype(np.float32), done, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def fork(self, src, envs=None, salt=None):
        """Branch on the device (Engine.fork): the envs `envs` (None: all; a boolean mask or indices) become copies of env src
        (an int, or one index per env) as they were before the call; salt: None, an int or one per env (fresh randomness from the
        same fork point).  Returns the observation batch the policy should see next -- what the last step_wait() would have
        returned had env i been env src[i].  Between step_async and step_wait the step ends first (its results are dropped)."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        s, sel = _fork_map(self.num_envs, src, envs)
        self.engine.fork(s, mask=sel, salt=salt)
        return self._frames()

    def checkpoint_slots(self, slots):
        """A fresh, empty checkpoint store of `slots` planes of num_envs cells on the device (Engine.checkpoint_slots); 0 releases it"""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        self.engine.checkpoint_slots(slots)

    def save_checkpoint(self, slot, envs=None):
        """The envs `envs` (None: all; a boolean mask or indices) are set aside in cell (slot, their own row) of the store.  Between
        step_async and step_wait the step ends first (its results are dropped)."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        self.engine.checkpoint_save(slot, mask=_fork_map(self.num_envs, 0, envs)[1])

    def restore_checkpoint(self, slot, rows=None, envs=None, salt=None):
        """The envs `envs` become the envs saved in cell (slot, rows[i]) (rows None: their own row); salt as in fork().  Returns the
        observation batch the policy should see next, as fork() does.  Between step_async and step_wait the step ends first."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        self.engine.checkpoint_restore(slot, rows=rows, mask=_fork_map(self.num_envs, 0, envs)[1], salt=salt)
        return self._frames()

    def lookahead(self, steps, first=None, rest=None, all_actions=False, seed=0, t=0):
        """What the next `steps` steps bring every env, without taking them (Engine.lookahead): the env plays action index `first`
        in the first step and `rest` in the others (None: drawn like Engine.step_synthetic(seed, t + step)); all_actions=True
        answers for every action index as the first one, arrays [num_envs, n_actions].  Returns a dict of ret (the reward summed),
        score, lives, frames_run and life_lost_at.  The env, its RNG and its next observation are untouched.  These are raw game
        frames from the state as it stands: an episode's end is the game's end and nothing is reset.  Between step_async and
        step_wait the step ends first (its results are dropped)."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        return _lookahead(self, int(steps), 1, first, rest, all_actions, seed, t)

    def lookahead_plan(self, steps, plan, rest=None, seed=0, t=0):
        """lookahead() under an action sequence (Engine.lookahead_plan): plan [depth] or [num_envs, depth] action indices, action p
        in step p, `rest` in the steps after the last.  The same dict of five."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        return _lookahead_plan(self, int(steps), 1, plan, rest, seed, t)

    def search(self, steps, depth, objective="return", rest=None, seed=0, t=0):
        """Every action sequence of `depth` steps, followed by `rest`, played `steps` steps ahead on the device without taking
        them (Engine.lookahead_search): for each first action index the best plan under objective "return" or "survival" -- ret,
        score, lives, frames_run, life_lost_at, code [num_envs, n_actions], plan [num_envs, n_actions, depth] (action indices) --
        and the winner among them, best_action [num_envs] and best_plan [num_envs, depth].  Nothing is touched; a pending
        step_async ends first, as in lookahead()."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        return _search(self, int(steps), 1, depth, objective, rest, seed, t)

    def beam_search(self, steps, depth, width, objective="return", rest=None, seed=0, t=0):
        """search() for plans deeper than it can enumerate (Engine.lookahead_beam): per first action index and level the `width`
        best action sequences are kept and extended by every action.  The dict of search(); with width 1 it is greedy search,
        with width >= n_actions ** (depth - 2) it is search()."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        return _beam(self, int(steps), 1, depth, width, objective, rest, seed, t)

    def evolve_search(self, steps, depth, population, generations, elite=None, mutation=None, plan_seed=0, init_plan=None, objective="return", rest=None,
                      seed=0, t=0):
        """Evolutionary search over whole plans of `depth` steps with a budget the caller chooses (Engine.lookahead_evolve): per
        first action index a population of `population` action sequences is played, ranked and bred `generations` times from its
        `elite` best by mutation.  init_plan ([depth] or [num_envs, depth] action indices; its first action is replaced by every
        first action in turn) seeds the population -- a rolling-horizon controller hands in the last best_plan shifted by one
        step.  The dict of search(); more generations are never worse.  Nothing is touched; a pending step_async ends first."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        return _evolve(self, int(steps), 1, depth, population, generations, elite, mutation, plan_seed, init_plan, objective, rest, seed, t)

    def tree_search(self, steps, depth, simulations, explore=0, objective="return", rest=None, seed=0, t=0, salt=0):
        """Monte-Carlo tree search over action prefixes up to `depth` steps deep (Engine.lookahead_tree): per first action index
        `simulations` futures of `steps` steps are spent adaptively -- each walks down the tree by mean value plus `explore` x
        the visit bonus, adds at most one node and plays its prefix, `rest` behind it.  The eight sums of sample_lookahead() over
        the root's futures, then the most visited path: code, pv_depth, pv_visits, pv_value [num_envs, n_actions]; best_action
        [num_envs] by sample_best_action and best_plan [num_envs, depth] (action indices, -1 beyond the path's depth).  Nothing
        is touched; a pending step_async ends first."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        return _tree(self, int(steps), 1, depth, simulations, explore, objective, rest, seed, t, salt)

    def plan_rollout(self, k, planner="evolve", steps=16, depth=4, hold=1, objective="return", rest=None, seed=0, t=0, **planner_keywords):
        """k closed-loop steps queued back to back on a stream of the env's own, no host synchronisation in between
        (Engine.lookahead_act_device): per step the planner ("search", "search_samples", "beam", "beam_samples" or "evolve";
        planner_keywords: width, samples, salt, population, generations, elite, mutation, plan_seed, init; or "tree", the tree
        search through Engine.lookahead_tree_act_device with simulations, explore, salt and reuse=True: the subtree under the
        played action starts the next step's trees, and the trees of envs whose game ended are dropped on the device) looks `steps` steps of
        `hold` frames each ahead with plans of `depth` steps, every env's winner is picked on the device, and its first action is
        played for `hold` frames with auto-reset, read by the step from the device buffer the pick wrote.  Step i plans with
        counter t + i, so drawn `rest` actions line up across calls.  The evolution (default population 16, generations 2) is
        seeded from the second planned step of this env on with the last winner's plan shifted by one step (init="carry");
        init=-1 switches that off.  Returns what step() returns with a leading axis k on rewards (summed over the held frames)
        and dones (any of them): (obs after the last step, float32 [k, num_envs], bool [k, num_envs], infos of the last frame,
        without cached_state).  plan_actions() reads the chosen action indices back."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        if int(k) < 1 or int(hold) < 1:
            raise ValueError("plan_rollout takes k >= 1 steps of hold >= 1 frames")
        if self._plan is None:
            self._plan = _PlanLoop(self)
        eng = self.engine
        reward, done = self._plan.run(int(k), planner, int(steps) * int(hold), int(hold), depth, objective, rest, seed, t, planner_keywords,
                                      lambda action, stream: eng.step_device(action, auto_reset=True, stream=stream), _abi.BUF_REWARD, 4, _abi.BUF_DONE, int(hold), _abi.BUF_DONE)
        lives, score = np.empty(self.num_envs, np.int32), np.empty(self.num_envs, np.int32)
        self._plan.hip.memcpy_dtoh(lives, eng.device_buffer(_abi.BUF_LIVES)[0], lives.nbytes)
        self._plan.hip.memcpy_dtoh(score, eng.device_buffer(_abi.BUF_SCORE)[0], score.nbytes)
        last = done[-1, -1].astype(bool)
        infos = LazyInfos(self.num_envs, {"lives": lives, "score": np.where(last, 0, score)}, {})
        return self._frames(), reward.sum(axis=1).astype(np.float32), done.any(axis=1), infos

    def plan_step(self, planner="evolve", steps=16, depth=4, hold=1, objective="return", rest=None, seed=0, t=0, **planner_keywords):
        """One closed-loop step, plan_rollout(1, ...): plan on the device, pick every env's winner there and play its first action
        for `hold` frames.  Returns what step() returns."""
        obs, reward, done, infos = self.plan_rollout(1, planner, steps, depth, hold, objective, rest, seed, t, **planner_keywords)
        return obs, reward[0], done[0], infos

    def plan_actions(self):
        """The action indices the last plan_step / plan_rollout chose, int64 [k, num_envs], read back from the device on demand"""
        if self._plan is None:
            raise RuntimeError("plan_actions before the first plan_step / plan_rollout")
        return self._plan.actions()

    def lookahead_samples(self, steps, samples, rest=None, seed=0, t=0, salt=0, objective="return"):
        """`samples` random futures of `steps` steps per env and first action index, summed on the device without taking them
        (Engine.lookahead_samples): future s draws its actions (rest None) under its own seed and, with a salt that is not 0,
        plays with the game's randomness salted by salt + s.  Returns samples, ret_sum, ret_min, ret_max, lives_sum, lost, ended,
        safe_frames_sum [num_envs, n_actions], the means ret_mean, lost_frac, ended_frac, and best_action [num_envs] under
        objective "return" (ret_sum, then fewer lost, then more safe frames) or "survival" (fewer lost, then more safe frames,
        then ret_sum); ties to the smaller index.  Nothing is touched; a pending step_async ends first, as in lookahead()."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        return _samples(self, int(steps), 1, samples, rest, seed, t, salt, objective)

    def beam_search_samples(self, steps, depth, width, samples, objective="return", rest=None, seed=0, t=0, salt=0):
        """beam_search() over sampled futures (Engine.lookahead_beam_samples): search_samples() for plans deeper than it can
        enumerate.  Per first action index and level the `width` best action sequences by the summed outcome of the same
        `samples` futures are kept and extended by every action.  The dict of search_samples(): the eight sums, code, plan
        (action indices), the means, best_action and best_plan.  Nothing is touched; a pending step_async ends first."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        return _beam_samples(self, int(steps), 1, depth, width, samples, objective, rest, seed, t, salt)

    def search_samples(self, steps, depth, samples, objective="return", rest=None, seed=0, t=0, salt=0):
        """search() over sampled futures (Engine.lookahead_search_samples): every action sequence of `depth` steps is played on
        the same `samples` futures -- future s its own drawn action stream after the plan (rest None) and, with a salt that is
        not 0, its own game randomness -- and for each first action index the best plan by the summed outcome comes back: the
        eight sums of lookahead_samples() and code [num_envs, n_actions], plan [num_envs, n_actions, depth] (action indices),
        the means ret_mean, lost_frac, ended_frac, and the winner among the rows (the order of lookahead_samples()),
        best_action [num_envs] and best_plan [num_envs, depth].  Nothing is touched; a pending step_async ends first."""
        if self._in_flight is not None or self._pending is not None:
            self.step_wait()
        return _search_samples(self, int(steps), 1, depth, samples, objective, rest, seed, t, salt)

    def get_images(self):
        return self.engine.render(3)

    def render(self, mode="rgb_array"):
        imgs = self.get_images()
        if mode == "rgb_array":
            return imgs
        raise NotImplementedError("only rgb_array rendering is provided")

    def close(self):
        if not self.closed:
            if self._in_flight is not None:
                self.step_wait()
            if self._plan is not None:
                self._plan.close()
                self._plan = None
            self.engine.close()                 # (the page-locked arrays live on while a caller holds an observation)
            self.closed = True

    @property
    def unwrapped(self):
        return self

    def get_action_meanings(self):
        from .constants import ACTION_MEANING
        return list(ACTION_MEANING.values())


class PlaneStack:
    """The stacked observation of every env as its `stack` planes, oldest first, each uint8[N, h, w] in page-locked host memory
    -- the batched counterpart of the reference's LazyFrames (atari_wrappers.py:288-317: "common frames between the observations
    are only stored once ... should only be converted to numpy array before being passed to the model").  np.asarray(obs) is
    the uint8[N, h, w, stack] array VecFrameStack / FrameStack would have returned; obs[i] one env's (h, w, stack); obs.planes
    the planes themselves (no copy).  Valid until the env's next step: the planes are shared with the following observations
    and VecFrameStack's zeroing of a finished env's older frames (vec_frame_stack.py:21-23) happens in place."""

    def __init__(self, planes):
        self.planes = tuple(planes)
        n, h, w = self.planes[0].shape
        self.shape = (n, h, w, len(self.planes))
        self.dtype = np.dtype(np.uint8)
        self.ndim = 4

    def __array__(self, dtype=None, copy=None):
        out = np.stack(self.planes, axis=-1)
        return out if dtype is None else out.astype(dtype)

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, i):
        if isinstance(i, (int, np.integer)):
            return np.stack([p[i] for p in self.planes], axis=-1)
        return np.asarray(self)[i]

    def astype(self, dtype):
        return np.asarray(self).astype(dtype)


class ToyboxPreprocVecEnv:
    """The DeepMind-style pipeline of the reference's baselines fork -- MaxAndSkipEnv(skip) -> WarpFrame(84x84 gray) ->
    ClipRewardEnv -> VecFrameStack(stack) (atari_wrappers.py:193-244,324-360; vec_frame_stack.py:17-30) -- as ONE device
    pass per agent step (tbx_agent_step): the learner only ever sees uint8[N, size, size, stack].

    episode_life / fire_reset / noop_max switch on the reset-time wrappers of wrap_deepmind / make_atari
    (EpisodicLifeEnv :58-96, FireResetEnv :38-56, NoopResetEnv :12-36), run inside the reset kernel; the Monitor
    record of a finished game arrives as info["episode"] = {"r", "l", "t"} like bench/monitor.py:64-76 (t = seconds since this
    adapter was constructed, where Monitor / VecMonitor count from their own construction; 6 decimals).  env_offset is the
    global index of env 0 (multi-GPU sharding) so no-op counts do not depend on the shard layout.

    frame_stack="vec" (default) stacks like VecFrameStack over the vector env: a reset leaves zeros in the older slots.
    frame_stack="env" stacks like wrap_deepmind(frame_stack=True), a FrameStack(k) inside every env
    (atari_wrappers.py:246-275): a reset fills the whole stack with its observation.  scale=True is ScaledFloatFrame
    (atari_wrappers.py:277-286): observations come back as float32 in [0, 1] (uint8 / 255, converted on the host; the device
    buffer TBX_BUF_AGENT_OBS stays uint8).

    How the observation reaches the host (obs_layout; results are the same array values in every case):
      "device_stack" (default)  the stacks are rolled on the device and the whole uint8[N, size, size, stack] crosses PCIe into a
                                rotating pool of obs_pool page-locked arrays (see ToyboxVecEnv);
      "planes"                  the reference's data flow: ONE new size x size plane per env and step crosses PCIe
                                (subproc_vec_env.py:63-74 sends one frame per env; VecFrameStack stacks on the receiving side,
                                vec_frame_stack.py:17-30) into a ring of page-locked planes, and the observation is a
                                PlaneStack over the newest `stack` of them -- a quarter of the bytes, no roll at all (nor on
                                the device: tbx_agent_config_t::new_plane = 2, the observation kernels write the plane alone); a
                                finished env's older planes are zeroed (frame_stack="env": overwritten with the reset
                                observation) in place, exactly the values VecFrameStack / FrameStack produce;
      "host_stack"              the same one-plane transfer, then VecFrameStack's roll on the host into a real
                                uint8[N, size, size, stack] array of the rotating pool (tbx_host_stack_push: np.roll's data
                                movement as threaded host code; 9 bytes of host memory traffic per pixel, so at 10^4 envs it is
                                the host's memory system that sets the rate, not the link).
    step_async() queues the device work and the copies; step_wait() waits for them (vec_env/__init__.py:67-87).

    size: the side of the square observation, from the smallest size with at most 8 source pixels per output pixel on each axis
    (frame / size, rounded up, plus one <= 8) to 84 (size x size <= 7056): Breakout 35..84, SpaceInvaders 46..84, Amidar
    36..84, GridWorld 23..84.  Engine.agent_init takes non-square out_h x out_w within the limits of include/toybox_amd.h
    (tbx_agent_config_t); anything outside them raises ToyboxAmdError."""

    def __init__(self, game, num_envs, skip=4, size=84, stack=4, clip_rewards=True, seed=None, engine=None,
                 episode_life=False, fire_reset=False, noop_max=0, noop_seed=0, env_offset=0, frame_stack="vec", scale=False,
                 obs_pool=2, obs_layout="device_stack", reuse_obs_buffer=None):
        self.game = {"spaceinvaders": "space_invaders"}.get(game, game)
        self.num_envs = int(num_envs)
        self.engine = engine if engine is not None else _make_engine(self.game, self.num_envs)
        self._action_set = sorted(self.engine.legal_actions)
        self._lut = np.asarray(self._action_set, dtype=np.int32)
        self.action_space = Discrete(len(self._action_set))
        if frame_stack not in ("vec", "env"):
            raise ValueError("frame_stack must be 'vec' (VecFrameStack) or 'env' (FrameStack inside every env)")
        if obs_layout not in ("device_stack", "planes", "host_stack"):
            raise ValueError("obs_layout must be 'device_stack', 'planes' or 'host_stack'")
        self.obs_layout = obs_layout
        self._fill_repeat = frame_stack == "env"
        self.scale = bool(scale)
        self.stack, self.size = int(stack), int(size)
        self._skip = int(skip)
        self.observation_space = Box(0, 1.0, (size, size, stack), "float32") if self.scale else Box(0, 255, (size, size, stack), "uint8")
        if seed is not None:
            self.engine.seed_array([hash_seed(int(seed) + i + 1) % 2 ** 31 for i in range(self.num_envs)])
        self.engine.agent_init(skip=skip, out_h=size, out_w=size, stack=stack, clip_reward=clip_rewards,
                               episodic_life=episode_life, fire_reset=fire_reset, noop_max=noop_max, noop_seed=noop_seed,
                               env_offset=env_offset, stack_fill=1 if frame_stack == "env" else 0,
                               new_plane=0 if obs_layout == "device_stack" else 2)     # host layouts: no stack on the device at all
        self._pending = None
        self._in_flight = None
        self._plan = None                   # plan_step / plan_rollout: made by the first call
        self.closed = False
        self.tstart = time.time()                # Monitor.tstart (bench/monitor.py:19), VecMonitor.tstart (vec_monitor.py:12)
        n = self.num_envs
        pool = _pool_size(obs_pool, reuse_obs_buffer)
        self._pool, self._turn = [], 0
        if obs_layout != "planes":
            self._pool = [self.engine.host_array((n, size, size, stack)) for _ in range(pool)]
        if obs_layout != "device_stack":
            # the plane ring: the `stack` planes of the current observation + one per further observation that has to stay intact
            self._ring = [self.engine.host_array((n, size, size)) for _ in range(stack + max(1, pool) - (1 if obs_layout == "planes" else 0))]
            for r in self._ring:
                r[...] = 0
            self._head = 0                       # ring slot of the newest plane
            if obs_layout == "host_stack":
                self._ring = self._ring[:1]      # one landing plane is enough: the stack itself lives in the pool arrays
                self._stacked = None             # the array the last observation went out in (the roll's source)
        self._st = {"reward": self.engine.host_array((n,), np.float32), "done": self.engine.host_array((n,), np.uint8),
                    "ep_done": self.engine.host_array((n,), np.uint8), "ep_return": self.engine.host_array((n,), np.float32),
                    "ep_length": self.engine.host_array((n,), np.int32)}

    # ------------------------------------------------------------------ observation plumbing
    def _next_obs_array(self):
        if not self._pool:
            return np.empty((self.num_envs, self.size, self.size, self.stack), np.uint8)
        a = self._pool[self._turn % len(self._pool)]
        self._turn += 1
        return a

    def _landing(self):
        """(where the device's output of this step goes, keyword of the descriptor)"""
        if self.obs_layout == "device_stack":
            return self._next_obs_array(), "obs"
        if self.obs_layout == "host_stack":
            return self._ring[0], "plane"
        self._head = (self._head + 1) % len(self._ring)
        return self._ring[self._head], "plane"

    def _stacked_obs(self, landed, done, reset):
        """What VecFrameStack.step_wait / .reset (vec_frame_stack.py:17-33) -- or FrameStack inside the envs
        (atari_wrappers.py:261-275) -- hand out once the new plane has landed."""
        if self.obs_layout == "device_stack":
            return landed
        k = self.stack
        if self.obs_layout == "planes":
            R = len(self._ring)
            older = [self._ring[(self._head - j) % R] for j in range(1, k)]
            idx = slice(None) if reset else np.flatnonzero(done)
            if reset or len(idx):
                for p in older:                  # stackedobs[i] = 0  (FrameStack.reset: the observation k times)
                    p[idx] = landed[idx] if self._fill_repeat else 0
            return PlaneStack(older[::-1] + [landed])
        out = self._next_obs_array()                 # (one pool array: rolled in place)
        src = self._stacked if self._stacked is not None else out
        self.engine.host_stack_push(out, src, landed, done=None if reset else done, reset=reset, fill_repeat=self._fill_repeat)
        self._stacked = out
        return out

    def _obs(self, obs):
        # ScaledFloatFrame.observation: np.array(observation).astype(np.float32) / 255.0
        return np.asarray(obs).astype(np.float32) / 255.0 if self.scale else obs

    def reset(self):
        if self._in_flight is not None:
            self.step_wait()
        landed, key = self._landing()
        self.engine.agent_reset()
        self.engine.agent_fetch(**{key: landed})
        return self._obs(self._stacked_obs(landed, None, True))

    def step_async(self, actions):
        a = np.asarray(actions)
        if a.shape != (self.num_envs,):
            raise ValueError("actions must have shape (%d,)" % self.num_envs)
        if a.min() < 0 or a.max() >= len(self._action_set):
            raise AssertionError("action index out of range")
        landed, key = self._landing()
        st = self._st
        self.engine.agent_step_begin(self._lut[a.astype(np.int64)], reward=st["reward"], done=st["done"], ep_done=st["ep_done"],
                                     ep_return=st["ep_return"], ep_length=st["ep_length"], **{key: landed})
        self._in_flight = landed

    def step_wait(self):
        assert self._in_flight is not None, "step_wait without step_async"
        landed, self._in_flight = self._in_flight, None
        self.engine.agent_step_end()
        st = self._st
        reward, done = st["reward"].copy(), st["done"].astype(bool)
        ended = np.flatnonzero(st["ep_done"])
        ret, length = st["ep_return"], st["ep_length"]
        t = round(time.time() - self.tstart, 6) if len(ended) else 0.0
        extras = {int(i): {"episode": {"r": float(ret[i]), "l": int(length[i]), "t": t}} for i in ended}
        return self._obs(self._stacked_obs(landed, done, False)), reward, done, LazyInfos(self.num_envs, None, extras)

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def fork(self, src, envs=None, salt=None):
        """Branch on the device (Engine.fork): the envs `envs` (None: all; a boolean mask or indices) become copies of env src
        (an int, or one index per env) as they were before the call -- the game, the wrapper stack's per-env state (Monitor,
        EpisodicLifeEnv, the two frames of MaxAndSkipEnv) and the frame stack; salt: None, an int or one per env (fresh
        randomness from the same fork point).  Returns the observation batch the policy should see next: what the last
        step_wait() / reset() would have returned had env i been env src[i].  What this adapter keeps per env on the host moves
        with it: the page-locked planes of obs_layout="planes" are permuted IN PLACE (the PlaneStack handed out last shares them,
        like every observation of that layout it is valid until the next call), the rolled array of "host_stack" into the next
        array of the pool.  Between step_async and step_wait the step ends first (its results are dropped)."""
        if self._in_flight is not None:
            self.step_wait()
        s, sel = _fork_map(self.num_envs, src, envs)
        self.engine.fork(s, mask=sel, salt=salt)
        dst = np.flatnonzero(sel & (s != np.arange(self.num_envs)))
        if self.obs_layout == "device_stack":
            obs = self._next_obs_array()
            self.engine.agent_fetch(obs=obs)
            return self._obs(obs)
        if self.obs_layout == "planes":
            R, k = len(self._ring), self.stack
            planes = [self._ring[(self._head - j) % R] for j in range(k)]
            for p in planes:
                p[dst] = p[s[dst]]                   # (the right-hand side is gathered before anything is written)
            return self._obs(PlaneStack(planes[::-1]))
        if self._stacked is None:
            raise RuntimeError("fork before the first reset()")
        prev, out = self._stacked, self._next_obs_array()
        if out is not prev:
            out[...] = prev
        out[dst] = prev[s[dst]]
        self._stacked = out
        return self._obs(out)

    def checkpoint_slots(self, slots):
        """A fresh, empty checkpoint store of `slots` planes of num_envs cells on the device (Engine.checkpoint_slots); 0 releases it"""
        if self._in_flight is not None:
            self.step_wait()
        self.engine.checkpoint_slots(slots)

    def save_checkpoint(self, slot, envs=None):
        """The envs `envs` (None: all; a boolean mask or indices) are set aside in cell (slot, their own row) of the store: the game,
        the wrapper stack's per-env state and the frame stack, as the device holds them.  Between step_async and step_wait the step
        ends first (its results are dropped)."""
        if self._in_flight is not None:
            self.step_wait()
        self.engine.checkpoint_save(slot, mask=_fork_map(self.num_envs, 0, envs)[1])

    def restore_checkpoint(self, slot, rows=None, envs=None, salt=None):
        """The envs `envs` become the envs saved in cell (slot, rows[i]) (rows None: their own row); salt as in fork().  Returns the
        observation batch the policy should see next, as fork() does.  The host-side stacks of obs_layout="planes" (in place) and
        "host_stack" (into the next array of the pool) take the restored envs' planes from the device's plane ring, oldest first;
        the other envs' host data stays.  Between step_async and step_wait the step ends first (its results are dropped)."""
        if self._in_flight is not None:
            self.step_wait()
        sel = _fork_map(self.num_envs, 0, envs)[1]
        self.engine.checkpoint_restore(slot, rows=rows, mask=sel, salt=salt)
        if self.obs_layout == "device_stack":
            obs = self._next_obs_array()
            self.engine.agent_fetch(obs=obs)
            return self._obs(obs)
        from .. import hip
        k, n = self.stack, self.num_envs
        ptr, nbytes = self.engine.device_buffer(_abi.BUF_AGENT_RING)
        ring = np.empty((k, n, self.size, self.size), np.uint8)
        self.engine.sync()
        hip.memcpy_dtoh(ring, ptr, nbytes)
        head = self.engine.agent_ring_head()
        logical = [ring[(head + 1 + c) % k] for c in range(k)]           # oldest first
        idx = np.flatnonzero(sel)
        if self.obs_layout == "planes":
            R = len(self._ring)
            planes = [self._ring[(self._head - j) % R] for j in range(k)][::-1]
            for p, src in zip(planes, logical):
                p[idx] = src[idx]
            return self._obs(PlaneStack(planes))
        if self._stacked is None:
            raise RuntimeError("restore_checkpoint before the first reset()")
        prev, out = self._stacked, self._next_obs_array()
        if out is not prev:
            out[...] = prev
        for c, src in enumerate(logical):
            out[idx, :, :, c] = src[idx]
        self._stacked = out
        return self._obs(out)

    def lookahead(self, steps, first=None, rest=None, all_actions=False, seed=0, t=0):
        """What the next `steps` agent steps (steps x skip raw frames, every action held for skip frames) bring every env, without
        taking them (Engine.lookahead): action index `first` in the first step, `rest` in the others (None: drawn like
        Engine.step_synthetic(seed, t + step)); all_actions=True answers for every action index as the first one, arrays
        [num_envs, n_actions].  Returns a dict of ret, score, lives, frames_run and life_lost_at, counted in RAW frames.
        The wrappers are NOT simulated: no no-op or fire reset, no episodic life (the run ends when the GAME ends, not at a lost
        life -- life_lost_at tells where that was), no reward clipping (ret sums raw score steps), no frame maximum.  The env, its
        wrapper state and its next observation are untouched.  Between step_async and step_wait the step ends first."""
        if self._in_flight is not None:
            self.step_wait()
        return _lookahead(self, int(steps) * self._skip, self._skip, first, rest, all_actions, seed, t)

    def lookahead_plan(self, steps, plan, rest=None, seed=0, t=0):
        """lookahead() under an action sequence (Engine.lookahead_plan): plan [depth] or [num_envs, depth] action indices, action p
        held for the skip frames of agent step p, `rest` in the steps after the last.  Raw frames, no wrapper, as in lookahead()."""
        if self._in_flight is not None:
            self.step_wait()
        return _lookahead_plan(self, int(steps) * self._skip, self._skip, plan, rest, seed, t)

    def search(self, steps, depth, objective="return", rest=None, seed=0, t=0):
        """ToyboxVecEnv.search in agent steps: steps x skip raw frames, every action held for skip frames; raw frames, no wrapper,
        as in lookahead().  Between step_async and step_wait the step ends first."""
        if self._in_flight is not None:
            self.step_wait()
        return _search(self, int(steps) * self._skip, self._skip, depth, objective, rest, seed, t)

    def beam_search(self, steps, depth, width, objective="return", rest=None, seed=0, t=0):
        """ToyboxVecEnv.beam_search in agent steps: steps x skip raw frames, every action held for skip frames; raw frames, no
        wrapper, as in lookahead().  Between step_async and step_wait the step ends first."""
        if self._in_flight is not None:
            self.step_wait()
        return _beam(self, int(steps) * self._skip, self._skip, depth, width, objective, rest, seed, t)

    def evolve_search(self, steps, depth, population, generations, elite=None, mutation=None, plan_seed=0, init_plan=None, objective="return", rest=None,
                      seed=0, t=0):
        """ToyboxVecEnv.evolve_search in agent steps: steps x skip raw frames, every action held for skip frames; raw frames, no
        wrapper, as in lookahead().  Between step_async and step_wait the step ends first."""
        if self._in_flight is not None:
            self.step_wait()
        return _evolve(self, int(steps) * self._skip, self._skip, depth, population, generations, elite, mutation, plan_seed, init_plan, objective, rest, seed, t)

    def tree_search(self, steps, depth, simulations, explore=0, objective="return", rest=None, seed=0, t=0, salt=0):
        """ToyboxVecEnv.tree_search in agent steps: steps x skip raw frames, every action held for skip frames; raw frames, no
        wrapper, as in lookahead().  Between step_async and step_wait the step ends first."""
        if self._in_flight is not None:
            self.step_wait()
        return _tree(self, int(steps) * self._skip, self._skip, depth, simulations, explore, objective, rest, seed, t, salt)

    def plan_rollout(self, k, planner="evolve", steps=16, depth=4, objective="return", rest=None, seed=0, t=0, **planner_keywords):
        """ToyboxVecEnv.plan_rollout in agent steps (planner "tree" included: simulations, explore, salt, reuse; the trees of envs
        whose EPISODE ended -- a game over, not a lost life -- are dropped): per step the planner looks steps x skip raw frames ahead with hold = skip
        (on the engine pass hold = skip yourself: Engine.lookahead_act_device plans in raw frames) and ONE agent step
        (tbx_agent_step_device) plays the winner's first action, read from the device buffer the pick wrote; raw frames, no
        wrapper in the plan, as in lookahead().  k > 1 needs obs_layout="device_stack" (the host-side stacks of the other layouts
        take one plane per step).  Returns (obs after the last step, rewards float32 [k, num_envs], dones bool [k, num_envs],
        infos of the last step)."""
        if self._in_flight is not None:
            self.step_wait()
        if int(k) < 1:
            raise ValueError("plan_rollout takes k >= 1 steps")
        if int(k) > 1 and self.obs_layout != "device_stack":
            raise ValueError("plan_rollout with k > 1 needs obs_layout='device_stack'")
        if self._plan is None:
            self._plan = _PlanLoop(self)
        eng = self.engine
        reward, done = self._plan.run(int(k), planner, int(steps) * self._skip, self._skip, depth, objective, rest, seed, t, planner_keywords,
                                      lambda action, stream: eng.agent_step_device(action, stream=stream), _abi.BUF_AGENT_REWARD, 4, _abi.BUF_AGENT_DONE, 1, _abi.BUF_AGENT_EP_DONE)
        landed, key = self._landing()
        st = self._st
        eng.agent_fetch(ep_done=st["ep_done"], ep_return=st["ep_return"], ep_length=st["ep_length"], **{key: landed})
        last = done[-1, 0].astype(bool)
        ended = np.flatnonzero(st["ep_done"])
        ts = round(time.time() - self.tstart, 6) if len(ended) else 0.0
        extras = {int(i): {"episode": {"r": float(st["ep_return"][i]), "l": int(st["ep_length"][i]), "t": ts}} for i in ended}
        return self._obs(self._stacked_obs(landed, last, False)), reward[:, 0], done[:, 0].astype(bool), LazyInfos(self.num_envs, None, extras)

    def plan_step(self, planner="evolve", steps=16, depth=4, objective="return", rest=None, seed=0, t=0, **planner_keywords):
        """One closed-loop agent step, plan_rollout(1, ...).  Returns what step() returns."""
        obs, reward, done, infos = self.plan_rollout(1, planner, steps, depth, objective, rest, seed, t, **planner_keywords)
        return obs, reward[0], done[0], infos

    def plan_actions(self):
        """The action indices the last plan_step / plan_rollout chose, int64 [k, num_envs], read back from the device on demand"""
        if self._plan is None:
            raise RuntimeError("plan_actions before the first plan_step / plan_rollout")
        return self._plan.actions()

    def lookahead_samples(self, steps, samples, rest=None, seed=0, t=0, salt=0, objective="return"):
        """ToyboxVecEnv.lookahead_samples in agent steps: steps x skip raw frames, every action held for skip frames; raw frames,
        no wrapper, as in lookahead().  Between step_async and step_wait the step ends first."""
        if self._in_flight is not None:
            self.step_wait()
        return _samples(self, int(steps) * self._skip, self._skip, samples, rest, seed, t, salt, objective)

    def beam_search_samples(self, steps, depth, width, samples, objective="return", rest=None, seed=0, t=0, salt=0):
        """ToyboxVecEnv.beam_search_samples in agent steps: steps x skip raw frames, every action held for skip frames; raw
        frames, no wrapper, as in lookahead().  Between step_async and step_wait the step ends first."""
        if self._in_flight is not None:
            self.step_wait()
        return _beam_samples(self, int(steps) * self._skip, self._skip, depth, width, samples, objective, rest, seed, t, salt)

    def search_samples(self, steps, depth, samples, objective="return", rest=None, seed=0, t=0, salt=0):
        """ToyboxVecEnv.search_samples in agent steps: steps x skip raw frames, every action held for skip frames; raw frames,
        no wrapper, as in lookahead().  Between step_async and step_wait the step ends first."""
        if self._in_flight is not None:
            self.step_wait()
        return _search_samples(self, int(steps) * self._skip, self._skip, depth, samples, objective, rest, seed, t, salt)

    def close(self):
        if not self.closed:
            if self._in_flight is not None:
                try:
                    self.step_wait()
                except Exception:
                    pass
            if self._plan is not None:
                self._plan.close()
                self._plan = None
            self.engine.close()
            self.closed = True
