"""The agent observation at the edges of the output geometry (include/toybox_amd.h, tbx_agent_config_t: out_w <= 128,
out_h * out_w <= 7056, at most 8 source pixels per output pixel and axis), where the observation kernels change form:
each lane's second column slot (out_w > 64; column 127's window at the frame edge), all 8 column taps (the smallest out_w),
out_h = H (every scanline finishes an output row), the quad / dword / byte stack commits and the 16-byte ring commit
(out_h * out_w modulo 4 and 16, stack depth).

(a) the HIP library -- the per-game fused kernels and the generic warp kernel, in lockstep -- against the oracle, every
    output of every env at every agent step;
(b) the newest plane of the agent layer against the definition itself (an area average with exact rational weights, rounded
    half up, tests/support.py), from the frames of a twin engine without an agent layer: the fused kernels never build a
    full-resolution frame, so this is the only check of them that does not go through the oracle's warp."""
import numpy as np
import pytest

from support import FRAME_DIMS, agent_geometry_ok, area_resize_int, read_buffer, stack_from_ring, synthetic_actions
from toybox_amd import Engine, _abi

N = 257                                    # not a whole number of 4-wave blocks

# (game, out_h, out_w, stack, new_plane, stack_fill); the comment gives out_h * out_w and what the case is for
CASES = [
    ("breakout", 55, 128, 4, 0, 0),        # 7040 = 0 mod 16  out_w = 128 with the largest out_h
    ("breakout", 160, 35, 4, 2, 1),        # 5600 = 0 mod 16  out_h = H, smallest out_w (8 column taps), ring
    ("breakout", 23, 98, 3, 1, 0),         # 2254 = 2 mod 4   smallest out_h
    ("breakout", 147, 48, 4, 1, 1),        # 7056             non-square full plane, quad commit + dword plane
    ("breakout", 80, 64, 2, 0, 0),         # 5120             out_w = 64, integer row ratio
    ("breakout", 101, 65, 4, 0, 1),        # 6565 odd         out_w = 65, depth-4 byte commit
    ("breakout", 52, 61, 4, 2, 0),         # 3172 = 4 mod 16  ring, dword-size tail
    ("breakout", 40, 60, 1, 1, 0),         # 2400             integer ratio 4 x 4
    ("space_invaders", 55, 128, 4, 2, 0),  # 7040 = 0 mod 16  out_w = 128, ring
    ("space_invaders", 153, 46, 4, 0, 1),  # 7038 = 2 mod 4   smallest out_w with the largest out_h (sums near the 2^25 bound)
    ("space_invaders", 30, 101, 2, 1, 0),  # 3030 = 2 mod 4   smallest out_h
    ("space_invaders", 63, 112, 4, 1, 0),  # 7056             non-square full plane
    ("space_invaders", 105, 64, 3, 0, 1),  # 6720             out_w = 64, integer row ratio
    ("space_invaders", 105, 65, 4, 0, 0),  # 6825 odd         out_w = 65
    ("space_invaders", 70, 80, 1, 0, 0),   # 5600             integer ratio 3 x 4
    ("space_invaders", 66, 106, 4, 2, 1),  # 6996 = 4 mod 16  ring
    ("amidar", 55, 128, 4, 1, 1),          # 7040             out_w = 128
    ("amidar", 250, 23, 4, 0, 0),          # 5750 = 2 mod 4   out_h = H, smallest out_w
    ("amidar", 36, 77, 4, 2, 0),           # 2772 = 4 mod 16  smallest out_h, ring
    ("amidar", 196, 36, 2, 2, 1),          # 7056             non-square full plane, ring
    ("amidar", 100, 64, 4, 0, 1),          # 6400             out_w = 64
    ("amidar", 107, 65, 3, 1, 0),          # 6955 odd         out_w = 65
    ("amidar", 50, 32, 4, 0, 0),           # 1600             integer ratio 5 x 5
    ("gridworld", 55, 128, 4, 0, 1),       # 7040             out_w = 128
    ("gridworld", 128, 23, 4, 2, 0),       # 2944 = 0 mod 16  out_h = H, smallest out_w, ring
    ("gridworld", 19, 85, 3, 1, 0),        # 1615 odd         smallest out_h
    ("gridworld", 126, 56, 4, 1, 1),       # 7056             non-square full plane
    ("gridworld", 64, 64, 2, 0, 0),        # 4096             out_w = 64, integer row ratio
    ("gridworld", 102, 65, 4, 2, 1),       # 6630 = 2 mod 4   out_w = 65, ring byte form
    ("gridworld", 33, 40, 4, 2, 0),        # 1320 = 8 mod 16  ring
    ("gridworld", 32, 40, 1, 0, 1),        # 1280             integer ratio 4 x 4
]
STEPS, RESET_AT = 60, 30                   # agent steps (skip 2), and a second venv.reset() in the middle: every stack afresh


def _ids(c):
    return "%s-%dx%d-s%d-p%d-f%d" % c


def observation(e, n, oh, ow, stack, new_plane, obs):
    """uint8[N][oh][ow][slots]: the stack (new_plane 0), the stack and the newest plane as slot `stack` (1), or the ring read
    through its head, oldest first (2)"""
    if new_plane == 2:
        return stack_from_ring(read_buffer(e, _abi.BUF_AGENT_RING, (stack, n, oh, ow)), e.agent_ring_head())
    if new_plane == 1:
        return np.concatenate([obs, read_buffer(e, _abi.BUF_AGENT_PLANE, (n, oh, ow))[..., None]], axis=-1)
    return obs


def check_equal(got, want, what):
    """got / want uint8[N][oh][ow][slots]: the first differing (env, y, x, slot) and the number of envs that differ"""
    if np.array_equal(got, want):
        return
    n = got.shape[0]
    bad = np.flatnonzero((got != want).reshape(n, -1).any(axis=1))
    i = int(bad[0])
    y, x, c = (int(v) for v in np.argwhere(got[i] != want[i])[0])
    raise AssertionError("%s: first difference at env %d y=%d x=%d slot %d (got %d, want %d); %d envs of %d differ"
                         % (what, i, y, x, c, got[i, y, x, c], want[i, y, x, c], len(bad), n))


@pytest.mark.gpu
@pytest.mark.parametrize("game,oh,ow,stack,new_plane,fill", CASES, ids=[_ids(c) for c in CASES])
def test_gpu_observation_at_edge_geometry_equals_oracle(game, oh, ow, stack, new_plane, fill, hip_lib, oracle_lib):
    """The fused observation kernel and the generic warp kernel (OPT_AGENT_GENERIC) of the HIP library and the oracle, in
    lockstep from the same seed with EpisodicLifeEnv on: after every reset and agent step, the whole stack / plane / ring of
    every env, rewards, dones and the ring head are equal, byte for byte.  Skip 2: the max of two frames every step, the raw
    frame after a reset; a second reset in the middle starts every stack afresh (zeros, or the frame with stack_fill)."""
    H, W = FRAME_DIMS[game]
    assert agent_geometry_ok(H, W, oh, ow)
    engines = {"fused": Engine(game, N, lib=hip_lib), "generic": Engine(game, N, lib=hip_lib), "oracle": Engine(game, N, lib=oracle_lib)}
    engines["generic"].set_option(_abi.OPT_AGENT_GENERIC, 1)
    for e in engines.values():
        e.seed(1009)
        e.agent_init(skip=2, out_h=oh, out_w=ow, stack=stack, clip_reward=False, episodic_life=True, stack_fill=fill,
                     new_plane=new_plane)

    def compare(outs, step):
        o, r, d = outs["oracle"]
        want = observation(engines["oracle"], N, oh, ow, stack, new_plane, o)
        for path in ("fused", "generic"):
            g, rg, dg = outs[path]
            check_equal(observation(engines[path], N, oh, ow, stack, new_plane, g), want,
                        "%s %dx%d %s path, step %d" % (game, oh, ow, path, step))
            if r is not None:
                assert np.array_equal(rg, r) and np.array_equal(dg, d), "%s path, step %d: rewards / dones differ" % (path, step)
            if new_plane == 2:
                assert engines[path].agent_ring_head() == engines["oracle"].agent_ring_head(), (path, step)

    compare({k: (e.agent_reset(), None, None) for k, e in engines.items()}, -1)
    dones = 0
    for t in range(STEPS):
        a = synthetic_actions(game, N, t, seed=17)
        outs = {k: e.agent_step(a, tolerate_needs_reset=True) for k, e in engines.items()}
        compare(outs, t)
        dones += int(outs["oracle"][2].sum())
        if t == RESET_AT:
            compare({k: (e.agent_reset(), None, None) for k, e in engines.items()}, t)
    if game in ("breakout", "gridworld"):
        assert dones > 0                                        # envs restarted their stacks beside envs that rolled theirs
    for e in engines.values():
        e.close()


# (game, out_h, out_w, skip): a subset of CASES; skip 1 is the one-frame observation (MaxAndSkipEnv's slot A stays zero)
DEFINITION_CASES = [("breakout", 55, 128, 2), ("breakout", 160, 35, 3), ("breakout", 23, 98, 1),
                    ("space_invaders", 153, 46, 2), ("space_invaders", 55, 128, 2), ("space_invaders", 30, 101, 3),
                    ("amidar", 250, 23, 2), ("amidar", 55, 128, 1), ("amidar", 36, 77, 2),
                    ("gridworld", 128, 23, 2), ("gridworld", 55, 128, 3), ("gridworld", 19, 85, 2)]


def newest_plane_against_definition(lib, game, oh, ow, skip, n, steps, generic=False):
    """An agent engine without reset wrappers and a twin engine without an agent layer, same seed: the twin repeats every agent
    action `skip` times and renders gray frames after substeps skip-2 and skip-1 (MaxAndSkipEnv's buffer, zero until written);
    the agent engine's newest plane == area_resize_int(max(frame A, frame B)), for every env up to its first episode end (the
    twin does not reset)."""
    H, W = FRAME_DIMS[game]
    agent, twin = Engine(game, n, lib=lib), Engine(game, n, lib=lib)
    if generic:
        agent.set_option(_abi.OPT_AGENT_GENERIC, 1)
    for e in (agent, twin):
        e.seed(4242)
    agent.agent_init(skip=skip, out_h=oh, out_w=ow, stack=2, clip_reward=False)
    twin.new_game()
    what = "%s %dx%d skip %d%s" % (game, oh, ow, skip, " (generic path)" if generic else "")
    obs = agent.agent_reset()
    check_equal(obs[..., -1:], area_resize_int(twin.render(1)[..., 0], oh, ow)[..., None], what + ", reset (raw frame)")
    live = np.ones(n, bool)
    frame_a = np.zeros((n, H, W), np.uint8)
    for t in range(steps):
        a = synthetic_actions(game, n, t, seed=23)
        for k in range(skip):
            twin.step(a)
            if k == skip - 2:
                frame_a = twin.render(1)[..., 0]
            if k == skip - 1:
                frame_b = twin.render(1)[..., 0]
        obs, _, done = agent.agent_step(a)
        live &= ~np.asarray(done, bool)
        want = area_resize_int(np.maximum(frame_a, frame_b), oh, ow)
        got = np.where(live[:, None, None], obs[..., -1], want)             # envs past their first episode end are not compared
        check_equal(got[..., None], want[..., None], "%s, step %d" % (what, t))
    assert live.sum() > n // 2
    agent.close(); twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("game,oh,ow,skip", DEFINITION_CASES, ids=["%s-%dx%d-k%d" % c for c in DEFINITION_CASES])
def test_gpu_newest_plane_is_the_area_average_of_the_frames(game, oh, ow, skip, hip_lib):
    """The HIP library's fused observation kernel (and the generic warp kernel) against the definition, not the oracle."""
    for generic in (False, True):
        newest_plane_against_definition(hip_lib, game, oh, ow, skip, N, 30, generic)


@pytest.mark.parametrize("game,oh,ow,skip", DEFINITION_CASES[::3], ids=["%s-%dx%d-k%d" % c for c in DEFINITION_CASES[::3]])
def test_oracle_newest_plane_is_the_area_average_of_the_frames(game, oh, ow, skip, oracle_lib):
    """The oracle's agent layer the same way (what every GPU observation test compares the HIP library with)."""
    newest_plane_against_definition(oracle_lib, game, oh, ow, skip, 24, 20)


def right_edge_formations(engines, n):
    """SpaceInvaders states with the enemy formation pushed over the right edge of the frame by 64 .. 127 pixels (env i by
    64 + i % 64), after 140 played frames: the game's own frames are blank or flat in the columns of output column 127 at
    out_w = 128, so only such states show whether that column's window is its own.  No game reaches these states: they are
    artificial on purpose, written through set_states_np, and the test that uses them asserts that they still put something
    into column 127 (should set_states ever refuse or clamp them, it fails rather than passing without power).  The painters
    clip to the frame, so enemies partly or wholly off screen draw nothing outside it."""
    for e in engines:
        e.seed(17)
        e.new_game()
    for t in range(140):
        a = synthetic_actions("space_invaders", n, t, seed=4)
        for e in engines:
            e.step(a)
    recs = engines[-1].get_states_np()
    for i in range(n):
        ne = int(recs[i]["n_enemies"])
        recs[i]["enemies"]["x"][:ne] += 64 + i % 64
    for e in engines:
        e.set_states_np(0, recs)


@pytest.mark.gpu
@pytest.mark.parametrize("oh,stack,new_plane", [(55, 4, 0), (40, 3, 2)])
def test_gpu_observation_of_the_right_edge_column_at_out_w_128(oh, stack, new_plane, hip_lib, oracle_lib):
    """out_w = 128 with something to see in output column 127 (source columns 317.5 .. 320): the fused and the generic
    kernels == the oracle at every step, and the oracle's column 127 differs from its column 126 (the case has power)."""
    n = 64
    engines = [Engine("space_invaders", n, lib=hip_lib), Engine("space_invaders", n, lib=hip_lib), Engine("space_invaders", n, lib=oracle_lib)]
    engines[1].set_option(_abi.OPT_AGENT_GENERIC, 1)
    right_edge_formations(engines, n)
    for e in engines:
        e.agent_init(skip=2, out_h=oh, out_w=128, stack=stack, clip_reward=False, new_plane=new_plane)
    seen = 0
    for t in range(12):                                         # (no agent_reset: it would start new games)
        a = synthetic_actions("space_invaders", n, 200 + t, seed=4)
        outs = [e.agent_step(a, tolerate_needs_reset=True) for e in engines]
        want = observation(engines[2], n, oh, 128, stack, new_plane, outs[2][0])
        seen += int((want[:, :, 127] != want[:, :, 126]).any(axis=(1, 2)).sum())
        for e, out, path in zip(engines, outs, ("fused", "generic")):
            check_equal(observation(e, n, oh, 128, stack, new_plane, out[0]), want, "space_invaders %dx128 %s path, step %d" % (oh, path, t))
            assert np.array_equal(out[1], outs[2][1]) and np.array_equal(out[2], outs[2][2]), (path, t)
    assert seen > 0
    for e in engines:
        e.close()
