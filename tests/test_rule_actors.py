"""The rule-based actors (magent_amd/csrc/actors.hip, magent_amd/builtin/rule_model.py) on the CPU.

* the import surface of the reference's `magent.builtin.rule_model`;
* GridWorld.get_channel against observations of oracle worlds;
* the three host symbols against the compiled reference (oracle/_ref, called by its C++-mangled names): the same actions and the
  same libc random() state afterwards, on observations of oracle-driven pursuit, gather and battle episodes and on synthetic ones;
* the device kernels compiled against tests/hipemu (a library of their own): where they drew nothing, the host path's actions;
  where they drew, an action in the set the reference draws from (`possible_sets`, a numpy restatement).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H

ROOT = H.ROOT
LIBC = ctypes.CDLL(None)
LIBC.random.restype = ctypes.c_long
need_ref = pytest.mark.skipif(not H.have_ref(), reason="compiled reference (oracle/_ref) not present")

_vp, _i = ctypes.c_void_p, ctypes.c_int
REF_SYMBOLS = {   # the reference exports its boosters C++-mangled
    "runaway": ("_Z20runaway_infer_actionPfS_iiiiiPiii", [_vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _i]),
    "rush": ("_Z22rush_prey_infer_actionPfS_iiiiPiiiS0_f", [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, ctypes.c_float]),
    "gather": ("_Z19gather_infer_actionPfS_iiiiPiiS0_", [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp]),
}
PRODUCT_SYMBOLS = {"runaway": "runaway_infer_action", "rush": "rush_prey_infer_action", "gather": "gather_infer_action"}
KIND = {"runaway": 0, "rush": 1, "gather": 2}


def product():
    from magent_amd import c_lib
    if not os.path.exists(H.HIP_LIB):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return c_lib.load(H.HIP_LIB)


def reference(kind):
    lib = ctypes.CDLL(H.REF_LIB)
    name, argtypes = REF_SYMBOLS[kind]
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = None, argtypes
    return fn


def call(fn, kind, view, feat, p):
    """one call of a booster symbol (the reference's or the product's) with its own argument order -> int32[n]"""
    view = np.ascontiguousarray(view, dtype=np.float32)
    feat = np.ascontiguousarray(feat, dtype=np.float32)
    n, h, w, c = view.shape
    out = np.full(n, -7, dtype=np.int32)
    v2a = np.ascontiguousarray(p["v2a"], dtype=np.int32)
    if kind == "runaway":
        fn(view.ctypes.data, feat.ctypes.data, n, h, w, c, p["base"], out.ctypes.data, p["channel"], p["move_back"])
    elif kind == "rush":
        fn(view.ctypes.data, feat.ctypes.data, n, h, w, c, out.ctypes.data, p["channel"], p["base"], v2a.ctypes.data,
           ctypes.c_float(p["threshold"]))
    else:
        fn(view.ctypes.data, feat.ctypes.data, n, h, w, c, out.ctypes.data, p["base"], v2a.ctypes.data)
    return out


def assert_same_as_reference(kind, view, feat, p, seed, what=""):
    """byte-equal actions and the same libc state afterwards (the next random() agrees)"""
    H.single_threaded_reference()
    ref, mine = reference(kind), getattr(product(), PRODUCT_SYMBOLS[kind])
    LIBC.srandom(seed)
    want = call(ref, kind, view, feat, p)
    want_next = LIBC.random()
    LIBC.srandom(seed)
    got = call(mine, kind, view, feat, p)
    got_next = LIBC.random()
    bad = np.nonzero(want != got)[0]
    assert want.tobytes() == got.tobytes(), "%s: %d of %d actions differ, first %s: %s vs %s" % (
        what, len(bad), len(want), bad[:5], want[bad[:5]], got[bad[:5]])
    assert want_next == got_next, what + ": libc state differs afterwards"
    return want


# ---------------------------------------------------------------------------------------------- the numpy restatement
def _get_action(dr, dc, stride):
    if dr < 0:
        return 1 if dc < 0 else ((0 if stride else 2) if dc == 0 else 3)
    if dr == 0:
        return (4 if stride else 5) if dc < 0 else (6 if dc == 0 else (8 if stride else 7))
    return 9 if dc < 0 else ((12 if stride else 10) if dc == 0 else 11)


def possible_sets(kind, view, feat, p):
    """-> (drew bool[n], list of sets): which agents' reference actions come from a draw, and the set each draws from
    (None where nothing is drawn)"""
    n, h, w, c = view.shape
    base, v2a = p["base"], np.asarray(p["v2a"]).reshape(h, w)
    drew, sets = np.zeros(n, dtype=bool), [None] * n
    flat_feat = np.ascontiguousarray(feat, dtype=np.float32).reshape(-1)
    every = set(range(base))
    for i in range(n):
        o = view[i]
        if kind == "runaway":
            continue
        if kind == "rush":
            if not flat_feat[i] < np.float32(p["threshold"]):
                drew[i], sets[i] = True, every
                continue
            hit = (o[:, :, p["channel"]] > 0.5) | (o[:, :, 1] > 0.5)
            if (hit & (v2a != -1)).any():
                continue
            if hit.any() and int(float(o[h - 1, w // 2, 0]) + 0.5) != 1:
                continue
            drew[i], sets[i] = True, every
            continue
        food = o[:, :, 4] == np.float32(1.0)
        att = food & (v2a != -1)
        if att.any():
            drew[i], sets[i] = True, set((v2a[att] + base).tolist())
            continue
        disp = np.argwhere(food & (v2a == -1))
        if len(disp):
            dr, dc = disp[0][0] - h // 2, disp[0][1] - w // 2
            if dr == dc and abs(dc) == 1:
                drew[i], sets[i] = True, {_get_action(0, dc, False), _get_action(dr, 0, False)}
            continue
        me = np.argwhere(o[:, :, 3] > 1.0)
        mr, mc = (me[-1][0], me[-1][1]) if len(me) else (-1, -1)
        s = set()
        for r, cc in np.argwhere(o[:, :, 6] > 0.0):
            a = _get_action(r - mr, cc - mc, True)
            s |= every if a == 6 else {a}
        drew[i], sets[i] = True, (s if s else every)
    return drew, sets


def gather_divides_by_zero(view, p):
    """agents for which the reference's gather reaches its minimap step with no minimap cell (a division by zero there)"""
    food = view[:, :, :, 4] == np.float32(1.0)
    return ~food.any(axis=(1, 2)) & ~(view[:, :, :, 6] > 0.0).any(axis=(1, 2))


# ---------------------------------------------------------------------------------------------- worlds
def episode(game, size, settings, counts, acting, steps, seed, lib=None):
    """observations {group: (view, feature)} of every step of an episode of random actions on a world of `lib` (the oracle)"""
    cfg = H.config_for(game, size)
    cfg.set(settings)
    env = H.gridworld(cfg, lib=lib or H.ensure_oracle())
    env.set_seed(seed)
    env.reset()
    hs = env.get_handles()
    for h, n in zip(hs, counts):
        env.add_agents(h, "random", n=n)
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        out.append({h.value: tuple(np.array(a) for a in env.get_observation(h)) for h in hs})
        for g in acting:
            env.set_action(hs[g], rs.randint(env.get_action_space(hs[g])[0], size=env.get_num(hs[g])).astype(np.int32))
        env.step()
        env.clear_dead()
    return env, out


def actor_params(env, kind, handle, other=None, threshold=100.0):
    base, v2a = env.get_view2attack(handle)
    p = {"base": base, "v2a": v2a, "threshold": threshold, "move_back": 4, "channel": 0}
    if other is not None:
        p["channel"] = env.get_channel(other, handle)
    return p


# ---------------------------------------------------------------------------------------------- import surface
def test_rule_model_exports_the_reference_actors():
    from magent.builtin.rule_model import RandomActor, RunawayPrey, RushGatherer, RushPredator  # noqa: F401
    import magent.builtin.rule_model as rm
    assert sorted(rm.__all__) == ["RandomActor", "RunawayPrey", "RushGatherer", "RushPredator"]


def test_header_declares_the_reference_boosters():
    text = open(os.path.join(ROOT, "include", "magent_runtime_api.h")).read()
    for name in PRODUCT_SYMBOLS.values():
        assert "void %s(" % name in text
    out = subprocess.run(["nm", "-D", "--defined-only", product()._name], capture_output=True, text=True).stdout.split()
    for name in list(PRODUCT_SYMBOLS.values()) + ["actor_infer_action_device"]:
        assert name in out, name       # unmangled C symbols


# ---------------------------------------------------------------------------------------------- get_channel
def _lattice_world(game, size, settings, rs, skip=None):
    """every group placed on slots of a sparse lattice (2x2 bodies fit), group `skip` left out; the same slots with or without it"""
    cfg = H.config_for(game, size)
    cfg.set(settings)
    env = H.gridworld(cfg, lib=H.ensure_oracle())
    env.set_seed(3)
    env.reset()
    slots = [(x, y) for x in range(2, size - 3, 4) for y in range(2, size - 3, 4)]
    order = rs.permutation(len(slots))
    hs = env.get_handles()
    per = len(slots) // len(hs)
    for k, h in enumerate(hs):
        if k == skip:
            continue
        env.add_agents(h, "custom", pos=[slots[j] for j in order[k * per:(k + 1) * per]])
    return env


@pytest.mark.parametrize("game,settings", [("pursuit", {}), ("pursuit", {"food_mode": True}), ("gather", {}),
                                           ("battle", {}), ("battle", {"minimap_mode": False})])
def test_get_channel_names_the_group_layers_in_the_observers_view(game, settings):
    """a group left out of a world changes only its own layers (has, hp[, minimap]) of every other group's view, which start at
    get_channel(group, observer); an observer always sees itself in get_channel(observer, observer)"""
    probe = _lattice_world(game, 40, settings, np.random.RandomState(0))
    hs = probe.get_handles()
    n_group = len(hs)
    cfg_food, cfg_mm = probe._channel_modes["food_mode"], probe._channel_modes["minimap_mode"]
    scale = 2 + cfg_mm
    for h in hs:
        assert probe.get_channel(h) == 1 + cfg_food + h.value * scale
    for obs in range(n_group):
        full = _lattice_world(game, 40, settings, np.random.RandomState(0))
        view = full.get_observation(full.get_handles()[obs])[0].copy()
        ch = full.get_channel(obs, obs)
        assert ch == 1 + cfg_food and (view[:, :, :, ch] > 0).any(axis=(1, 2)).all()
        for other in range(n_group):
            if other == obs:
                continue
            part = _lattice_world(game, 40, settings, np.random.RandomState(0), skip=other)
            pview = part.get_observation(part.get_handles()[obs])[0]
            changed = sorted(np.nonzero((view != pview).any(axis=(0, 1, 2)))[0].tolist())
            first = full.get_channel(other, obs)
            assert changed and set(changed) <= set(range(first, first + scale)), (game, settings, obs, other, changed, first)
            if view.shape[1] >= 5:      # (a 3 x 3 view -- gather's food -- sees no neighbour on the lattice: its minimap layer only)
                assert first in changed, (game, settings, obs, other, changed, first)
    if game == "pursuit":      # the issue's example: the prey's predator layers are channel 3
        assert probe.get_channel(0, 1) == 3 + cfg_food


# ---------------------------------------------------------------------------------------------- host symbols vs the reference
WORLDS = {   # name -> (game, map size, settings, agents per group, acting groups, steps)
    "pursuit": ("pursuit", 40, {}, (40, 80), (0, 1), 8),
    "pursuit_food": ("pursuit", 40, {"food_mode": True}, (40, 80), (0, 1), 6),
    "gather": ("gather", 60, {}, (300, 200), (1,), 8),
    "battle": ("battle", 40, {}, (250, 250), (0, 1), 8),
    "battle_nominimap": ("battle", 40, {"minimap_mode": False}, (200, 200), (0, 1), 5),
}
_EPISODES = {}


def world_obs(name):
    if name not in _EPISODES:
        game, size, settings, counts, acting, steps = WORLDS[name]
        _EPISODES[name] = episode(game, size, settings, counts, acting, steps, seed=11)
    return _EPISODES[name]


@need_ref
@pytest.mark.parametrize("name", ["pursuit", "pursuit_food", "battle", "battle_nominimap"])
def test_rush_and_runaway_match_the_reference(name):
    env, steps = world_obs(name)
    hs = env.get_handles()
    for t, obs in enumerate(steps):
        for me, other in ((0, 1), (1, 0)):
            view, feat = obs[me]
            if not len(view):
                continue
            for seed in (1, 12345 + t):
                p = actor_params(env, "runaway", hs[me], hs[other])
                assert_same_as_reference("runaway", view, feat, p, seed, "%s step %d runaway %d" % (name, t, me))
                for threshold in (100.0, 0.5):
                    p = actor_params(env, "rush", hs[me], hs[other], threshold)
                    assert_same_as_reference("rush", view, feat, p, seed, "%s step %d rush %d thr %g" % (name, t, me, threshold))


@need_ref
def test_gather_matches_the_reference():
    env, steps = world_obs("gather")
    h = env.get_handles()[1]
    p = actor_params(env, "gather", h)
    seen = np.zeros(4, dtype=int)
    for t, obs in enumerate(steps):
        view, feat = obs[1]
        keep = ~gather_divides_by_zero(view, p)
        view, feat = view[keep], feat[keep]
        for seed in (2, 777 + t):
            assert_same_as_reference("gather", view, feat, p, seed, "gather step %d" % t)
        drew, sets = possible_sets("gather", view, feat, p)
        seen += np.bincount([0 if s is None else min(len(s), 3) for s in sets], minlength=4)
    assert seen[0] > 0 and seen[1:].sum() > 0, seen        # both kinds of agent occur


def synthetic(kind, n, h, w, c, rs, density=0.08):
    """sparse observations that reach every branch: 0 mostly, then 1.0, 0.5 (not > 0.5), 2.0 (> 1), 0.7"""
    view = np.zeros((n, h, w, c), dtype=np.float32)
    mask = rs.rand(n, h, w, c) < density
    view[mask] = rs.choice(np.array([1.0, 0.5, 2.0, 0.7], dtype=np.float32), size=int(mask.sum()))
    view[:, h - 1, w // 2, 0] = rs.rand(n) < 0.3            # the wall in front
    feat = (rs.rand(n, 5) * 150).astype(np.float32)          # (the threshold test reads the flattened array)
    v2a = -np.ones((h, w), dtype=np.int32)
    cells = rs.permutation(h * w)[:12]
    v2a.reshape(-1)[cells] = np.arange(len(cells))           # (a view of fewer than 12 cells: all of them)
    return view, feat, {"base": 13, "v2a": v2a, "threshold": 100.0, "move_back": 4, "channel": 3 if kind != "gather" else 0}


@need_ref
@pytest.mark.parametrize("kind", ["runaway", "rush", "gather"])
def test_synthetic_observations_match_the_reference(kind):
    rs = np.random.RandomState(KIND[kind])
    for shape in ((300, 13, 13, 7), (200, 15, 15, 7), (100, 9, 11, 8)):
        view, feat, p = synthetic(kind, *shape, rs)
        if kind == "gather":
            keep = ~gather_divides_by_zero(view, p)
            view, feat = view[keep], feat[keep]
        for seed in (5, 99):
            assert_same_as_reference(kind, view, feat, p, seed, "%s %s" % (kind, shape))


def test_gather_without_a_minimap_cell_draws_once():
    """the case the reference divides by zero on: no food in view and no minimap cell -> one rand() % attack_base"""
    lib = product()
    rs = np.random.RandomState(4)
    view, feat, p = synthetic("gather", 40, 13, 13, 7, rs)
    view[:, :, :, 4] = 0
    view[:, :, :, 6] = 0
    for seed in (1, 8):
        LIBC.srandom(seed)
        want = np.array([LIBC.rand() % p["base"] for _ in range(len(view))], dtype=np.int32)
        want_next = LIBC.random()
        LIBC.srandom(seed)
        got = call(lib.gather_infer_action, "gather", view, feat, p)
        assert got.tobytes() == want.tobytes() and LIBC.random() == want_next


def test_actors_on_numpy_observations_call_the_host_symbols():
    """RushPredator / RunawayPrey / RushGatherer on numpy observations: the host symbols, with the reference's constants and
    get_channel(other, self)"""
    from magent.builtin.rule_model import RunawayPrey, RushGatherer, RushPredator
    lib = product()
    env, steps = world_obs("pursuit")
    pred, prey = env.get_handles()
    view_p, feat_p = steps[2][0]
    view_q, feat_q = steps[2][1]
    a, b = RushPredator(env, pred, prey), RunawayPrey(env, prey, pred)
    assert (a.attack_channel, b.away_channel, b.move_back, a.threshold) == (3, 3, 4, 100.0)
    LIBC.srandom(3)
    got = a.infer_action((view_p, feat_p))
    LIBC.srandom(3)
    want = call(lib.rush_prey_infer_action, "rush", view_p, feat_p, actor_params(env, "rush", pred, prey))
    assert got.dtype == np.int32 and got.tobytes() == want.tobytes()
    got = b.infer_action((view_q, feat_q))
    assert got.tobytes() == call(lib.runaway_infer_action, "runaway", view_q, feat_q, actor_params(env, "runaway", prey, pred)).tobytes()
    genv, gsteps = world_obs("gather")
    g = RushGatherer(genv, genv.get_handles()[1])
    view, feat = gsteps[1][1]
    LIBC.srandom(9)
    got = g.infer_action((view, feat))
    LIBC.srandom(9)
    assert got.tobytes() == call(lib.gather_infer_action, "gather", view, feat, actor_params(genv, "gather", genv.get_handles()[1])).tobytes()
    assert RushPredator(env, pred, prey).infer_action((view_p[:0], feat_p[:0])).shape == (0,)


def test_bf16_observations_are_refused():
    torch = pytest.importorskip("torch")
    from magent.builtin.rule_model import RushPredator
    env, steps = world_obs("pursuit")
    pred, prey = env.get_handles()
    view = torch.zeros((4,) + env.get_view_space(pred)[:2] + (8,), dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="bf16"):
        RushPredator(env, pred, prey).infer_action((view, torch.zeros(4, 3)))


# ---------------------------------------------------------------------------------------------- the device kernels, emulated
EMU_DIR = os.path.join(ROOT, "tests", "hipemu", "_build", "actors")
EMU_LIB = os.path.join(EMU_DIR, "libactors_emu.so")


def build_actor_emu():
    """actors.hip alone, compiled as plain C++ against tests/hipemu (hipemu.build's compiler, flags and LDS rewrite), into a
    library of its own; its headers are copied beside it so that nothing stale from the engine's emulated build is found first"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build as emu_build
    import fcntl
    csrc = emu_build.CSRC
    deps = [os.path.join(csrc, f) for f in ("actors.hip", "actors_dev.h")] + [
        os.path.join(ROOT, "include", "magent_runtime_api.h"), os.path.join(emu_build.HERE, "emu_runtime.cc"),
        os.path.join(emu_build.HERE, "hip", "hip_runtime.h"), os.path.abspath(__file__)]
    os.makedirs(EMU_DIR, exist_ok=True)
    with open(os.path.join(EMU_DIR, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if os.path.exists(EMU_LIB) and all(os.path.getmtime(d) <= os.path.getmtime(EMU_LIB) for d in deps):
            return EMU_LIB
        sub = lambda text: emu_build.DYN.sub(lambda m: "%s *%s = (%s *)hipemu::dynamic_lds();" % (m.group(1), m.group(2), m.group(1)), text)
        src = os.path.join(csrc, "actors_dev.h")
        open(os.path.join(EMU_DIR, "actors_dev.h"), "w").write('#line 1 "%s"\n' % src + sub(open(src).read()))
        src = os.path.join(csrc, "actors.hip")
        cc = os.path.join(EMU_DIR, "actors_emu.cc")
        open(cc, "w").write('#line 1 "%s"\n' % src + sub(open(src).read()).replace('"../../include/', '"'))
        objs = [cc.replace(".cc", ".o"), os.path.join(EMU_DIR, "emu_runtime.o")]
        subprocess.check_call([emu_build.CXX] + emu_build.FLAGS + ["-c", cc, "-o", objs[0]])
        subprocess.check_call([emu_build.CXX] + emu_build.FLAGS + ["-c", os.path.join(emu_build.HERE, "emu_runtime.cc"), "-o", objs[1]])
        tmp = EMU_LIB + ".%d.tmp" % os.getpid()
        subprocess.check_call([emu_build.CXX, "-shared", "-fPIC", "-o", tmp] + objs + ["-Wl,-Bsymbolic", "-lpthread"])
        os.replace(tmp, EMU_LIB)
    return EMU_LIB


class ActorArgs(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("n", ctypes.c_int), ("height", ctypes.c_int), ("width", ctypes.c_int),
                ("n_channel", ctypes.c_int), ("attack_base", ctypes.c_int), ("channel", ctypes.c_int), ("move_back", ctypes.c_int),
                ("threshold", ctypes.c_float), ("seed", ctypes.c_ulonglong), ("counter", ctypes.c_ulonglong)]


def device_call(lib_path, kind, view, feat, p, seed=1, counter=0):
    """actor_infer_action_device of the emulated library (its "device" memory is the host heap) -> (actions, drew)"""
    lib = ctypes.CDLL(lib_path, mode=os.RTLD_LOCAL)
    fn = lib.actor_infer_action_device
    fn.restype, fn.argtypes = ctypes.c_int, [_vp] * 7
    view = np.ascontiguousarray(view, dtype=np.float32)
    feat = np.ascontiguousarray(feat, dtype=np.float32)
    n, h, w, c = view.shape
    v2a = np.ascontiguousarray(p["v2a"], dtype=np.int32)
    act, drew = np.full(n, -7, dtype=np.int32), np.full(n, 9, dtype=np.uint8)
    a = ActorArgs(KIND[kind], n, h, w, c, p["base"], p["channel"], p["move_back"], p["threshold"], seed, counter)
    assert fn(ctypes.byref(a), view.ctypes.data, feat.ctypes.data, v2a.ctypes.data, act.ctypes.data, drew.ctypes.data, None) == 0
    return act, drew


def check_device_actions(kind, view, feat, p, act, drew, host, what=""):
    """drew == 0: the host path's action; drew == 1: an action in the reference's set; drew as the reference draws"""
    want_drew, sets = possible_sets(kind, view, feat, p)
    assert drew.dtype == np.uint8 and set(np.unique(drew).tolist()) <= {0, 1}, what
    assert (drew.astype(bool) == want_drew).all(), "%s: drew differs at %s" % (what, np.nonzero(drew.astype(bool) != want_drew)[0][:5])
    exact = drew == 0
    assert (act[exact] == host[exact]).all(), "%s: exact actions differ at %s" % (what, np.nonzero(exact & (act != host))[0][:5])
    for i in np.nonzero(~exact)[0]:
        assert int(act[i]) in sets[i], (what, i, int(act[i]), sets[i])


def emu_cases():
    """(kind, view, feature, params) from the oracle worlds and synthetic observations"""
    out = []
    env, steps = world_obs("pursuit")
    pred, prey = env.get_handles()
    for t in (0, 4):
        out.append(("runaway", steps[t][1][0], steps[t][1][1], actor_params(env, "runaway", prey, pred)))
        out.append(("rush", steps[t][0][0], steps[t][0][1], actor_params(env, "rush", pred, prey)))
    env, steps = world_obs("battle")
    b0, b1 = env.get_handles()
    out.append(("rush", steps[3][0][0][:120], steps[3][0][1][:120], actor_params(env, "rush", b0, b1, threshold=2.0)))
    env, steps = world_obs("gather")
    for t in (0, 5):
        out.append(("gather", steps[t][1][0][:150], steps[t][1][1][:150], actor_params(env, "gather", env.get_handles()[1])))
    rs = np.random.RandomState(21)
    for kind in ("runaway", "rush", "gather"):
        out.append((kind,) + synthetic(kind, 70, 13, 13, 7, rs))
        out.append((kind,) + synthetic(kind, 33, 7, 9, 8, rs, density=0.03))
    return out


def test_emulated_kernels_match_the_host_path():
    lib = build_actor_emu()
    prod = product()
    for k, (kind, view, feat, p) in enumerate(emu_cases()):
        LIBC.srandom(1)
        host = call(getattr(prod, PRODUCT_SYMBOLS[kind]), kind, view, feat, p)
        act, drew = device_call(lib, kind, view, feat, p, seed=k + 1)
        check_device_actions(kind, view, feat, p, act, drew, host, "%s case %d" % (kind, k))
        again = device_call(lib, kind, view, feat, p, seed=k + 1)
        assert (again[0] == act).all()
        if drew.any():
            other = device_call(lib, kind, view, feat, p, seed=k + 1, counter=1)
            assert (other[1] == drew).all() and (other[0][drew == 0] == act[drew == 0]).all()
    act, drew = device_call(lib, "rush", np.zeros((0, 5, 5, 7), np.float32), np.zeros((0, 3), np.float32),
                            {"base": 3, "v2a": np.zeros((5, 5), np.int32), "channel": 3, "move_back": 4, "threshold": 1.0})
    assert act.shape == (0,)


def test_emulated_kernels_do_not_depend_on_lane_order():
    """the same under scrambled lane and workgroup orders (a subprocess each: the order is fixed when the library starts)"""
    lib = build_actor_emu()
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np, test_rule_actors as T\n"
            "out = [T.device_call(T.EMU_LIB, kind, v, f, p, seed=3) for kind, v, f, p in T.emu_cases()]\n"
            "np.save(sys.argv[1], np.concatenate([np.concatenate([a, d.astype(np.int32)]) for a, d in out]))\n") % (ROOT, os.path.join(ROOT, "tests"))
    results = []
    for seed in ("0", "1", "7"):
        path = os.path.join(EMU_DIR, "scramble_%s.npy" % seed)
        env = dict(os.environ, OMP_NUM_THREADS="1")
        if seed != "0":
            env["HIPEMU_SCRAMBLE"] = seed
        p = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
        results.append(np.load(path))
    assert lib and all((r == results[0]).all() for r in results[1:])
