"""Shared scenario driver for the parity tests.

One driver, three engines: the product (HIP, magent_amd/lib/libmagent.so), the CPU restatement
(oracle/liboracle.so) and -- when present -- the compiled reference (oracle/_ref/libmagent_ref.so).
All are driven through the same magent_amd.GridWorld wrapper with the same seeds and action streams.
"""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np

import magent_amd
from magent_amd import gridworld as gw  # noqa: F401
from magent_amd.builtin.config import _games

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_LIB = os.path.join(ROOT, "oracle", "liboracle.so")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libmagent_ref.so")
HIP_LIB = os.path.join(ROOT, "magent_amd", "lib", "libmagent.so")
PRODUCT_LIB = HIP_LIB          # (tools/fuzz_parity.py points HIP_LIB at the emulated build when asked for "emu")
EMU_LIB = os.path.join(ROOT, "tests", "hipemu", "_build", "libmagent_emu.so")


def ensure_emu():
    """the engine's HIP sources compiled as plain C++ against tests/hipemu (kernels run lane by lane on the CPU): a checker of
    the kernels' logic for the GPU-less build container, never the product"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build as emu_build
    return emu_build.build()
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def build_policy_emu(name, sources, headers, caller):
    """`sources` (of magent_amd/csrc) compiled as plain C++ against tests/hipemu (hipemu.build's compiler, flags and LDS rewrite) into a
    library of their own, tests/hipemu/_build/<name>/lib<name>_emu.so; `headers` are copied beside them so that nothing stale from the
    engine's emulated build is found first.  Rebuilt when a source, a header, the emulator, this file or `caller` (the test file) is newer."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build as emu_build
    import fcntl
    csrc = emu_build.CSRC
    out = os.path.join(ROOT, "tests", "hipemu", "_build", name)
    lib = os.path.join(out, "lib%s_emu.so" % name)
    deps = [os.path.join(csrc, f) for f in headers + sources] + [
        os.path.join(ROOT, "include", "magent_policy.h"), os.path.join(emu_build.HERE, "emu_runtime.cc"),
        os.path.join(emu_build.HERE, "hip", "hip_runtime.h"), os.path.abspath(__file__), os.path.abspath(caller)]
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if os.path.exists(lib) and all(os.path.getmtime(d) <= os.path.getmtime(lib) for d in deps):
            return lib
        sub = lambda text: emu_build.DYN.sub(lambda m: "%s *%s = (%s *)hipemu::dynamic_lds();" % (m.group(1), m.group(2), m.group(1)),
                                             text).replace('"../../include/', '"')
        for h in headers:
            src = os.path.join(csrc, h)
            open(os.path.join(out, h), "w").write('#line 1 "%s"\n' % src + sub(open(src).read()))
        objs = []
        for f in sources:
            src = os.path.join(csrc, f)
            cc = os.path.join(out, f.replace(".hip", "_emu.cc"))
            open(cc, "w").write('#line 1 "%s"\n' % src + sub(open(src).read()))
            objs.append(cc.replace(".cc", ".o"))
            subprocess.check_call([emu_build.CXX] + emu_build.FLAGS + ["-c", cc, "-o", objs[-1]])
        objs.append(os.path.join(out, "emu_runtime.o"))
        subprocess.check_call([emu_build.CXX] + emu_build.FLAGS + ["-c", os.path.join(emu_build.HERE, "emu_runtime.cc"), "-o", objs[-1]])
        tmp = lib + ".%d.tmp" % os.getpid()
        subprocess.check_call([emu_build.CXX, "-shared", "-fPIC", "-o", tmp] + objs + ["-Wl,-Bsymbolic", "-lpthread"])
        os.replace(tmp, lib)
    return lib


# The emulated library of every policy source set: name -> (sources, headers copied beside them).  One list per set, here and nowhere
# else: a block that moves to another header cannot leave a stale list behind in a test file.  "policy": all six, for tools/policy_bits.py.
_POLICY_HEADERS = ["policy_bf16_dev.h", "policy_f32_dev.h", "policy_host.h", "tune.h"]
POLICY_EMU = {
    "drqn": (["policy_f32.hip", "policy_drqn_f32.hip"], _POLICY_HEADERS[1:]),
    "a2c": (["policy_a2c_f32.hip"], _POLICY_HEADERS[1:3]),
    "drqn_bf16": (["policy.hip", "policy_drqn_bf16.hip"], _POLICY_HEADERS),
    "a2c_bf16": (["policy_a2c_bf16.hip"], _POLICY_HEADERS[:3]),
    "policy": (["policy.hip", "policy_f32.hip", "policy_drqn_f32.hip", "policy_drqn_bf16.hip", "policy_a2c_f32.hip", "policy_a2c_bf16.hip"], _POLICY_HEADERS),
}


def policy_emu(name):
    """the emulated library of the policy source set `name` (POLICY_EMU), built by build_policy_emu"""
    return build_policy_emu(name, POLICY_EMU[name][0], POLICY_EMU[name][1], __file__)


class PolicyLeg(object):
    """one of the two legs of a policy-kernel test.  `emu`: an emulated build (`emu_lib()` returns its path) on CPU tensors, with
    MAGENT_TUNE=`tune` if given (read at the library's first call); `gpu`: the product library on cuda:0.
    policy(...): the leg's `policy_class` of hip_policy (the emulated leg hands it its library)."""

    def __init__(self, name, emu_lib, tune=None, policy_class=None):
        import ctypes
        import torch
        from magent_amd import c_lib
        self.name, self.policy_class = name, policy_class
        if name == "emu":
            if tune:
                os.environ.setdefault("MAGENT_TUNE", tune)
            self.lib = c_lib.declare_policy(ctypes.CDLL(emu_lib(), mode=os.RTLD_LOCAL))
            self.dev = torch.device("cpu")
        else:
            self.lib = c_lib.load()
            self.dev = torch.device("cuda", 0)

    def policy(self, net, vs, feat, A, chunk=131072):
        from magent_amd.builtin.torch_model import hip_policy
        return getattr(hip_policy, self.policy_class)(net, vs, (feat,), A, self.dev, chunk=chunk, lib=self.lib if self.name == "emu" else None)

    def sync(self):
        import torch
        if self.dev.type == "cuda":
            torch.cuda.synchronize()


def policy_legs(emu_lib, tune=None, policy_class=None):
    """(leg, LEGS) of a test module: leg(name) makes the module's PolicyLeg at first use; LEGS parametrises a test over both legs"""
    import pytest
    made = {}

    def leg(name):
        if name not in made:
            made[name] = PolicyLeg(name, emu_lib, tune, policy_class)
        return made[name]
    return leg, ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


def make_policy_inputs(view_space, feat, n, seed, extra=0, fill=0.0):
    """observation-like view (sparse, fractions) and features [n + extra]; the `extra` rows behind the n agents hold `fill`"""
    import torch
    g = torch.Generator().manual_seed(seed)
    view = (torch.rand((n + extra,) + view_space, generator=g) < 0.3).float() * torch.rand((n + extra,) + view_space, generator=g)
    featv = torch.rand((n + extra, feat), generator=g) * 2 - 0.5
    view[n:] = fill
    featv[n:] = fill
    return view, featv


def make_rnet(vs, feat, A, dueling, seed, dev="cpu", scale=3.0):
    import torch
    from magent_amd.builtin.torch_model.drqn import _RecurrentQNet
    torch.manual_seed(seed)
    q = _RecurrentQNet(vs, (feat,), A, dueling)
    with torch.no_grad():
        for p in q.parameters():          # larger weights than the default init: every layer matters in Q and in the gates
            p.mul_(scale)
    return q.to(dev)


class DictModel(object):
    """the Python-dict path's state semantics (drqn.py: agent_states), over the kernels' own output rows (S units each)"""

    def __init__(self, S=512):
        self.states, self.S = {}, S

    def lookup(self, ids):
        zero = np.zeros(self.S, np.float32)
        return np.stack([self.states.get(int(i), zero) for i in ids]) if len(ids) else np.zeros((0, self.S), np.float32)

    def store(self, ids, h):
        self.states = {int(i): h[k] for k, i in enumerate(ids)}


def cells_of(view):
    """the engine's bf16 cells of a float32 view (a torch tensor; on its device), as env_get_observation_device_bf16 defines them: the
    channels rounded to nearest even, zeros, 1.0 in channel 7"""
    import torch
    n, h, w, c = view.shape
    cells = torch.zeros((n, h, w, 8), dtype=torch.bfloat16, device=view.device)
    cells[..., :c] = view.to(torch.bfloat16)
    cells[..., 7] = 1.0
    return cells


class SpacesEnv(object):          # a model's constructor reads the spaces only
    device_id = 0

    def __init__(self, vs=(9, 9, 5), feat=20, A=13):
        self.vs, self.feat, self.A = vs, feat, A

    def get_view_space(self, h):
        return self.vs

    def get_feature_space(self, h):
        return (self.feat,)

    def get_action_space(self, h):
        return (self.A,)


def battle(seed, device_obs=True, n=300, size=40):
    """a battle of n random agents a side on the product engine with device-resident observations (True: float32 views, "bf16": cells)"""
    env = magent_amd.GridWorld("battle", map_size=size, device_obs=device_obs)
    env.set_seed(seed)
    env.reset()
    hs = env.get_handles()
    for h in hs:
        env.add_agents(h, "random", n=n)
    return env, hs


def net_params(net):
    """a module's state_dict as float64 NumPy arrays"""
    return {k: v.detach().cpu().double().numpy() for k, v in net.state_dict().items()}


def merge_env(*dicts):
    """environment dicts merged; MAGENT_TUNE entries (magent_amd/csrc/tune.h: "key=value,key=value") are joined, not overwritten"""
    out = {}
    for d in dicts:
        for k, v in d.items():
            out[k] = out[k] + "," + v if k == "MAGENT_TUNE" and out.get(k) else v
    return out


def ensure_oracle():
    """build oracle/liboracle.so from its own source if needed (gcc only; no GPU involved)"""
    src = os.path.join(ROOT, "oracle", "gridworld_oracle.cc")
    if not os.path.exists(ORACLE_LIB) or os.path.getmtime(ORACLE_LIB) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "liboracle.so"])
    return ORACLE_LIB


def have_ref():
    return os.path.exists(REF_LIB)


def single_threaded_reference():
    """the compiled reference's attack loop is order-nondeterministic with more than one OpenMP thread.  The
    OMP_NUM_THREADS=1 of tests/conftest.py only counts if the OpenMP runtime starts after it was set: in a process where something
    started it earlier, under the host's own OMP_NUM_THREADS, the reference ran multithreaded and its trajectories drifted.  So the
    calling thread's team size is set through the runtime itself, whenever a world of the reference is made."""
    import ctypes
    ref = ctypes.CDLL(REF_LIB)          # (the reference links the OpenMP runtime: its symbols resolve through this handle)
    ref.omp_set_num_threads(1)
    assert ref.omp_get_max_threads() == 1


_WORLDS = {}


def is_emu(lib):
    return lib is not None and os.path.abspath(lib) == os.path.abspath(EMU_LIB)


def torch_device(env, lib):
    """where the caller-owned "device" tensors of the *_device API live: the GPU -- or, for the emulated library, host memory
    (its HBM is the host heap, a CPU tensor's data_ptr() is a valid device pointer there)"""
    import torch
    return torch.device("cpu") if is_emu(lib) else torch.device("cuda", env.device_id)


def device_sync(lib):
    import torch
    if not is_emu(lib):
        torch.cuda.synchronize()


def world_on(lib):
    """the GridWorld wrapper bound to engine library `lib` (None / HIP_LIB: the product class itself).  The product has no
    switch for this: the test suite subclasses it and overrides the class attribute that names the library."""
    if lib is None or os.path.abspath(lib) == os.path.abspath(PRODUCT_LIB):
        return magent_amd.GridWorld
    key = os.path.abspath(lib)
    if key == os.path.abspath(REF_LIB):
        single_threaded_reference()
    if key not in _WORLDS:
        _WORLDS[key] = type("CheckerWorld", (magent_amd.GridWorld,), {"_engine_path": key})
    return _WORLDS[key]


def gridworld(config, lib=None, **kwargs):
    return world_on(lib)(config, **kwargs)


# ---------------------------------------------------------------------------------------------- scenarios
def config_for(game, map_size, **over):
    """built-in game, optionally with agent-type overrides {type_name: {attr: value}} for edge-case scenarios"""
    cfg = _games.make(game, map_size)
    for tname, attrs in over.items():
        cfg.agent_type_dict[tname].update(attrs)
    return cfg


def custom_tri(map_w, map_h):
    """three groups of three different types, every supported rule shape (subject / object receivers, kill, collide),
    in-group attack, kill_supply, a non-square map"""
    cfg = gw.Config()
    cfg.set({"map_width": map_w, "map_height": map_h, "minimap_mode": True, "embedding_size": 4})
    a = cfg.register_agent_type("a", dict(width=1, length=1, hp=6, speed=2, view_range=gw.CircleRange(5), attack_range=gw.CircleRange(1.5),
                                          damage=2, step_recover=0.1, step_reward=-0.01, kill_reward=3, dead_penalty=-0.5, attack_penalty=-0.05))
    b = cfg.register_agent_type("b", dict(width=1, length=1, hp=4, speed=3, view_range=gw.CircleRange(4), attack_range=gw.CircleRange(2),
                                          damage=3, step_recover=0, attack_in_group=1, kill_supply=2.5, kill_reward=1, dead_penalty=-1))
    c = cfg.register_agent_type("c", dict(width=1, length=1, hp=9, speed=1, view_range=gw.CircleRange(2), attack_range=gw.CircleRange(1),
                                          damage=1.5, step_recover=-0.3, kill_supply=4, attack_penalty=-0.2, step_reward=0.25))
    ga, gb, gc = cfg.add_group(a), cfg.add_group(b), cfg.add_group(c)
    sa, sb, sc_ = gw.AgentSymbol(ga, "any"), gw.AgentSymbol(gb, "any"), gw.AgentSymbol(gc, "any")
    cfg.add_reward_rule(gw.Event(sa, "attack", sb), receiver=[sa, sb], value=[0.3, -0.7])
    cfg.add_reward_rule(gw.Event(sb, "kill", sc_), receiver=sb, value=2.25)
    cfg.add_reward_rule(gw.Event(sc_, "collide", sa), receiver=[sa], value=[-0.125])
    cfg.add_reward_rule(gw.Event(sb, "attack", sb), receiver=sb, value=0.0625)      # same symbol twice: never fires
    sb2 = gw.AgentSymbol(gb, "any")
    cfg.add_reward_rule(gw.Event(sb, "attack", sb2), receiver=sb, value=0.03125)    # in-group attack, subject paid
    cfg.add_reward_rule(gw.Event(sb2, "attack", sb), receiver=sb, value=-0.015625)  # in-group attack, object pays
    cfg.add_reward_rule(gw.Event(sc_, "attack", sa), receiver=[sa, sa, sc_], value=[-0.2, 0.05, 0.4])
    return cfg


def custom_chase(map_size):
    """no minimap, no embedding (the pursuit layout with a 1x1 predator): rule rewards land on the object of the event"""
    cfg = gw.Config()
    cfg.set({"map_width": map_size, "map_height": map_size})
    pred = cfg.register_agent_type("predator", dict(width=1, length=1, hp=1, speed=1, view_range=gw.CircleRange(5),
                                                    attack_range=gw.CircleRange(2), attack_penalty=-0.2))
    prey = cfg.register_agent_type("prey", dict(width=1, length=1, hp=1, speed=1.5, view_range=gw.CircleRange(4),
                                                attack_range=gw.CircleRange(0)))
    gp, gq = cfg.add_group(pred), cfg.add_group(prey)
    a, b = gw.AgentSymbol(gp, "any"), gw.AgentSymbol(gq, "any")
    cfg.add_reward_rule(gw.Event(a, "attack", b), receiver=[a, b], value=[1, -1])
    return cfg


def custom_quad(map_size):
    """four groups (the unpacked 8-byte view-cell format; 4 x 8 = 32 attack offsets fill the per-cell hit word)"""
    cfg = gw.Config()
    cfg.set({"map_width": map_size, "map_height": map_size, "minimap_mode": True, "embedding_size": 3})
    t = cfg.register_agent_type("q", dict(width=1, length=1, hp=5, speed=2, view_range=gw.CircleRange(3), attack_range=gw.CircleRange(1.5),
                                          damage=2, step_recover=0.05, step_reward=-0.01, kill_reward=2, dead_penalty=-0.3,
                                          attack_penalty=-0.1))
    gs = [cfg.add_group(t) for _ in range(4)]
    syms = [gw.AgentSymbol(g, "any") for g in gs]
    for i in range(4):
        cfg.add_reward_rule(gw.Event(syms[i], "attack", syms[(i + 1) % 4]), receiver=syms[i], value=0.1 * (i + 1))
    return cfg


def custom_bodies(map_w, map_h):
    """multi-cell bodies of three shapes (3x2, 2x2, 1x1) that attack and block each other; minimap on"""
    cfg = gw.Config()
    cfg.set({"map_width": map_w, "map_height": map_h, "minimap_mode": True, "embedding_size": 5})
    big = cfg.register_agent_type("big", dict(width=3, length=2, hp=8, speed=2, view_range=gw.CircleRange(5), attack_range=gw.CircleRange(2.5),
                                              damage=2, step_recover=0.2, kill_reward=2, dead_penalty=-1, attack_penalty=-0.1))
    mid = cfg.register_agent_type("mid", dict(width=2, length=2, hp=4, speed=1, view_range=gw.CircleRange(4), attack_range=gw.CircleRange(2),
                                              damage=1.5, step_recover=-0.1, kill_supply=1.5, kill_reward=1, attack_in_group=1))
    tiny = cfg.register_agent_type("tiny", dict(width=1, length=1, hp=2, speed=3, view_range=gw.CircleRange(3), attack_range=gw.CircleRange(1),
                                                damage=1, step_reward=0.05, dead_penalty=-2))
    g0, g1, g2 = cfg.add_group(big), cfg.add_group(mid), cfg.add_group(tiny)
    a, b, c = gw.AgentSymbol(g0, "any"), gw.AgentSymbol(g1, "any"), gw.AgentSymbol(g2, "any")
    cfg.add_reward_rule(gw.Event(a, "attack", b), receiver=[a, b], value=[0.5, -0.25])
    cfg.add_reward_rule(gw.Event(b, "kill", c), receiver=b, value=1.5)
    cfg.add_reward_rule(gw.Event(c, "collide", a), receiver=c, value=-0.0625)
    cfg.add_reward_rule(gw.Event(b, "collide", b2 := gw.AgentSymbol(g1, "any")), receiver=b, value=-0.03125)
    return cfg


def custom_trans(map_size):
    """examples/train_trans.py:17-37: ONE group, a type registered without any attack range, a 2:1 map"""
    cfg = gw.Config()
    cfg.set({"map_width": map_size * 2, "map_height": map_size, "minimap_mode": True, "embedding_size": 10})
    agent = cfg.register_agent_type("agent", dict(width=1, length=1, hp=10, speed=1, view_range=gw.CircleRange(6),
                                                  damage=2, step_recover=0.1, step_reward=-1))
    cfg.add_group(agent)
    return cfg


def custom_duo(map_size):
    """Event(a, p, c) & Event(b, p, c) in every supported arrangement: both subjects in one group with different values
    (the per-agent float adds interleave by agent order), the second subject declared first, subjects in two groups,
    the object paid, different predicates for the two subjects, in-group targets"""
    cfg = gw.Config()
    cfg.set({"map_width": map_size, "map_height": map_size, "embedding_size": 3})
    deer = cfg.register_agent_type("deer", dict(width=1, length=1, hp=6, speed=1, view_range=gw.CircleRange(2), attack_range=gw.CircleRange(0),
                                                step_recover=0.2, kill_supply=3, step_reward=0.0625))
    tiger = cfg.register_agent_type("tiger", dict(width=1, length=1, hp=10, speed=1, view_range=gw.CircleRange(4), attack_range=gw.CircleRange(1.5),
                                                  damage=1, step_recover=-0.1, step_reward=-0.03125, attack_penalty=-0.1))
    wolf = cfg.register_agent_type("wolf", dict(width=2, length=1, hp=7, speed=2, view_range=gw.CircleRange(3), attack_range=gw.CircleRange(2),
                                                damage=1.5, attack_in_group=1, kill_reward=1.5))
    gd, gt, gwf = cfg.add_group(deer), cfg.add_group(tiger), cfg.add_group(wolf)
    b0 = gw.AgentSymbol(gt, "any")      # declared before its partner: it is the outer loop of the search
    a, b, c = gw.AgentSymbol(gt, "any"), gw.AgentSymbol(gt, "any"), gw.AgentSymbol(gd, "any")
    w1, w2 = gw.AgentSymbol(gwf, "any"), gw.AgentSymbol(gwf, "any")
    ev = gw.Event
    cfg.add_reward_rule(ev(a, "attack", c) & ev(b, "attack", c), receiver=[a, b], value=[1, 0.3])
    cfg.add_reward_rule(ev(a, "attack", c) & ev(b0, "attack", c), receiver=[a, b0], value=[0.7, -0.15])
    cfg.add_reward_rule(ev(a, "attack", c) & ev(w1, "attack", c), receiver=[w1, a, c], value=[0.45, 0.11, -0.6])
    cfg.add_reward_rule(ev(w1, "kill", c) & ev(a, "attack", c), receiver=[a, w1, a], value=[2.2, 0.9, -0.05])
    cfg.add_reward_rule(ev(w1, "attack", w2) & ev(a, "attack", w2), receiver=[w1, a], value=[0.35, 0.21])
    cfg.add_reward_rule(ev(a, "attack", c) & ev(b, "kill", c), receiver=[b, a], value=[1.3, 0.17])
    cfg.add_reward_rule(ev(w1, "attack", c), receiver=[w1], value=[0.019])
    return cfg


def custom_arrange(map_size, live):
    """examples/train_arrange.py:181-214: goals are agents of a `can_absorb` type; the first mover that bumps into a free goal
    is taken in (it dies, the goal's hp doubles) and is paid by the collide rule.  `live` adds a 2x2 group that attacks goals and movers and bumps into goals
    itself; the goals are observed too (a goal-typed observer leaves taken goals out of its minimap)"""
    cfg = gw.Config()
    cfg.set({"map_width": map_size, "map_height": map_size, "minimap_mode": True, "embedding_size": 12})
    goal = cfg.register_agent_type("goal", {"width": 1, "length": 1, "can_absorb": True})
    agent = cfg.register_agent_type("agent", dict(width=1, length=1, hp=10, speed=2, view_range=gw.CircleRange(6),
                                                  step_recover=-10.0 / 400, step_reward=0))
    g_goal, g_agent = cfg.add_group(goal), cfg.add_group(agent)
    g, a = gw.AgentSymbol(g_goal, "any"), gw.AgentSymbol(g_agent, "any")
    cfg.add_reward_rule(gw.Event(a, "collide", g), receiver=a, value=10)
    if live:
        brute = cfg.register_agent_type("brute", dict(width=2, length=2, hp=6, speed=1, view_range=gw.CircleRange(4),
                                                      attack_range=gw.CircleRange(2), damage=0.75, kill_reward=1, step_reward=-0.01))
        g_brute = cfg.add_group(brute)
        b = gw.AgentSymbol(g_brute, "any")
        cfg.add_reward_rule(gw.Event(b, "collide", g), receiver=[b, g], value=[3, 0.5])
        cfg.add_reward_rule(gw.Event(b, "attack", g), receiver=b, value=0.25)
    return cfg


def custom_rules(map_size):
    """rule expressions beyond Event(a, p, b): die / at / in leaves and and / or / not over them, for searches that iterate a
    single symbol (the partner of a binary event is inferred from the subject's op_obj); one rule ends the game"""
    cfg = gw.Config()
    cfg.set({"map_width": map_size, "map_height": map_size, "minimap_mode": True, "embedding_size": 6})
    t = cfg.register_agent_type("r", dict(width=1, length=1, hp=3, speed=2, view_range=gw.CircleRange(4), attack_range=gw.CircleRange(1.5),
                                          damage=2, step_recover=-0.02, step_reward=-0.01, kill_reward=1, dead_penalty=-0.5, attack_penalty=-0.05))
    big = cfg.register_agent_type("b", dict(width=2, length=2, hp=9, speed=1, view_range=gw.CircleRange(3), attack_range=gw.CircleRange(2),
                                            damage=1.5, attack_in_group=1))
    g0, g1, g2 = cfg.add_group(t), cfg.add_group(t), cfg.add_group(big)
    a, b, c = gw.AgentSymbol(g0, "any"), gw.AgentSymbol(g1, "any"), gw.AgentSymbol(g2, "any")
    b2, c2 = gw.AgentSymbol(g1, "any"), gw.AgentSymbol(g2, "any")
    ev = gw.Event
    half = map_size // 2
    cfg.add_reward_rule(ev(a, "die"), receiver=a, value=-0.7)
    cfg.add_reward_rule(ev(a, "in", ((1, 1), (half, half))) & ~ev(a, "die"), receiver=a, value=0.11)
    cfg.add_reward_rule(ev(a, "attack", b) & ev(b, "attack", a), receiver=[a, b], value=[0.9, -0.3])         # duel
    cfg.add_reward_rule(ev(b2, "kill", c) | ev(b2, "collide", c), receiver=[b2, c, b2], value=[0.4, -0.2, 0.05])
    cfg.add_reward_rule(~ev(c2, "attack", a) & ev(c2, "in", ((half, 0), (map_size, map_size))), receiver=c2, value=0.021)
    cfg.add_reward_rule(ev(b, "at", (half, half)), receiver=b, value=5, terminal=True)
    cfg.add_reward_rule(ev(a, "kill", c) & ev(c, "die"), receiver=[c, a], value=[-1.5, 2.5])
    return cfg


def custom_search(map_size):
    """rule shapes only the reference's recursive search takes (RewardEngine.cc:373-443) -- on the HIP engine they send ALL rules
    of the game to the host evaluation: two iterated symbols (O(N^2) bindings), 'all' symbols as subject and as receiver (group
    reward), a fixed-index symbol (with the reference's Agent::index quirk: 0 until the agent has been through a clear_dead),
    in_a_line, subject and object paid in one group"""
    cfg = gw.Config()
    cfg.set({"map_width": map_size, "map_height": map_size, "minimap_mode": True, "embedding_size": 4})
    t = cfg.register_agent_type("s", dict(width=1, length=1, hp=3, speed=2, view_range=gw.CircleRange(4), attack_range=gw.CircleRange(1.5),
                                          damage=2, step_recover=-0.02, step_reward=-0.01, kill_reward=1, dead_penalty=-0.5, attack_penalty=-0.05,
                                          attack_in_group=1))
    post = cfg.register_agent_type("post", dict(width=1, length=1, hp=2, speed=0, view_range=gw.CircleRange(2), attack_range=gw.CircleRange(0)))
    g0, g1, g2 = cfg.add_group(t), cfg.add_group(t), cfg.add_group(post)
    ev, sym = gw.Event, gw.AgentSymbol
    a, b, c, d = sym(g0, "any"), sym(g1, "any"), sym(g0, "any"), sym(g1, "any")
    cfg.add_reward_rule(ev(a, "attack", b) & ev(c, "attack", d), receiver=[a, d], value=[0.0625, -0.03125])          # two subjects, two objects
    e, f = sym(g0, "any"), sym(g1, "any")
    cfg.add_reward_rule(ev(e, "attack", f) & ev(d, "die"), receiver=[e, d, f], value=[0.5, -0.25, 0.125])          # a binding per (attacker, dead agent)
    all1, all2 = sym(g1, "all"), sym(g2, "all")
    cfg.add_reward_rule(ev(all1, "in", ((0, 0), (map_size, map_size))), receiver=all1, value=0.015625)              # group reward
    first = sym(g0, 0)
    cfg.add_reward_rule(ev(first, "attack", b), receiver=[first, b], value=[1.5, -0.75])                             # a fixed agent
    third = sym(g1, 3)
    cfg.add_reward_rule(ev(a, "attack", third), receiver=[a, third], value=[0.3, -0.7])                              # ... as the object
    cfg.add_reward_rule(ev(all2, "in_a_line"), receiver=[all2], value=[0.2])
    x, y = sym(g0, "any"), sym(g0, "any")
    cfg.add_reward_rule(ev(x, "attack", y), receiver=[x, y], value=[0.11, -0.13])                                    # subject and object in one group
    cfg.add_reward_rule(ev(a, "kill", b) & ev(c, "kill", d), receiver=[a, c], value=[2, 3], terminal=True)
    return cfg


def custom_sector(map_w, map_h):
    """sector ranges (Range.h:104-144): the view is a wedge in front of the agent (a window that does not contain the agent itself,
    wider than high or higher than wide), attacks reach forward only; a 2x2 body among them.  With turn_mode the wedge turns with
    the agent; without it everybody looks north"""
    cfg = gw.Config()
    cfg.set({"map_width": map_w, "map_height": map_h, "minimap_mode": True, "embedding_size": 6})
    scout = cfg.register_agent_type("scout", dict(width=1, length=1, hp=5, speed=2, view_range=gw.SectorRange(7, 100), attack_range=gw.SectorRange(2.5, 120),
                                                  damage=2, step_recover=0.1, step_reward=-0.01, kill_reward=2, dead_penalty=-0.3, attack_penalty=-0.05))
    guard = cfg.register_agent_type("guard", dict(width=2, length=2, hp=9, speed=1, view_range=gw.SectorRange(4, 60), attack_range=gw.CircleRange(2),
                                                  damage=1.5, step_recover=-0.05, kill_supply=1, attack_in_group=1))
    lurker = cfg.register_agent_type("lurker", dict(width=1, length=1, hp=3, speed=1, view_range=gw.CircleRange(3), attack_range=gw.SectorRange(3, 40),
                                                    damage=3, dead_penalty=-1))
    g0, g1, g2 = cfg.add_group(scout), cfg.add_group(guard), cfg.add_group(lurker)
    a, b, c = gw.AgentSymbol(g0, "any"), gw.AgentSymbol(g1, "any"), gw.AgentSymbol(g2, "any")
    cfg.add_reward_rule(gw.Event(a, "attack", b), receiver=[a, b], value=[0.25, -0.125])
    cfg.add_reward_rule(gw.Event(c, "kill", a), receiver=c, value=1.5)
    return cfg


CUSTOM = {"sector": custom_sector, "search": custom_search, "rules": custom_rules, "arrange": custom_arrange, "duo": custom_duo, "trans": custom_trans, "tri": custom_tri, "chase": custom_chase, "quad": custom_quad, "bodies": custom_bodies}


class Scenario(object):
    """a reproducible episode: game + placement recipe + random action stream

    game     : built-in game name, or ("custom-name", args...) for one of the CUSTOM configs
    events   : {step: [("add", group, method, kw) | ("walls", method, kw) | ("reset", placements)]} applied before
               that step's observations -- mid-episode placement and a second episode on the same engine (the RNG
               stream continues across reset, GridWorld.cc:72-118)
    observed : (run_cycle / run_cycle_batch only) the groups that are given view / feature buffers: None (all), a list, or a callable
               step -> list.  A group left out is not observed by the checker's leg either and has no view%d / feat%d key
    rewarded : likewise for the reward buffers (reward%d)
    probe    : steps BEFORE whose cycle both legs observe EVERY non-empty group through the ordinary calls (probe_view%d, probe_feat%d:
               the last_reward / last_action columns and the hp cells of a group that was left out), and read every group's reward
               behind the cycle (probe_reward%d); when any is given, the same is done once more behind the last cycle"""

    def __init__(self, name, game, map_size, seed=12345, place=(), steps=10, action_seed=0, walls=0,
                 acting=None, over=None, clear_every=1, obs_every=1, events=None, settings=None, engine=True, still=(),
                 observed=None, rewarded=None, probe=()):
        self.observed, self.rewarded, self.probe = observed, rewarded, tuple(probe)
        self.name, self.game, self.map_size, self.seed = name, game, map_size, seed
        self.engine = engine                # False: the engine refuses this game (turn_mode); the oracle is pinned on it all the same
        self.settings = settings or {}      # extra GridWorld settings (food_mode, ...) and, for custom games, type overrides
        self.place, self.steps, self.action_seed, self.walls = list(place), steps, action_seed, walls
        self.acting, self.over, self.clear_every, self.obs_every = acting, over or {}, clear_every, obs_every
        self.events = events or {}
        self.still = tuple(still)           # groups that are given actions but told to stand still: every move drawn becomes the zero move

    def draw(self, rs, env, g, h, n):
        """this step's actions of group g: uniform over its action space (one draw from `rs`, whatever `still` says)"""
        a = rs.randint(env.get_action_space(h)[0], size=n).astype(np.int32)
        if g in self.still:
            n_move = env.get_view2attack(h)[0] - (2 if self.settings.get("turn_mode") else 0)
            a[:] = n_move // 2              # (the move tables are circle ranges: the centre, (0, 0), is the middle entry)
        return a

    def groups_at(self, which, step, n_group):
        """the groups that `which` (self.observed or self.rewarded) names at `step`"""
        sel = which(step) if callable(which) else which
        return list(range(n_group)) if sel is None else list(sel)

    def probe_before(self, env, handles, step, rec):
        """a probe step: every non-empty group observed through the reference ABI, whatever `observed` says"""
        if step not in self.probe:
            return
        for g, h in enumerate(handles):
            if env.get_num(h) > 0:
                v, f = env.get_observation(h)
                rec["probe_view%d" % g], rec["probe_feat%d" % g] = v.copy(), f.copy()

    def probe_after(self, env, handles, step, rec):
        """behind a probe step's cycle every group's reward is read through the reference ABI (behind clear_dead: what Agent::init_reward and
        Group::init_reward left); behind the last cycle every non-empty group is observed once more"""
        if step in self.probe:
            for g, h in enumerate(handles):
                rec["probe_reward%d" % g] = np.array(env.get_reward(h), dtype=np.float32)
        if self.probe and step == self.steps - 1:
            for g, h in enumerate(handles):
                if env.get_num(h) > 0:
                    v, f = env.get_observation(h)
                    rec["end_view%d" % g], rec["end_feat%d" % g] = v.copy(), f.copy()

    def config(self):
        if callable(self.game):
            return self.game()
        if isinstance(self.game, tuple):
            cfg = CUSTOM[self.game[0]](*self.game[1:])
            for tname, attrs in self.over.items():
                cfg.agent_type_dict[tname].update(attrs)
        else:
            cfg = config_for(self.game, self.map_size, **self.over)
        if self.settings:
            cfg.set(dict(self.settings))
        return cfg

    def populate(self, env, place, walls):
        if walls:
            env.add_walls(method="random", n=walls)
        handles = env.get_handles()
        for g, method, kw in place:
            env.add_agents(handles[g], method, **kw)

    def build(self, lib):
        env = gridworld(self.config(), lib=lib)
        env.set_seed(self.seed)
        env.reset()
        self.populate(env, self.place, self.walls)
        return env, env.get_handles()

    def apply_events(self, env, step):
        for ev in self.events.get(step, ()):
            if ev[0] == "add":
                env.add_agents(env.get_handles()[ev[1]], ev[2], **ev[3])
            elif ev[0] == "walls":
                env.add_walls(method=ev[1], **ev[2])
            elif ev[0] == "goal":
                env.set_goal(env.get_handles()[ev[1]], "random")
            elif ev[0] == "reset":
                env.reset()
                self.populate(env, ev[1], 0)


def run(sc, lib, record=None, device_io=False, env_out=None):
    """Play scenario `sc` on library `lib`; returns list (one dict per step) of every observable output.

    Order of calls per step follows examples/train_battle.py:61-109: get_observation + set_action per group,
    step, get_reward / get_alive / get_pos / get_num per group, clear_dead.

    device_io (HIP engine only): the call sequence bench.py times -- env_get_observation_device into caller-owned torch
    tensors allocated ONCE for the initial population, env_set_action_device from a device tensor, env_get_reward_device --
    instead of the host-buffer reference ABI; the arrays are brought to the host only to be recorded."""
    env, handles = sc.build(lib)
    if env_out is not None:
        env_out.append(env)        # (the caller wants to look at the engine afterwards: engine_stats)
    rs = np.random.RandomState(sc.action_seed)
    twice = np.random.RandomState(sc.action_seed ^ 0x7A1CE) if os.environ.get("FUZZ_TWICE", "0") == "1" else None
    acting = sc.acting if sc.acting is not None else list(range(len(handles)))
    if device_io:
        import torch
        dev = torch_device(env, lib)
        cap = [env.get_num(h) for h in handles]
        d_view = [torch.empty((cap[g],) + env.get_view_space(h), device=dev) for g, h in enumerate(handles)]
        d_feat = [torch.empty((cap[g],) + env.get_feature_space(h), device=dev) for g, h in enumerate(handles)]
        d_rew = [torch.empty(cap[g], device=dev) for g in range(len(handles))]
    out = []
    for step in range(sc.steps):
        rec = {}
        sc.apply_events(env, step)
        for g, h in enumerate(handles):
            n = env.get_num(h)
            if device_io:
                assert n <= cap[g], "device_io: the population grew beyond the caller's buffers"
                if step % sc.obs_every == 0 and n > 0:
                    env.get_observation_device(h, d_view[g], d_feat[g])
                    env.sync()
                    rec["view%d" % g], rec["feat%d" % g] = d_view[g][:n].cpu().numpy(), d_feat[g][:n].cpu().numpy()
                rec["id%d" % g] = env.get_agent_id(h)
                if g in acting:
                    a = torch.from_numpy(sc.draw(rs, env, g, h, n)).to(dev)
                    device_sync(lib)
                    env.set_action_device(h, a)
                continue
            if step % sc.obs_every == 0 and n > 0:
                view, feat = env.get_observation(h)
                rec["view%d" % g], rec["feat%d" % g] = view.copy(), feat.copy()
            rec["id%d" % g] = env.get_agent_id(h)
            if g in acting:
                env.set_action(h, sc.draw(rs, env, g, h, n))
        if twice is not None and not device_io:      # FUZZ_TWICE=1: some groups are given actions again before the step (GridWorld.cc:403-454 appends)
            for g in [g for g in acting if twice.rand() < 0.4]:
                env.set_action(handles[g], twice.randint(env.get_action_space(handles[g])[0], size=env.get_num(handles[g])).astype(np.int32))
        rec["done"] = np.array([env.step()], dtype=np.int32)
        for g, h in enumerate(handles):
            if device_io:
                env.get_reward_device(h, d_rew[g])
                env.sync()
                rec["reward%d" % g] = d_rew[g][:env.get_num(h)].cpu().numpy()
            else:
                rec["reward%d" % g] = env.get_reward(h)
            rec["alive%d" % g] = env.get_alive(h).astype(np.uint8)
            rec["pos%d" % g] = env.get_pos(h)
            rec["num%d" % g] = np.array([env.get_num(h)], dtype=np.int32)
        if step % 7 == 3:
            rec["global_minimap"] = env.get_global_minimap(5, 6).copy()
        if (step + 1) % sc.clear_every == 0:
            env.clear_dead()
        out.append(rec)
        if record is not None:
            record(step, rec)
        if all(env.get_num(h) == 0 for h in handles) and not any(k > step for k in sc.events):
            break
    return out


def mean_info_trace(sc, lib, steps=6):
    """get_info("mean_info") (GridWorld.cc:765-786, "deprecated" there) of every acting, non-empty group of scenario `sc` at three points of
    every step: between set_action and step (Agent::get_action already shows the new action), behind the step (the dead still counted), behind
    clear_dead.  Only groups that have been given actions are asked: the reference counts an agent that never acted one past the end of a
    heap array."""
    env, handles = sc.build(lib)
    rs = np.random.RandomState(sc.action_seed)
    acting = sc.acting if sc.acting is not None else list(range(len(handles)))
    out = []
    for step in range(min(steps, sc.steps)):
        sc.apply_events(env, step)
        asked = []
        for g, h in enumerate(handles):
            n = env.get_num(h)
            if g in acting:
                env.set_action(h, sc.draw(rs, env, g, h, n))
                if n > 0:
                    asked.append(h)
        out += [env.get_mean_info(h).copy() for h in asked]
        env.step()
        out += [env.get_mean_info(h).copy() for h in asked]
        env.clear_dead()
        out += [env.get_mean_info(h).copy() for h in asked if env.get_num(h) > 0]
    return out


def run_cycle(sc, lib, fused, preset=False, reduce=None):
    """Play `sc` one environment CYCLE at a time (observe + set_action per group, step, rewards, clear_dead) and record what a
    caller of magent_amd.EnvBatch.cycle can see: observations, ids, rewards, done, and the state AFTER clear_dead.

    fused=True : the HIP engine through env_cycle_many (EnvBatch.cycle: two launches per cycle for small worlds), device buffers
    fused=False: any library, the same calls one after the other through the reference API (the CPU checkers take this leg)
    reduce     : what is kept of a step's record (hash_rec for worlds whose trajectories do not fit in memory)"""
    assert sc.clear_every == 1
    env, handles = sc.build(lib)
    rs = np.random.RandomState(sc.action_seed)
    acting = sc.acting if sc.acting is not None else list(range(len(handles)))
    if fused:
        import torch
        dev = torch_device(env, lib)
        batch = magent_amd.EnvBatch([env], n_threads=1)
        batch.order_streams = not is_emu(lib)
    out = []
    for step in range(sc.steps):
        rec = {}
        sc.apply_events(env, step)
        nums = [env.get_num(h) for h in handles]
        acts = [sc.draw(rs, env, g, h, nums[g]) if g in acting else None for g, h in enumerate(handles)]
        seen, paid = sc.groups_at(sc.observed, step, len(handles)), sc.groups_at(sc.rewarded, step, len(handles))
        observe = [step % sc.obs_every == 0 and nums[g] > 0 and g in seen for g in range(len(handles))]
        sc.probe_before(env, handles, step, rec)
        for g, h in enumerate(handles):
            rec["id%d" % g] = env.get_agent_id(h)
        if fused:
            views = [torch.empty((nums[g],) + env.get_view_space(h), device=dev) if observe[g] else None for g, h in enumerate(handles)]
            feats = [torch.empty((nums[g],) + env.get_feature_space(h), device=dev) if observe[g] else None for g, h in enumerate(handles)]
            d_acts = [torch.from_numpy(a).to(dev) if a is not None else None for a in acts]
            rews = [torch.empty(nums[g], device=dev) if g in paid else None for g in range(len(handles))]
            device_sync(lib)
            done = batch.cycle([views], [feats], [d_acts], [rews])[0]
            env.sync()
            for g in range(len(handles)):
                if observe[g]:
                    rec["view%d" % g], rec["feat%d" % g] = views[g].cpu().numpy(), feats[g].cpu().numpy()
                if g in paid:
                    rec["reward%d" % g] = rews[g].cpu().numpy()
        else:
            assert not (preset and fused)
            for g, h in enumerate(handles):       # (preset: every set_action ahead of every observation)
                if preset and acts[g] is not None:
                    env.set_action(h, acts[g])
            for g, h in enumerate(handles):
                if observe[g]:
                    v, f = env.get_observation(h)
                    rec["view%d" % g], rec["feat%d" % g] = v.copy(), f.copy()
                if not preset and acts[g] is not None:
                    env.set_action(h, acts[g])
            done = env.step()
            for g, h in enumerate(handles):
                if g in paid:
                    rec["reward%d" % g] = env.get_reward(h)
            env.clear_dead()
        rec["done"] = np.array([done], dtype=np.int32)
        for g, h in enumerate(handles):       # the state after clear_dead
            rec["num%d" % g] = np.array([env.get_num(h)], dtype=np.int32)
            rec["pos%d" % g] = env.get_pos(h)
            rec["alive%d" % g] = env.get_alive(h).astype(np.uint8)
            rec["ids_after%d" % g] = env.get_agent_id(h)
        sc.probe_after(env, handles, step, rec)
        out.append(reduce(rec) if reduce else rec)
        if all(env.get_num(h) == 0 for h in handles) and not any(k > step for k in sc.events):
            break
    return out


def run_cycle_batch(scs, lib, preset=False, envs_out=None, counters_out=None, reduce=None):
    """run_cycle(fused=True) for SEVERAL environments of one configuration at once: a single magent_amd.EnvBatch, so that for
    small worlds all of them share one pair of launches per cycle (k_render_batch + k_step_solo_batch).  Returns one trajectory
    per scenario; an environment whose groups are all empty keeps cycling with the others (its trajectory stops there, as
    run_cycle's does).
    preset: the actions are handed over by env_set_action_device BEFORE the call and the cycle is given none (the NULL entries
    include/magent_runtime_api.h documents): the observations then show the new last_action, as the reference's do when
    set_action comes first (GridWorld.cc:386-396) -- the checker's leg is run_cycle(..., preset=True).
    counters_out: a list that receives, per cycle, every environment's count of cycles through the batched pipeline so far
    (pipeline_stats()[6]) -- which environment was in the pipeline in which cycle (expected_pipe_cycles)."""
    import torch
    built = [sc.build(lib) for sc in scs]
    envs, handles = [b[0] for b in built], [b[1] for b in built]
    if envs_out is not None:
        envs_out.extend(envs)
    dev = torch_device(envs[0], lib)
    batch = magent_amd.EnvBatch(envs, n_threads=1)
    batch.order_streams = not is_emu(lib)
    rss = [np.random.RandomState(sc.action_seed) for sc in scs]
    out, live = [[] for _ in scs], [True] * len(scs)
    for step in range(max(sc.steps for sc in scs)):
        recs, views, feats, d_acts, rews, observes = [], [], [], [], [], []
        for k, (sc, env, hs) in enumerate(zip(scs, envs, handles)):
            assert sc.clear_every == 1
            acting = sc.acting if sc.acting is not None else list(range(len(hs)))
            rec = {}
            sc.apply_events(env, step)
            nums = [env.get_num(h) for h in hs]
            acts = [rss[k].randint(env.get_action_space(h)[0], size=nums[g]).astype(np.int32) if g in acting else None for g, h in enumerate(hs)]
            seen, paid = sc.groups_at(sc.observed, step, len(hs)), sc.groups_at(sc.rewarded, step, len(hs))
            observe = [step % sc.obs_every == 0 and nums[g] > 0 and g in seen for g in range(len(hs))]
            if live[k] and step < sc.steps:
                sc.probe_before(env, hs, step, rec)
            for g, h in enumerate(hs):
                rec["id%d" % g] = env.get_agent_id(h)
            views.append([torch.empty((nums[g],) + env.get_view_space(h), device=dev) if observe[g] else None for g, h in enumerate(hs)])
            feats.append([torch.empty((nums[g],) + env.get_feature_space(h), device=dev) if observe[g] else None for g, h in enumerate(hs)])
            d_acts.append([torch.from_numpy(a).to(dev) if a is not None else None for a in acts])
            rews.append([torch.empty(nums[g], device=dev) if g in paid else None for g in range(len(hs))])
            recs.append(rec); observes.append(observe)
        device_sync(lib)
        if preset:
            for env, hs, per_env in zip(envs, handles, d_acts):
                for h, a in zip(hs, per_env):
                    if a is not None:
                        env.set_action_device(h, a)
            dones = batch.cycle(views, feats, None, rews)
        else:
            dones = batch.cycle(views, feats, d_acts, rews)
        if counters_out is not None:
            counters_out.append([env.pipeline_stats()[6] for env in envs])
        for k, (sc, env, hs) in enumerate(zip(scs, envs, handles)):
            env.sync()
            rec = recs[k]
            for g in range(len(hs)):
                if observes[k][g]:
                    rec["view%d" % g], rec["feat%d" % g] = views[k][g].cpu().numpy(), feats[k][g].cpu().numpy()
                if rews[k][g] is not None:
                    rec["reward%d" % g] = rews[k][g].cpu().numpy()
            rec["done"] = np.array([dones[k]], dtype=np.int32)
            for g, h in enumerate(hs):
                rec["num%d" % g] = np.array([env.get_num(h)], dtype=np.int32)
                rec["pos%d" % g] = env.get_pos(h)
                rec["alive%d" % g] = env.get_alive(h).astype(np.uint8)
                rec["ids_after%d" % g] = env.get_agent_id(h)
            if live[k] and step < sc.steps:
                sc.probe_after(env, hs, step, rec)
                out[k].append(reduce(rec) if reduce else rec)
                if all(env.get_num(h) == 0 for h in hs) and not any(e > step for e in sc.events):
                    live[k] = False
    return out


def expected_pipe_cycles(scs, trajs, tune=""):
    """per cycle, which environments of ONE EnvBatch the engine sends through the batched pipeline (Env::cycle_many / Env::pipe_eligible restated
    for the plain games of pipe_partial_scenarios; `trajs`: the checker's trajectories, whose id%d arrays give the sizes at the start of every
    cycle): a plain world of which no two observed, non-empty groups look through different windows under minimap_mode; from `batch_pipe_min`
    (1537) agents on -- at every size when MAGENT_TUNE sets batch_pipe_min=1 or fixes attack_pairs (the one-launch step is off then); and only
    when at least two environments of the call qualify.  Returns the running counts, [cycle][environment], as run_cycle_batch's counters_out."""
    forced = "batch_pipe_min=1" in tune or "attack_pairs=" in tune
    windows = []
    for sc in scs:
        cfg = sc.config()
        ranges = [cfg.agent_type_dict[cfg.groups[g]]["view_range"] for g in range(len(cfg.groups))]
        windows.append((bool(cfg.config_dict.get("minimap_mode")), [(r.radius, r.angle) for r in ranges]))
    counts, out = [0] * len(scs), []
    for step in range(max(sc.steps for sc in scs)):
        ok = []
        for sc, traj, (minimap, win) in zip(scs, trajs, windows):
            assert step < len(traj), "expected_pipe_cycles: every environment of the batch plays every cycle"
            nums = [len(traj[step]["id%d" % g]) for g in range(len(win))]
            seen = [g for g in sc.groups_at(sc.observed, step, len(win)) if nums[g] > 0 and step % sc.obs_every == 0]
            ok.append(sum(nums) > 0 and (forced or sum(nums) >= 1537) and not (minimap and len(set(win[g] for g in seen)) > 1))
        for k in range(len(scs)):
            counts[k] += ok[k] and sum(ok) >= 2
        out.append(list(counts))
    return out


def check_pipe_partial(lib, what):
    """pipe_partial_scenarios in ONE EnvBatch on engine library `lib`, every environment against the oracle driven alone through the reference
    call sequence; which environment went through the batched pipeline in which cycle, from the engine's own counter, against
    expected_pipe_cycles under this process's MAGENT_TUNE.  Returns the final counts."""
    tune = os.environ.get("MAGENT_TUNE", "")
    scs = pipe_partial_scenarios()
    want = [run_cycle(sc, ensure_oracle(), fused=False) for sc in scs]
    for sc, w in zip(scs, want):
        if sc.name.startswith("gather_bench"):   # food is eaten and the group that nobody looks at compacted in (far more than) half of the steps
            sizes = [len(w[0]["id0"])] + [int(r["num0"][0]) for r in w]
            assert len(w) == sc.steps >= 12 and sum(b < a for a, b in zip(sizes, sizes[1:])) * 2 >= sc.steps, (sc.name, sizes)
        assert not sc.probe or (any(k.startswith("probe_view") for k in w[sc.probe[0]]) and any(k.startswith("end_view") for k in w[-1])), sc.name
    expect = expected_pipe_cycles(scs, want, tune)
    # (the restatement itself, pinned: with the defaults the eight partial worlds play every cycle in the pipeline but for the two that
    # gather_changing goes alone; pipe_a falls below 1537 agents in its last two; the two-launch world never gets there)
    forced = "batch_pipe_min=1" in tune or "attack_pairs=" in tune
    assert expect[-1] == [12, 12, 12, 12, 12, 12, 10, 12, 12 if forced else 10, 12 if forced else 0], expect[-1]
    assert [c[6] for c in expect[3:7]] == [4, 4, 4, 5], expect      # (the counter stands still in cycles 4 and 5)
    seen, counters = [], []
    got = run_cycle_batch(scs, lib, envs_out=seen, counters_out=counters)
    for sc, w, g in zip(scs, want, got):
        assert_same(w, g, "%s (%s)" % (sc.name, what))
    assert counters == expect, (what, counters, expect)
    return counters[-1]


def check_cycle_partial(lib, what):
    """cycle_partial_scenarios through run_cycle(fused=True) one by one and as batches of three (the two-launch cycle: k_render_batch +
    k_step_solo_batch), every environment against the oracle driven alone through the reference call sequence"""
    scs = cycle_partial_scenarios()
    want = [run_cycle(sc, ensure_oracle(), fused=False) for sc in scs]
    for sc, w in zip(scs, want):
        assert_same(w, run_cycle(sc, lib, fused=True), "%s (alone, %s)" % (sc.name, what))
    for pick in ([0, 1, 2], [3, 2, 1]):
        for k, g in zip(pick, run_cycle_batch([scs[k] for k in pick], lib)):
            assert_same(want[k], g, "%s (batch of three, %s)" % (scs[k].name, what))


def handover_scenarios():
    """two plain battle worlds, 60 x 60 with 2 x 830 agents at hp 4 / damage 3 (kills in every step), whose population crosses the limits
    between the engine's step drivers several times in 40 steps (HANDOVER_PLAN; the sizes at every step come from the oracle and are pinned
    by check_driver_handovers): reinforcements at steps 12 and 30"""
    rnd = lambda g, n: (g, "random", {"n": n})
    more = lambda a, b: [("add", 0, "random", {"n": a}), ("add", 1, "random", {"n": b})]
    return [Scenario("handover_%d" % k, "battle", 60, seed=6100 + 31 * k, place=[rnd(0, 830), rnd(1, 830)], steps=40, action_seed=400 + k,
                     over={"small": {"hp": 4, "damage": 3}}, events={12: more(600, 600), 30: more(700, 700)}) for k in range(2)]


# one environment's life across the drivers (play_handovers).  Steps 0 .. batch_from - 1 go call by call (Env::step_begin / step_end):
#   0-4    above 1536 agents: the single-environment pipeline of plain games; clear_dead skipped behind step 1: step 2 meets stale events
#          and does not fuse the rules
#   5-11   deaths have brought the world below 1537: the one-launch step; clear_dead skipped behind step 7
#   12     reinforcements: above 1536 again; group 0 is given actions twice in steps 13 and 16 -- the literal loop, at a size at which no
#          one-launch step exists -- and clear_dead is skipped behind step 14
#   23-39  deaths have brought it below 1537 again: env_cycle_many over the two worlds -- below batch_pipe_min (1537) the two-launch cycle,
#          from the reinforcements of step 30 on the batched pipeline
HANDOVER_PLAN = {"skip_clear": (1, 7, 14), "twice": (13, 16), "batch_from": 23}


def play_handovers(lib, fused, counters_out=None):
    """handover_scenarios by HANDOVER_PLAN on engine library `lib`; returns one trajectory per world.  Up to `batch_from` every world makes
    the reference's calls one after the other (as run does); from there on `fused` sends both through ONE magent_amd.EnvBatch.cycle per step
    (env_cycle_many), while a checker (fused=False) goes on alone through the reference call sequence (as run_cycle does).
    counters_out receives, per step and world, (agents at the start of the step, engine_stats(), pipeline_stats()) read behind the step."""
    scs, plan = handover_scenarios(), HANDOVER_PLAN
    built = [sc.build(lib) for sc in scs]
    envs, handles = [b[0] for b in built], [b[1] for b in built]
    rss = [np.random.RandomState(sc.action_seed) for sc in scs]
    again = [np.random.RandomState(sc.action_seed + 1000) for sc in scs]
    if fused:
        import torch
        dev = torch_device(envs[0], lib)
        batch = magent_amd.EnvBatch(envs, n_threads=1)
        batch.order_streams = not is_emu(lib)
    out = [[] for _ in scs]
    for step in range(scs[0].steps):
        recs, nums = [{} for _ in scs], []
        for sc, env in zip(scs, envs):
            sc.apply_events(env, step)
        nums = [[env.get_num(h) for h in hs] for env, hs in zip(envs, handles)]
        together = fused and step >= plan["batch_from"]
        if together:
            views = [[torch.empty((n,) + env.get_view_space(h), device=dev) for n, h in zip(ns, hs)] for env, hs, ns in zip(envs, handles, nums)]
            feats = [[torch.empty((n,) + env.get_feature_space(h), device=dev) for n, h in zip(ns, hs)] for env, hs, ns in zip(envs, handles, nums)]
            rews = [[torch.empty(n, device=dev) for n in ns] for ns in nums]
            acts = [[torch.from_numpy(sc.draw(rs, env, g, h, ns[g])).to(dev) for g, h in enumerate(hs)] for sc, rs, env, hs, ns in zip(scs, rss, envs, handles, nums)]
            for env, hs, rec in zip(envs, handles, recs):
                for g, h in enumerate(hs):
                    rec["id%d" % g] = env.get_agent_id(h)
            device_sync(lib)
            dones = batch.cycle(views, feats, acts, rews)
            for k, (env, rec) in enumerate(zip(envs, recs)):
                env.sync()
                for g in range(len(handles[k])):
                    rec["view%d" % g], rec["feat%d" % g], rec["reward%d" % g] = views[k][g].cpu().numpy(), feats[k][g].cpu().numpy(), rews[k][g].cpu().numpy()
                rec["done"] = np.array([dones[k]], dtype=np.int32)
        for k, (sc, env, hs, rec) in enumerate(zip(scs, envs, handles, recs)):
            if not together:
                for g, h in enumerate(hs):
                    if nums[k][g] > 0:
                        view, feat = env.get_observation(h)
                        rec["view%d" % g], rec["feat%d" % g] = view.copy(), feat.copy()
                    rec["id%d" % g] = env.get_agent_id(h)
                    env.set_action(h, sc.draw(rss[k], env, g, h, nums[k][g]))
                if step in plan["twice"]:       # (GridWorld.cc:403-454 appends: every agent of the group acts once per call)
                    env.set_action(hs[0], sc.draw(again[k], env, 0, hs[0], nums[k][0]))
                rec["done"] = np.array([env.step()], dtype=np.int32)
                for g, h in enumerate(hs):
                    rec["reward%d" % g] = env.get_reward(h)
                    if step < plan["batch_from"]:       # (the state behind the step, the dead still listed)
                        rec["alive_before%d" % g], rec["pos_before%d" % g] = env.get_alive(h).astype(np.uint8), env.get_pos(h)
                if step not in plan["skip_clear"]:
                    env.clear_dead()
            for g, h in enumerate(hs):              # the state behind clear_dead
                rec["num%d" % g] = np.array([env.get_num(h)], dtype=np.int32)
                rec["pos%d" % g], rec["alive%d" % g], rec["ids_after%d" % g] = env.get_pos(h), env.get_alive(h).astype(np.uint8), env.get_agent_id(h)
            out[k].append(rec)
        if counters_out is not None:
            counters_out.append([(sum(ns), env.engine_stats(), env.pipeline_stats()) for ns, env in zip(nums, envs)])
    return out


def check_driver_handovers(lib, what):
    """play_handovers on engine library `lib` against the oracle driven alone, bit for bit -- and, from the engine's own counters (deltas of
    pipeline_stats()[0], steps of the plain pipeline, and [6], cycles through the batched pipeline, step by step), which driver every step of
    every world took: each driver must have run.  No counter tells the one-launch step from the literal loop: a step outside the plain
    pipeline with a group given actions twice is the literal loop (Env::set_action_device), and steps 13 and 16 are such steps above 1536
    agents, where no one-launch form exists; the others are the one-workgroup kernel (k_step_solo alone, the two-launch cycle in a batch).
    MAGENT_TUNE attack_pairs=N fixes the optimistic rounds and thereby switches every one-workgroup form off (Env::solo_ok): under it those
    steps go through the pipeline too and every such step is finished by the host, which is asserted instead."""
    plan, fixed = HANDOVER_PLAN, "attack_pairs=" in os.environ.get("MAGENT_TUNE", "")
    want = play_handovers(ensure_oracle(), fused=False)
    for w in want:      # the plan's sizes, pinned on the oracle: above / below the limit of 1536 agents where the plan says so
        sizes = [sum(len(r["id%d" % g]) for g in range(2)) for r in w]
        assert len(w) == 40 and all(s > 1536 for s in sizes[0:5] + sizes[12:22] + sizes[30:40]) and all(s <= 1536 for s in sizes[5:12] + sizes[23:30]), sizes
    counters = []
    got = play_handovers(lib, fused=True, counters_out=counters)
    for k, (w, g) in enumerate(zip(want, got)):
        assert_same(w, g, "handover_%d (%s)" % (k, what))
    for k in range(2):
        took, plain, piped = [], 0, 0
        for step, per_env in enumerate(counters):
            total, _, ps = per_env[k]
            d_plain, d_pipe = ps[0] - plain, ps[6] - piped
            plain, piped = ps[0], ps[6]
            assert d_plain in (0, 1) and d_pipe in (0, d_plain), (k, step, ps)
            batch = step >= plan["batch_from"]
            took.append("batched pipeline" if d_pipe else "pipeline" if d_plain else "literal loop" if step in plan["twice"] else
                        "two-launch cycle" if batch else "one-launch step")
            assert (d_plain == 1) == (step not in plan["twice"] and (total > 1536 or fixed)), (k, step, total, took)
            assert d_pipe == (1 if batch and (total > 1536 or fixed) and (counters[step][1 - k][0] > 1536 or fixed) else 0), (k, step, total, took)
        # behind a skipped clear_dead a step of the pipeline (rules not fused: stale events) and one of the one-launch step
        assert took[2] == "pipeline" and took[15] == "pipeline" and took[8] == ("pipeline" if fixed else "one-launch step"), took
        drivers = {"pipeline", "literal loop", "batched pipeline"} | (set() if fixed else {"one-launch step", "two-launch cycle"})
        assert set(took) == drivers, (k, took)
        es, ps = counters[-1][k][1], counters[-1][k][2]
        if fixed and "attack_pairs=0" in os.environ["MAGENT_TUNE"]:
            assert es[4] == ps[0] and es[5] == 0, (es, ps)       # the host finished every step of the pipeline
        # the claim words are refilled for the first step of the pipeline and for the first one behind each literal loop (it leaves the scratch
        # dirty), not behind one-workgroup steps (they keep it clean); no window of 63 epochs ends in under 63 such steps
        assert ps[0] < 63 and ps[3] == 3, ps
    return [c[2] for c in counters[-1]]


def hash_rec(rec):
    """a step's record reduced to {key: xxh3-128 hex digest} as run_hashed does (the same digests as tests/golden/digests_fullsize.json)"""
    import xxhash
    return {k: xxhash.xxh3_128(np.ascontiguousarray(v).reshape(-1).view(np.uint8)).hexdigest() for k, v in rec.items()}


def fullsize_partial_batch():
    """bench.py's `extra.gather_500_100k` line at its size, in ONE EnvBatch with a battle world: (A) fullsize_scenarios()["c4_gather500"]
    itself -- gather 500 x 500, 20,000 food + 100,000 agents, its seed and action seed -- with the food never observed, never acting and
    without a reward buffer; (B) the same with other seeds; (C) the first 8 steps of "c2_battle200" (2 x 2000, everybody observed).  With
    groups left out run_cycle makes the reference's calls in run's order but for the left-out ones, so the arrays of A and C that mean the
    same in both drivers (FULLSIZE_PARTIAL_KEYS) equal the compiled reference's committed digests of those scenarios."""
    import copy
    full = fullsize_scenarios()
    a, c = copy.deepcopy(full["c4_gather500"]), copy.deepcopy(full["c2_battle200"])
    a.observed, a.rewarded, a.probe, c.steps = [1], [1], (4,), 8
    b = copy.deepcopy(a)
    b.name, b.seed, b.action_seed = "c4_gather500_other_seeds", 777, 9
    assert a.steps == b.steps == c.steps == 8 and a.acting == [1]
    return [a, b, c]


# (num / pos / alive are recorded before clear_dead by run and behind it by run_cycle: those are compared with the oracle only)
FULLSIZE_PARTIAL_KEYS = {"c4_gather500": ["done", "feat1", "id0", "id1", "reward1", "view1"],
                         "c2_battle200": ["done", "feat0", "feat1", "id0", "id1", "reward0", "reward1", "view0", "view1"]}


def check_fullsize_partial(lib, want, gold):
    """fullsize_partial_batch on engine library `lib`, hashed step by step: every key of all three worlds against `want` (the oracle driven
    alone: [run_cycle(sc, oracle, fused=False, reduce=hash_rec)]), FULLSIZE_PARTIAL_KEYS of A and C against `gold` (the compiled reference's
    digests); all three worlds in the batched pipeline in every cycle.  Returns the engines' render kernels (engine_stats()[6])."""
    scs = fullsize_partial_batch()
    seen, counters = [], []
    got = run_cycle_batch(scs, lib, envs_out=seen, counters_out=counters, reduce=hash_rec)
    for sc, w, g in zip(scs, want, got):
        assert_same_hashed(w, g, sc.name + " vs the oracle driven alone")
        if sc.name in FULLSIZE_PARTIAL_KEYS:
            assert len(g) == 8
            for s, rec in enumerate(g):
                for k in FULLSIZE_PARTIAL_KEYS[sc.name]:
                    assert k in rec, "%s step %d: %s was not recorded" % (sc.name, s, k)
                    assert rec[k] == gold[sc.name][s][k], "%s step %d: %s differs from the compiled reference's digest" % (sc.name, s, k)
                if sc.name == "c4_gather500":
                    assert not any(k in rec for k in ("view0", "feat0", "reward0")), (s, sorted(rec))
    assert counters == [[s + 1] * 3 for s in range(8)], counters
    return [e.engine_stats()[6] for e in seen]


def run_hashed(sc, lib, device_io=False, env_out=None):
    """run(sc, lib) for sizes whose trajectories do not fit in memory: every array of every step is reduced to its
    xxh3-128 (10 GB/s on one core; SHA-256 would cost more than the engines) as soon as the step is over.
    Returns [{key: hex digest} per step]."""
    import xxhash
    steps = []

    def keep(step, rec):
        steps.append({k: xxhash.xxh3_128(np.ascontiguousarray(v).reshape(-1).view(np.uint8)).hexdigest()
                      for k, v in rec.items()})
        rec.clear()

    run(sc, lib, record=keep, device_io=device_io, env_out=env_out)
    return steps


def assert_same_hashed(want, got, what=""):
    assert len(want) == len(got), "%s: step counts differ %d vs %d" % (what, len(want), len(got))
    for s, (a, b) in enumerate(zip(want, got)):
        assert sorted(a) == sorted(b), "%s step %d: keys differ" % (what, s)
        for k in sorted(a):
            assert a[k] == b[k], "%s step %d: %s differs" % (what, s, k)


def battle_formation(map_size, gap=3, first_left=1):
    """the placement of examples/train_battle.py:15-40 (`generate_map`) as Scenario.place entries: two squares of agents on
    every other cell, `side` = 2 * int(sqrt(0.04 * map_size^2)) cells wide, `gap` cells either side of the middle column; the
    script swaps leftID / rightID before it places (train_battle.py:21-22), so the FIRST round of a process puts handles[1] on
    the left and adds it first.  map_size 3536 -> 2 x 707^2 = 2 x 499,849 agents (BASELINE config 5's "1M agents")."""
    import math
    side = int(math.sqrt(map_size * map_size * 0.04)) * 2
    ys = np.arange((map_size - side) // 2, (map_size - side) // 2 + side, 2)

    def square(x0):
        xs = np.arange(x0, x0 + side, 2)
        pos = np.zeros((len(xs) * len(ys), 3), dtype=np.int32)
        pos[:, 0], pos[:, 1] = np.repeat(xs, len(ys)), np.tile(ys, len(xs))      # x outer, y inner: the script's loop order
        return pos

    left, right = square(map_size // 2 - gap - side), square(map_size // 2 + gap)
    return [(first_left, "custom", {"pos": left}), (1 - first_left, "custom", {"pos": right})]


def battle_melee(map_size):
    """the two lattices of battle_formation pushed INTO each other (the state a self-play episode reaches once the fronts have met,
    set up directly): one side on the even columns, the other on the odd columns of the same square -- every agent has hostile
    neighbours at distance 1, half of all cells of the square are occupied"""
    place = battle_formation(map_size)
    (g_l, _, kw_l), (g_r, _, kw_r) = place
    shifted = kw_r["pos"].copy()
    shifted[:, 0] += kw_l["pos"][0, 0] + 1 - shifted[0, 0]
    return [(g_l, "custom", {"pos": kw_l["pos"]}), (g_r, "custom", {"pos": shifted})]


def fullsize_scenarios():
    """BASELINE.json's configurations at their stated sizes.  Too large for full trajectories in memory:
    compared through per-step hashes (run_hashed); goldens from the compiled reference in tests/golden/digests_fullsize.json"""
    rnd = lambda g, n: (g, "random", {"n": n})
    S = [
        # C2: battle 200x200, 2x2000 agents placed by add_agents("random"), 40 steps
        Scenario("c2_battle200", "battle", 200, place=[rnd(0, 2000), rnd(1, 2000)], steps=40),
        # C3(i) with hp 4 / damage 3: deaths from the first step on -- kills, dead_penalty, compaction and the shuffle of
        # ~300k attack-list entries compared bit for bit at 2 x 400k
        Scenario("c3_battle1000_deaths", "battle", 1000, place=[rnd(0, 400000), rnd(1, 400000)], steps=6,
                 over={"small": {"hp": 4, "damage": 3}}),
        # C3(i) as bench.py plays it: default hp (10) / damage (2), 72 steps -- the first deaths come after a few steps, then
        # compaction every step; longer than a bench run (25 cycles), and past the two things of the plain pipeline that only change
        # with the length of an episode: the refill of the claim words (every 63 steps) and the fall from two optimistic pairs of
        # death-rank rounds to one (after 64 steps that did not need the second)
        Scenario("c3_battle1000_long", "battle", 1000, place=[rnd(0, 400000), rnd(1, 400000)], steps=72),
        # a whole episode's length of the multi-launch pipeline at a size the reference plays in a minute: battle 300 x 300, 2 x 10,000,
        # hp 4 / damage 3, 200 steps (examples/train_battle.py plays rounds of 550), reinforcements at steps 70 and 130 so that there are
        # kills in every one of the 200 steps -- three windows of claim-word epochs, the carried round stamps, both pair budgets
        Scenario("battle300_long", "battle", 300, place=[rnd(0, 10000), rnd(1, 10000)], steps=200, action_seed=77,
                 over={"small": {"hp": 4, "damage": 3}},
                 events={70: [("add", 0, "random", {"n": 9000}), ("add", 1, "random", {"n": 9000})],
                         130: [("add", 0, "random", {"n": 9000}), ("add", 1, "random", {"n": 9000})]}),
        # C4: gather 500x500 (train_gather.py), 20k food + 100k agents, only the agents act
        Scenario("c4_gather500", "gather", 500, place=[rnd(0, 20000), rnd(1, 100000)], acting=[1], steps=8),
        # whole episodes of the two smaller BASELINE configurations (round 6): config 2 for the 550 steps of a train_battle.py round (the
        # multi-launch pipeline at 4000 agents: nine epoch windows), config 4 until the agents have starved (train_gather.py's world: the
        # population falls from 100k to a few thousand -- the step moves from the pipeline to the one-launch step on the way)
        Scenario("c2_battle200_episode", "battle", 200, place=[rnd(0, 2000), rnd(1, 2000)], steps=550, action_seed=41),
        Scenario("c4_gather500_episode", "gather", 500, place=[rnd(0, 20000), rnd(1, 100000)], acting=[1], steps=150, action_seed=42),
        # the reference's own 1M harness (scripts/test/test_1m.py:62-71): map sqrt(20 N), N/10 walls, N/2 2x2 predators, N/2 prey
        Scenario("test_1m", "pursuit", 4472, walls=100000, place=[rnd(0, 500000), rnd(1, 500000)], steps=2),
        # C5 at the size BASELINE.json names: examples/train_battle.py --map_size 3536, its own formation (2 x 499,849 on every
        # other cell of two squares 6 columns apart; 12.5 M cells, large_map_mode), 8 steps of random actions
        # (round 6: 66 steps instead of 8 -- past the first refill of the claim words' epoch window and the fall to one optimistic pair at
        # this size too; the fronts meet around step 3, kills from step ~8 on)
        Scenario("c5_battle3536_formation", "battle", 3536, place=battle_formation(3536), steps=66, action_seed=31),
        # ... and the same two lattices interleaved, hp 4 / damage 3: a million agents with hostile neighbours on both sides --
        # ~380k attacks per step nearly all of which land, thousands of kills per step, dense move contention
        Scenario("c5_battle3536_melee", "battle", 3536, place=battle_melee(3536), steps=5, action_seed=32,
                 over={"small": {"hp": 4, "damage": 3}}),
    ]
    return {s.name: s for s in S}


def preset_batch_scenarios():
    """two battle worlds between the one-launch step's limit for an environment on its own (1536 agents) and its limit inside a batch
    (16384): env_set_action_device on such a world leaves tile counts (the multi-launch form), and a batch then steps it in one launch"""
    rnd = lambda g, n: (g, "random", {"n": n})
    return [Scenario("preset_a", "battle", 60, place=[rnd(0, 1000), rnd(1, 1000)], steps=6, action_seed=81, over={"small": {"hp": 4, "damage": 3}}),
            Scenario("preset_b", "battle", 60, place=[rnd(0, 900), rnd(1, 1100)], steps=6, action_seed=82, seed=4242, over={"small": {"hp": 4, "damage": 3}})]


def pipe_batch_scenarios():
    """environments of one env_cycle_many call that take all three of its forms: plain worlds beyond the one-launch step (the batched pipeline,
    pipe.hip: deaths from the first step, a group that dies out, reinforcements that change every grid size mid-episode, a non-square
    large_map_mode world), a world small enough for the two-launch cycle, and gather with BOTH groups observed (under minimap_mode its two groups
    look through different windows, 3 x 3 and 15 x 15: one minimap per environment and cycle does not do, Env::pipe_eligible and Env::cycle_eligible
    refuse it and it goes alone.  With only the agents observed -- as bench.py drives it -- gather goes through the pipeline: pipe_partial_scenarios)"""
    rnd = lambda g, n: (g, "random", {"n": n})
    S = scenarios()
    return [Scenario("pipe_a", "battle", 60, place=[rnd(0, 1000), rnd(1, 1000)], steps=12, action_seed=91, over={"small": {"hp": 4, "damage": 3}}),
            Scenario("pipe_b", "battle", 70, place=[rnd(0, 1500), rnd(1, 700)], steps=12, action_seed=92, seed=99, over={"small": {"hp": 3, "damage": 3, "step_recover": -0.3}},
                     events={4: [("add", 1, "random", {"n": 900})], 8: [("add", 0, "fill", {"pos": (2, 2), "size": (30, 20)})]}),
            Scenario("pipe_c", "battle", 104, place=[rnd(0, 2600), rnd(1, 60)], steps=12, action_seed=93, over={"small": {"damage": 11}}),
            S["battle_brawl"], S["gather"]]


def gather_schedule(step):
    """the observed groups of the `*_changing` gather worlds: the agents (a 15 x 15 window) for four cycles; food (3 x 3) AND agents for two --
    different windows under minimap_mode: one minimap per environment and cycle does not do, the world leaves the batch and goes alone; the
    agents again (back in; the minimap folded into the cycles that went alone was theirs); then the food alone -- the other window, whatever
    minimap the cycle before prepared for "the same groups" is stale"""
    return [1] if step < 4 else [0, 1] if step < 6 else [1] if step < 9 else [0]


def late_schedule(step):
    """the observed groups of the `*_late` battle worlds: nobody before step 3 (no window is known until then: nothing to fold the next
    minimap for), everybody every third step from there on"""
    return [0, 1] if step >= 3 and step % 3 == 0 else []


def pipe_partial_scenarios():
    """worlds of one env_cycle_many call in which groups are left out, as bench.py's gather line leaves the food out (never observed, never
    acting, no reward buffer) -- all of them plain worlds from 1537 agents on for the whole episode: the batched pipeline (pipe.hip), asserted
    cycle by cycle from the engine's own counter (expected_pipe_cycles):
      gather_bench_a/_b : gather as the bench drives it, two replicas with different seeds; food at hp 5 (one hit of the agents' damage 6
                          kills): food is eaten and the unobserved, unrewarded group compacted from the first steps on
      battle_*          : hp 4 / damage 3 (kills in every step); a side that is observed and rewarded but does not act; one that acts but is
                          not observed; one that is neither observed, nor acting, nor rewarded; one side rewarded but not observed while the
                          other is observed but not rewarded
      gather_changing   : gather_schedule; battle_late: late_schedule
      pipe_a, battle_brawl (12 steps of it): a fully observed pipeline world and a two-launch world in the same call
    Every scenario probes in the middle and at the end (Scenario.probe)."""
    import copy
    rnd = lambda g, n: (g, "random", {"n": n})
    hot = {"small": {"hp": 4, "damage": 3}}
    brawl = copy.deepcopy(scenarios()["battle_brawl"])
    brawl.steps = 12
    return [Scenario("gather_bench_a", "gather", 70, place=[rnd(0, 500), rnd(1, 2400)], steps=12, seed=501, action_seed=101, over={"food": {"hp": 5}},
                     acting=[1], observed=[1], rewarded=[1], probe=(6,)),
            Scenario("gather_bench_b", "gather", 70, place=[rnd(0, 600), rnd(1, 2500)], steps=12, seed=502, action_seed=102, over={"food": {"hp": 5}},
                     acting=[1], observed=[1], rewarded=[1], probe=(5,)),
            Scenario("battle_seen_idle", "battle", 64, place=[rnd(0, 1100), rnd(1, 1100)], steps=12, seed=503, action_seed=103, over=hot,
                     acting=[1], probe=(6,)),
            Scenario("battle_blind_actor", "battle", 64, place=[rnd(0, 1100), rnd(1, 1100)], steps=12, seed=504, action_seed=104, over=hot,
                     observed=[1], probe=(6,)),
            Scenario("battle_neither", "battle", 64, place=[rnd(0, 1100), rnd(1, 1100)], steps=12, seed=505, action_seed=105, over=hot,
                     acting=[0], observed=[0], rewarded=[0], probe=(7,)),
            Scenario("battle_paid_blind", "battle", 64, place=[rnd(0, 1100), rnd(1, 1100)], steps=12, seed=506, action_seed=106, over=hot,
                     observed=[0], rewarded=[1], probe=(6,)),
            Scenario("gather_changing", "gather", 70, place=[rnd(0, 500), rnd(1, 2400)], steps=12, seed=507, action_seed=107, over={"food": {"hp": 5}},
                     acting=[1], observed=gather_schedule, rewarded=[1], probe=(7,)),
            Scenario("battle_late", "battle", 64, place=[rnd(0, 1100), rnd(1, 1100)], steps=12, seed=508, action_seed=108, over=hot,
                     observed=late_schedule, rewarded=lambda step: [step % 2], probe=(5,)),
            pipe_batch_scenarios()[0], brawl]


def cycle_partial_scenarios():
    """the same shapes below 1537 agents: the two-launch cycle (k_render_batch + k_step_solo_batch; Env::cycle_prepare makes the next
    cycle's minimap for "the same groups") -- scenarios()["gather"] (300 food + 1200 agents) with only the agents observed and rewarded, the
    same with gather_schedule, a battle world with one side left out altogether, one observed late"""
    rnd = lambda g, n: (g, "random", {"n": n})
    hot = {"small": {"hp": 4, "damage": 3}}
    return [Scenario("gather_partial", "gather", 60, place=[rnd(0, 300), rnd(1, 1200)], acting=[1], steps=20, action_seed=11, over={"food": {"hp": 5}},
                     observed=[1], rewarded=[1], probe=(9,)),
            Scenario("gather_partial_changing", "gather", 60, place=[rnd(0, 300), rnd(1, 1200)], acting=[1], steps=14, action_seed=12, seed=77,
                     over={"food": {"hp": 5}}, observed=gather_schedule, rewarded=[1], probe=(7,)),
            Scenario("battle_partial", "battle", 30, place=[rnd(0, 200), rnd(1, 200)], steps=16, action_seed=13, seed=78, over=hot,
                     acting=[1], observed=[1], rewarded=[1], probe=(8,)),
            Scenario("battle_partial_late", "battle", 30, place=[rnd(0, 200), rnd(1, 200)], steps=16, action_seed=14, seed=79, over=hot,
                     acting=[0, 1], observed=late_schedule, rewarded=[0], probe=(8,))]


def episode_scenarios():
    """whole episodes at full size -- too long for the driver's suite (minutes of GPU time, an hour and a half of single-threaded reference to
    generate): compared once per round by hand (tools/gpu_golden_check.py --episodes; tests/golden/digests_episode.json; the run is kept under
    profiles/).  `c5_battle3536_episode`: BASELINE config 5's world (examples/train_battle.py --map_size 3536, 2 x 499,849 agents in the script's
    own formation) for the 550 steps of one of the script's rounds (train_battle.py:45-140: `while not done` ... `if step_ct > 550: break`)"""
    rnd = lambda g, n: (g, "random", {"n": n})
    return {"c5_battle3536_episode": Scenario("c5_battle3536_episode", "battle", 3536, place=battle_formation(3536), steps=550, action_seed=31),
            # ... and the bench's own workload (C3(i): battle 1000 x 1000, 2 x 400k placed at random) for the same 550 steps
            "c3_battle1000_episode": Scenario("c3_battle1000_episode", "battle", 1000, place=[rnd(0, 400000), rnd(1, 400000)], steps=550)}


def render_episode(lib, out_dir, steps=6, twice=False):
    """a short battle with the text video dump on: returns {file name: bytes} of what env.render() wrote
    (twice: group 0 is given actions a second time before every other step -- the attack events of the literal loop)"""
    sc = Scenario("render", "battle", 16, place=[(0, "random", {"n": 30}), (1, "random", {"n": 30})], steps=steps, action_seed=4,
                  over={"small": {"hp": 3, "damage": 2}})
    env, handles = sc.build(lib)
    env.set_render_dir(out_dir)
    rs = np.random.RandomState(sc.action_seed)
    for step in range(steps):
        for h in handles:
            env.set_action(h, rs.randint(21, size=env.get_num(h)).astype(np.int32))
        if twice and step % 2 == 1:
            env.set_action(handles[0], rs.randint(21, size=env.get_num(handles[0])).astype(np.int32))
        env.step()
        env.render()                       # before clear_dead, like examples/train_battle.py:88-96
        if step == 2:
            env._get_render_info((0, 15), (0, 15))
        env.clear_dead()
    return {name: open(os.path.join(out_dir, name), "rb").read() for name in sorted(os.listdir(out_dir))}


_ATTACK_COUNT = {0: 0, 1: 4, 1.5: 8, 2: 12, 2.5: 20}


def sector_shape(radius, angle, parity):
    """(width, height, count) of the reference's SectorRange (Range.h:104-144), float32 inputs as the C-ABI passes them"""
    import math
    PI = 3.1415926536
    radius, angle = np.float32(radius), np.float32(angle)
    height = int(float(radius) + 0.5)
    width = int(float(np.float32(2) * radius) * math.sin(float(angle / np.float32(2)) * (PI / 180)) + 0.5)
    if width % 2 != parity:
        width -= 1
    count = 0
    for i in range(height):
        for j in range(max(width, 0)):
            dx, dy = abs(j - (width - 1) / 2.0), abs(height - i)
            if math.sqrt(dx * dx + dy * dy) < float(radius) + 0.2 + 0.00001 and dx / dy < math.tan(float(angle / np.float32(2)) * PI / 180) + 0.00001:
                count += 1
    return width, height, count

TURN_MULTICELL_ON_ENGINE = True       # turn_mode with bodies larger than one cell / goals (the generic turn phase)


def fuzz_scenario(seed):
    """a random game inside the engine's scope: 2-4 groups, random body sizes / ranges / hp / damage / recover /
    kill_supply / in-group attack, random rules (subject and object receivers, attack | kill | collide, pairs of events
    joined by `&`), food_mode, random map
    shape, walls, densities, clear_dead cadence and non-acting groups -- for differential testing"""
    rs = np.random.RandomState(seed)
    G = int(rs.choice([2, 2, 2, 3, 3, 4]))
    w = int(rs.randint(12, 150))
    h = w if rs.rand() < 0.5 else int(rs.randint(12, 150))
    minimap, emb = bool(rs.rand() < 0.6), int(rs.choice([0, 3, 10]))
    food_mode = False
    # FUZZ_TURN=1: turn_mode in 60 % of the games; FUZZ_TURN=2: the same draws, but turn_mode only stays on in games the engine
    # takes today (see Env::reset)
    fuzz_turn = int(os.environ.get("FUZZ_TURN", "0"))
    turn_mode = fuzz_turn >= 1 and bool(rs.rand() < 0.6)
    frac = lambda lo, hi: float(rs.randint(int(lo * 16), int(hi * 16) + 1)) / 16.0
    while True:
        specs = []
        for g in range(G):
            bw, bl = (1, 1) if rs.rand() < 0.65 else (int(rs.randint(1, 4)), int(rs.randint(1, 4)))
            specs.append(dict(width=bw, length=bl, hp=frac(1, 12), speed=float(rs.choice([0, 1, 1, 1.5, 2, 2, 3])),
                              view_range=float(rs.choice([1, 2, 3, 4, 5, 6, 7])), attack_range=float(rs.choice([0, 1, 1, 1.5, 1.5, 2, 2.5])),
                              damage=frac(0, 6), step_recover=float(rs.choice([0, 0, 0.1, 0.25, -0.25, -0.5])),
                              kill_supply=float(rs.choice([0, 0, 0, 2.5, 8])), attack_in_group=int(rs.rand() < 0.3),
                              step_reward=frac(-0.25, 0.25), kill_reward=frac(0, 5), dead_penalty=frac(-2, 0),
                              attack_penalty=frac(-0.5, 0)))
        # FUZZ_SECTOR=1: sector ranges (a wedge in front of the agent) for some views and attacks
        for t in specs:
            t["n_attack"] = _ATTACK_COUNT[t["attack_range"]]
            if os.environ.get("FUZZ_SECTOR", "0") == "1":
                parity = t["width"] % 2
                if rs.rand() < 0.35:
                    r, a = float(rs.choice([3, 4, 5, 6, 7])), float(rs.choice([40, 60, 90, 120, 150]))
                    if sector_shape(r, a, parity)[0] >= 1:
                        t["view_sector"] = (r, a)
                if rs.rand() < 0.35:
                    r, a = float(rs.choice([1, 1.5, 2, 2.5, 3])), float(rs.choice([40, 60, 90, 120, 150]))
                    wd, ht, cnt = sector_shape(r, a, parity)
                    if wd >= 1:
                        t["attack_sector"], t["n_attack"] = (r, a), cnt
        # engine limits: the attack offsets of all groups share a 32-bit word; hit lists are bounded
        if sum(t["n_attack"] for t in specs) > 32:
            continue
        kmax = max(t["width"] * t["length"] * sum(a["n_attack"] for j, a in enumerate(specs)
                                                  if j != i or a["attack_in_group"]) for i, t in enumerate(specs))
        if kmax * (4 if turn_mode else 1) <= 256 and all(max(t["width"], t["length"]) + 2 < min(w, h) for t in specs):
            break
    # FUZZ_PLAIN=1: the same draws, bent into a game the pipeline of plain games takes (Env::reset: plain_world) with rules k_strike evaluates
    # itself -- one-cell bodies, no kill_supply / food / goals / turn_mode, one view window, subject-paying attack | kill rules only --
    # so that batches of them go through env_cycle_many's batched pipeline (pipe.hip)
    fuzz_plain = os.environ.get("FUZZ_PLAIN", "0") == "1"
    if fuzz_plain:
        turn_mode = False
        for t in specs:
            t.update(width=1, length=1, kill_supply=0.0, view_range=specs[0]["view_range"])
            t.pop("view_sector", None)
    rules = []
    for _ in range(int(rs.randint(0, 5))):
        a, b = int(rs.randint(G)), int(rs.randint(G))
        op = str(rs.choice(["attack", "attack", "kill", "collide"]))
        who = str(rs.choice(["s", "o", "so", "os", "ss"]))
        if a == b and "s" in who and "o" in who:
            who = "s"
        rules.append((a, op, b, who, [frac(-1, 1) for _ in who]))
    pair_rules = []
    for _ in range(int(rs.choice([0, 0, 1, 2]))):
        a, b, c = int(rs.randint(G)), int(rs.randint(G)), int(rs.randint(G))
        who = str(rs.choice(["ab", "ba", "a", "b", "abc", "cab", "aab", "c"]))
        if c in (a, b):
            who = who.replace("c", "") or "a"          # the object is paid only from another group (engine scope)
        pair_rules.append((a, b, str(rs.choice(["attack", "attack", "kill"])), str(rs.choice(["attack", "attack", "kill"])), c,
                           who, [frac(-1, 1) for _ in who], bool(rs.rand() < 0.5)))

    # expressions the engine takes: and / or / not over die / at / in / attack / kill / collide whose search iterates ONE symbol x
    # (a second symbol y only as the partner of a binary event with x)
    prog_rules = []
    for _ in range(int(rs.choice([0, 0, 1, 1, 2]))):
        gx, gy = int(rs.randint(G)), int(rs.randint(G))
        two = bool(rs.rand() < 0.6)
        def pleaf(force_binary=False):
            kind = "bin" if force_binary else str(rs.choice(["die", "at", "in", "bin", "bin"] if two else ["die", "at", "in"]))
            who = int(rs.randint(2)) if two else 0
            if kind == "die":
                return ("die", who)
            if kind == "at":
                return ("at", who, (int(rs.randint(1, w - 1)), int(rs.randint(1, h - 1))))
            if kind == "in":
                return ("in", who, ((int(rs.randint(0, w)), int(rs.randint(0, h))), (int(rs.randint(0, w)), int(rs.randint(0, h)))))
            return (str(rs.choice(["attack", "kill", "collide"])), who, 1 - who)
        def ptree(depth):
            if depth == 0 or rs.rand() < 0.4:
                return pleaf()
            op = str(rs.choice(["and", "or", "not"]))
            return (op, ptree(depth - 1)) if op == "not" else (op, ptree(depth - 1), ptree(depth - 1))
        expr = ptree(2)
        def has_binary(e):
            return e[0] in ("attack", "kill", "collide") or (e[0] in ("and", "or", "not") and any(has_binary(c) for c in e[1:]))
        if two and not has_binary(expr):
            expr = (str(rs.choice(["and", "or"])), expr, pleaf(force_binary=True))
        who = str(rs.choice(["x", "x", "y", "xy", "yx", "xx"])) if two else str(rs.choice(["x", "xx"]))
        if two and gx == gy and "x" in who and "y" in who:
            who = "x"
        prog_rules.append((gx, gy, two, expr, who, [frac(-1, 1) for _ in who], bool(rs.rand() < 0.05)))

    # FUZZ_RULES=1 (oracle-vs-reference runs only: the engine refuses these shapes): random expressions over die / at / in and
    # the binary events, joined by & | ~ -- they pin the oracle's literal restatement of the recursive rule search
    tree_rules = []
    fuzz_rules = int(os.environ.get("FUZZ_RULES", "0"))
    if fuzz_rules >= 1:
        # FUZZ_RULES=2 adds what only the recursive search handles: 'all' and fixed-index symbols, in_a_line.  Kept inside what
        # the reference defines: the object of a binary event is never 'all', in_a_line only takes 'all' (it asserts both)
        for _ in range(int(rs.randint(1, 4))):
            n_sym = int(rs.randint(1, 4))
            syms = [int(rs.randint(G)) for _ in range(n_sym)]      # group of each symbol
            kinds = ["any"] * n_sym
            if fuzz_rules >= 2:
                kinds = [str(rs.choice(["any", "any", "any", "any", "all", "idx"])) for _ in range(n_sym)]
                kinds = [int(rs.randint(0, 4)) if k == "idx" else k for k in kinds]
            def leaf():
                a = int(rs.randint(len(syms)))
                kind = str(rs.choice(["die", "at", "in", "bin", "bin"] + (["line"] if kinds[a] == "all" else [])))
                if kind == "line":
                    return ("in_a_line", a)
                if kind == "die":
                    return ("die", a)
                if kind == "at":
                    return ("at", a, (int(rs.randint(1, w - 1)), int(rs.randint(1, h - 1))))
                if kind == "in":
                    return ("in", a, ((int(rs.randint(0, w)), int(rs.randint(0, h))), (int(rs.randint(0, w)), int(rs.randint(0, h)))))
                objs = [k for k in range(len(syms)) if kinds[k] != "all"]
                if not objs:
                    return ("die", a)
                b = int(rs.choice(objs))
                return (str(rs.choice(["attack", "kill", "collide"])), a, b)
            def tree(depth):
                if depth == 0 or rs.rand() < 0.4:
                    return leaf()
                op = str(rs.choice(["and", "or", "not"]))
                return (op, tree(depth - 1)) if op == "not" else (op, tree(depth - 1), tree(depth - 1))
            expr = tree(2)
            used = set()
            def collect(e):
                if e[0] in ("and", "or", "not"):
                    for c in e[1:]:
                        collect(c)
                else:
                    used.add(e[1])
                    if e[0] in ("attack", "kill", "collide"):
                        used.add(e[2])
            collect(expr)
            recv = [k for k in sorted(used) if rs.rand() < 0.7] or [sorted(used)[0]]
            tree_rules.append((syms, kinds, expr, recv, [frac(-1, 1) for _ in recv], bool(rs.rand() < 0.1)))

    if fuzz_plain:
        rules = [(a, "attack" if op == "collide" else op, b, "s" * len(who), vals) for a, op, b, who, vals in rules]
        pair_rules, prog_rules = [], []

    def make():
        cfg = gw.Config()
        cfg.set({"map_width": w, "map_height": h, "minimap_mode": minimap, "embedding_size": emb})
        if food_mode:
            cfg.set({"food_mode": True})
        if turn_mode:
            cfg.set({"turn_mode": True})
        if goal_mode:
            cfg.set({"goal_mode": True})
        names = []
        for g, t in enumerate(specs):
            t = dict(t)
            t["view_range"] = gw.SectorRange(*t["view_sector"]) if "view_sector" in t else gw.CircleRange(t["view_range"])
            t["attack_range"] = gw.SectorRange(*t["attack_sector"]) if "attack_sector" in t else gw.CircleRange(t["attack_range"])
            for k in ("view_sector", "attack_sector", "n_attack"):
                t.pop(k, None)
            names.append(cfg.register_agent_type("t%d" % g, t))
        hs = [cfg.add_group(n) for n in names]
        for a, op, b, who, vals in rules:
            sa, sb = gw.AgentSymbol(hs[a], "any"), gw.AgentSymbol(hs[b], "any")
            cfg.add_reward_rule(gw.Event(sa, op, sb), receiver=[{"s": sa, "o": sb}[c] for c in who], value=vals)
        for a, b, opa, opb, c, who, vals, b_first in pair_rules:
            if b_first:
                sb, sa = gw.AgentSymbol(hs[b], "any"), gw.AgentSymbol(hs[a], "any")
            else:
                sa, sb = gw.AgentSymbol(hs[a], "any"), gw.AgentSymbol(hs[b], "any")
            sc_ = gw.AgentSymbol(hs[c], "any")
            cfg.add_reward_rule(gw.Event(sa, opa, sc_) & gw.Event(sb, opb, sc_),
                                receiver=[{"a": sa, "b": sb, "c": sc_}[k] for k in who], value=vals)
        def build_expr(S, e):
            if e[0] == "and":
                return build_expr(S, e[1]) & build_expr(S, e[2])
            if e[0] == "or":
                return build_expr(S, e[1]) | build_expr(S, e[2])
            if e[0] == "not":
                return ~build_expr(S, e[1])
            if e[0] == "die":
                return gw.Event(S[e[1]], "die")
            if e[0] in ("at", "in"):
                return gw.Event(S[e[1]], e[0], e[2])
            return gw.Event(S[e[1]], e[0], S[e[2]])
        for gx, gy, two, expr, who, vals, terminal in prog_rules:
            S = [gw.AgentSymbol(hs[gx], "any"), gw.AgentSymbol(hs[gy], "any")]
            cfg.add_reward_rule(build_expr(S, expr), receiver=[S["xy".index(c)] for c in who], value=vals, terminal=terminal)
        for syms, kinds, expr, recv, vals, terminal in tree_rules:
            S = [gw.AgentSymbol(hs[g], kinds[q]) for q, g in enumerate(syms)]
            def build(e):
                if e[0] == "and":
                    return build(e[1]) & build(e[2])
                if e[0] == "or":
                    return build(e[1]) | build(e[2])
                if e[0] == "not":
                    return ~build(e[1])
                if e[0] in ("die", "in_a_line"):
                    return gw.Event(S[e[1]], e[0])
                if e[0] in ("at", "in"):
                    return gw.Event(S[e[1]], e[0], e[2])
                return gw.Event(S[e[1]], e[0], S[e[2]])
            cfg.add_reward_rule(build(expr), receiver=[S[k] for k in recv], value=vals, terminal=terminal)
        return cfg

    area = (w - 2) * (h - 2)
    density = float(rs.choice([0.03, 0.1, 0.2, 0.3]))
    if any(t["width"] * t["length"] > 1 for t in specs):
        density = min(density, 0.12)       # rejection-sampled placement of big bodies needs room
    place = []
    for g, t in enumerate(specs):
        n = max(1, int(area * density / G / (t["width"] * t["length"])))
        if rs.rand() < 0.15:
            place.append((g, "fill", {"pos": (int(rs.randint(1, w // 2)), int(rs.randint(1, h // 2))),
                                      "size": (int(rs.randint(2, w // 5 + 3)), int(rs.randint(2, h // 5 + 3)))}))
        place.append((g, "random", {"n": min(n, 4000)}))
    acting = [g for g in range(G) if rs.rand() < 0.85] or [0]
    if rs.rand() < 0.3 and not fuzz_plain:           # food_mode: the killed leave food, attackers eat it
        food_mode = True
        for t in specs:
            t["food_supply"] = float(rs.choice([0, 0.05, 1, 2.5, 6]))
            t["eat_ability"] = float(rs.choice([0, 0.5, 1, 3]))
    if rs.rand() < 0.15 and not fuzz_plain:          # one group of goals (can_absorb); goals are never given actions (engine scope)
        goal = int(rs.randint(G))
        specs[goal]["can_absorb"] = True
        if os.environ.get("FUZZ_GOALS_ACT", "0") != "1":     # (=1: the goals are given actions like everybody -- they move: the literal loop)
            acting = [g for g in acting if g != goal]
    if fuzz_turn == 2 and turn_mode and not TURN_MULTICELL_ON_ENGINE and any(t["width"] * t["length"] > 1 or t.get("can_absorb") for t in specs):
        turn_mode = False
    # FUZZ_GOAL=1: goal_mode in half of the games and set_goal calls between steps (a generator of their own: the games of a seed stay
    # what they are without it)
    goal_mode, events = False, {}
    if os.environ.get("FUZZ_GOAL", "0") == "1":
        rg = np.random.RandomState(seed ^ 0x60A1)
        goal_mode = bool(rg.rand() < 0.5)
        for _ in range(int(rg.randint(1, 4))):
            events.setdefault(int(rg.randint(0, 8)), []).append(("goal", int(rg.randint(G))))
    sc = Scenario("fuzz%d" % seed, make, 0, seed=int(rs.randint(1, 1 << 20)), place=place, steps=int(rs.randint(6, 14)),
                  action_seed=seed, walls=int(area * float(rs.choice([0, 0, 0.02, 0.08]))), acting=acting,
                  clear_every=int(rs.choice([1, 1, 1, 2])), obs_every=int(rs.choice([1, 1, 2])), events=events)
    # FUZZ_PARTIAL=1 (with FUZZ_PLAIN=1; drawn behind everything else: the game of a seed stays what it is without it): groups left out of
    # the observations (at least one stays) and, independently, of the rewards -- run_cycle / run_cycle_batch hand over NULL entries for
    # them -- and, where there is no minimap (one minimap per environment and cycle: Env::pipe_eligible), a window of its own per group;
    # everybody is observed in the middle and at the end (Scenario.probe)
    if fuzz_plain and os.environ.get("FUZZ_PARTIAL", "0") == "1":
        sc.observed = [g for g in range(G) if rs.rand() < 0.6] or [int(rs.randint(G))]
        sc.rewarded = [g for g in range(G) if rs.rand() < 0.6]
        if not minimap:
            for t in specs:
                t["view_range"] = float(rs.choice([1, 2, 3, 4, 5, 6, 7]))
        sc.probe = (sc.steps // 2,)
    return sc


def digest(trajectory):
    """SHA-256 over every array of every step (dtype + shape + bytes), in key order"""
    h = hashlib.sha256()
    for rec in trajectory:
        for k in sorted(rec):
            a = np.ascontiguousarray(rec[k])
            h.update(k.encode()); h.update(str(a.dtype).encode()); h.update(str(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()


def assert_same(ta, tb, what=""):
    """bit-exact comparison of two trajectories (floats compared as raw uint32)"""
    assert len(ta) == len(tb), "%s: step counts differ %d vs %d" % (what, len(ta), len(tb))
    for s, (ra, rb) in enumerate(zip(ta, tb)):
        assert sorted(ra) == sorted(rb), "%s step %d: keys differ" % (what, s)
        for k in sorted(ra):
            a, b = np.ascontiguousarray(ra[k]), np.ascontiguousarray(rb[k])
            assert a.shape == b.shape and a.dtype == b.dtype, "%s step %d %s: shape/dtype %s%s vs %s%s" % (
                what, s, k, a.dtype, a.shape, b.dtype, b.shape)
            if a.dtype == np.float32:
                a, b = a.view(np.uint32), b.view(np.uint32)
            if not np.array_equal(a, b):
                bad = np.argwhere(a != b)
                raise AssertionError("%s step %d %s: %d mismatching elements, first at %s: %r vs %r" % (
                    what, s, k, len(bad), tuple(bad[0]), ra[k][tuple(bad[0])], rb[k][tuple(bad[0])]))


# the scenario table: sizes the CPU checkers finish in seconds.  Covers the reference's edge cases for this path:
# dense attacks (order dependence), walls, large_map_mode stripes (> 99x99), in-group attack (gather), a group that
# does not act (food), deaths + clear_dead compaction, skipped clear_dead (dead agents stay listed), map borders.
def scenarios():
    rnd = lambda g, n: (g, "random", {"n": n})
    S = [
        Scenario("battle_small_dense", "battle", 30, place=[rnd(0, 150), rnd(1, 150)], steps=25),
        Scenario("battle_brawl", "battle", 20, place=[rnd(0, 120), rnd(1, 120)], steps=25, action_seed=1,
                 over={"small": {"hp": 4, "damage": 3, "step_recover": 0}}),
        Scenario("battle_brawl_big", "battle", 110, place=[rnd(0, 4500), rnd(1, 4500)], steps=14, action_seed=2,
                 over={"small": {"hp": 5, "damage": 3, "step_recover": 0.3}}),
        Scenario("battle60", "battle", 60, place=[rnd(0, 1200), rnd(1, 1200)], steps=40),
        # a long episode: the plain pipeline's claim words carry an epoch that wraps every 63 steps (step.hip: claim_word)
        Scenario("battle_epochs", "battle", 26, place=[rnd(0, 90), rnd(1, 90)], steps=140, action_seed=61, over={"small": {"hp": 6}},
                 events={40: [("add", 0, "random", {"n": 50}), ("add", 1, "random", {"n": 50})],
                         85: [("add", 0, "random", {"n": 60}), ("add", 1, "random", {"n": 60})], 120: [("add", 1, "random", {"n": 40})]}),
        # goal_mode: two feature slots that nothing writes (GridWorld.cc:926-934); set_goal: two draws of the engine's generator per agent,
        # with or without goal_mode (GridWorld.cc:667-679) -- seen in the shuffles and the placements that follow
        Scenario("battle_goal_mode", "battle", 28, place=[rnd(0, 110), rnd(1, 110)], steps=16, action_seed=62, settings={"goal_mode": True},
                 over={"small": {"hp": 4, "damage": 3}}, clear_every=2,
                 events={0: [("goal", 0)], 5: [("goal", 1), ("add", 0, "random", {"n": 30})], 9: [("goal", 0), ("goal", 1)]}),
        Scenario("pursuit_goals_drawn", "pursuit", 30, walls=20, place=[rnd(0, 40), rnd(1, 80)], steps=14, action_seed=63,
                 events={3: [("goal", 1)], 4: [("add", 1, "random", {"n": 25})], 8: [("goal", 0)]}),
        # goals that are given actions: Map::do_move treats a goal that has taken nobody in like any mover (Map.cc:313-358; one that has
        # stands still, GridWorld.cc:580) -- the parallel move resolution rests on goals that stand still, so these steps run the
        # reference's own loops on one lane of the device (k_step_serial)
        Scenario("arrange_goals_move", ("arrange", 36, True), 0, place=[rnd(0, 150), rnd(1, 250), rnd(2, 30)], walls=40, steps=25, action_seed=64),
        Scenario("arrange_goals_move_turn", ("arrange", 40, True), 0, place=[rnd(0, 160), rnd(1, 260), rnd(2, 30)], walls=30, steps=20, action_seed=65,
                 settings={"turn_mode": True}, clear_every=2),
        # ... and goals that are given actions every step but told to stay where they are (the zero move): an ordinary step of the parallel
        # phases -- Env::set_action_device looks at the actions before it sends a step through the literal loop
        Scenario("arrange_goals_stand", ("arrange", 36, True), 0, place=[rnd(0, 150), rnd(1, 250), rnd(2, 30)], walls=40, steps=25, action_seed=66, still=(0,)),
        Scenario("arrange_goals_stand_turn", ("arrange", 40, True), 0, place=[rnd(0, 160), rnd(1, 260), rnd(2, 30)], walls=30, steps=20, action_seed=67,
                 settings={"turn_mode": True}, clear_every=2, still=(0,)),
        Scenario("battle_walls", "battle", 50, walls=200, place=[rnd(0, 400), rnd(1, 400)], steps=20, action_seed=3),
        Scenario("battle_largemap", "battle", 120, place=[rnd(0, 3000), rnd(1, 3000)], steps=12, action_seed=5),
        Scenario("battle_largemap_odd", "battle", 101, place=[rnd(0, 2500), rnd(1, 2500)], steps=10, action_seed=6),
        Scenario("battle_fill_full", "battle", 40,
                 place=[(0, "fill", {"pos": (1, 1), "size": (19, 38)}), (1, "fill", {"pos": (20, 1), "size": (19, 38)})],
                 steps=15, action_seed=7),
        Scenario("battle_no_clear", "battle", 40, place=[rnd(0, 400), rnd(1, 400)], steps=12, clear_every=3, action_seed=8),
        Scenario("battle_tiny", "battle", 8, place=[(0, "custom", {"pos": [(1, 1), (6, 6)]}), (1, "custom", {"pos": [(2, 1)]})],
                 steps=8, action_seed=9),
        Scenario("gather", "gather", 60, place=[rnd(0, 300), rnd(1, 1200)], acting=[1], steps=20, action_seed=11),
        Scenario("gather_largemap", "gather", 130, place=[rnd(0, 1500), rnd(1, 6000)], acting=[1], steps=8, action_seed=12),
        Scenario("battle_lowhp", "battle", 40, place=[rnd(0, 500), rnd(1, 500)], steps=15, action_seed=13,
                 over={"small": {"hp": 3, "step_recover": -0.4}}),
        Scenario("battle_brawl_dense_big", "battle", 300, place=[rnd(0, 40000), rnd(1, 40000)], steps=6, action_seed=21,
                 obs_every=3, over={"small": {"hp": 4, "damage": 3, "step_recover": 0}}),
        Scenario("forest", "forest", 50, place=[rnd(0, 500), rnd(1, 250)], walls=60, steps=25, action_seed=15),
        Scenario("tri_rect", ("tri", 70, 45), 0, place=[rnd(0, 500), rnd(1, 400), rnd(2, 450)], walls=80, steps=25, action_seed=16),
        Scenario("tri_rect_large", ("tri", 150, 101), 0, place=[rnd(0, 3000), rnd(1, 3000), rnd(2, 2500)], steps=10, action_seed=17),
        Scenario("quad", ("quad", 36), 0, place=[rnd(0, 150), rnd(1, 150), rnd(2, 150), rnd(3, 150)], steps=20, action_seed=22),
        Scenario("pursuit", "pursuit", 40, walls=48, place=[rnd(0, 20), rnd(1, 40)], steps=40, action_seed=23),
        Scenario("pursuit_dense", "pursuit", 30, walls=30, place=[rnd(0, 60), rnd(1, 120)], steps=30, action_seed=24),
        Scenario("pursuit_large", "pursuit", 140, walls=600, place=[rnd(0, 1500), rnd(1, 3000)], steps=10, action_seed=25),
        Scenario("bodies", ("bodies", 48, 37), 0, walls=40, place=[rnd(0, 60), rnd(1, 90), rnd(2, 150)], steps=30, action_seed=26),
        Scenario("bodies_large", ("bodies", 130, 111), 0, walls=300, place=[rnd(0, 500), rnd(1, 900), rnd(2, 1500),
                 (0, "fill", {"pos": (100, 80), "size": (12, 10)})], steps=10, action_seed=27),
        Scenario("trans", ("trans", 40), 0, walls=150, place=[rnd(0, 300), (0, "fill", {"pos": (60, 10), "size": (4, 12)})],
                 steps=15, action_seed=29),
        Scenario("chase", ("chase", 40), 0, place=[rnd(0, 150), rnd(1, 300)], walls=40, steps=20, action_seed=18),
        Scenario("battle_events", "battle", 45, place=[rnd(0, 300), rnd(1, 300)], steps=24, action_seed=19,
                 over={"small": {"hp": 4, "damage": 3}},
                 events={5: [("add", 0, "random", {"n": 80}), ("walls", "random", {"n": 30})],
                         9: [("add", 1, "custom", {"pos": [(1, 1), (2, 2), (2, 2), (43, 43), (0, 0)]}),
                             ("walls", "fill", {"pos": (20, 20), "size": (3, 2)})],
                         14: [("reset", [(0, "random", {"n": 200}), (1, "fill", {"pos": (5, 5), "size": (10, 12)})])]}),
        Scenario("battle_grow", "battle", 70, place=[rnd(0, 50), rnd(1, 50)], steps=12, action_seed=28,
                 over={"small": {"hp": 4, "damage": 3}},
                 events={3: [("add", 0, "random", {"n": 1800})], 6: [("add", 1, "random", {"n": 1500})],
                         9: [("add", 0, "fill", {"pos": (2, 2), "size": (6, 60)})]}),
        Scenario("double_attack", "double_attack", 30, place=[rnd(0, 120), rnd(1, 200)], walls=20, steps=25, action_seed=31),
        Scenario("duo", ("duo", 34), 0, place=[rnd(0, 150), rnd(1, 260), rnd(2, 60)], walls=30, steps=25, action_seed=32),
        Scenario("duo_dense", ("duo", 26), 0, place=[rnd(0, 80), rnd(1, 300), rnd(2, 30)], steps=20, action_seed=34),
        Scenario("duo_large", ("duo", 120), 0, place=[rnd(0, 2500), rnd(1, 3500), rnd(2, 800)], steps=8, action_seed=33),
        Scenario("arrange", ("arrange", 40, False), 0, place=[rnd(0, 180), rnd(1, 300)], walls=60, acting=[1], steps=30, action_seed=35),
        Scenario("arrange_live", ("arrange", 44, True), 0, place=[rnd(0, 220), rnd(1, 350), rnd(2, 40)], walls=40, steps=30,
                 acting=[1, 2], action_seed=36, clear_every=2),
        Scenario("arrange_large", ("arrange", 125, True), 0, place=[rnd(0, 2500), rnd(1, 3500), rnd(2, 300)], steps=10,
                 acting=[1, 2], action_seed=37),
        Scenario("battle_food", "battle", 24, place=[rnd(0, 160), rnd(1, 160)], steps=30, action_seed=38, settings={"food_mode": True},
                 over={"small": {"hp": 4, "damage": 3, "step_recover": -0.05, "food_supply": 2.5, "eat_ability": 1}}),
        Scenario("bodies_food", ("bodies", 48, 37), 0, walls=40, place=[rnd(0, 60), rnd(1, 90), rnd(2, 150)], steps=30, action_seed=39,
                 settings={"food_mode": True},
                 over={"big": {"food_supply": 6, "eat_ability": 2}, "mid": {"food_supply": 0.05, "eat_ability": 0.5}, "tiny": {"food_supply": 1, "eat_ability": 3}}),
        Scenario("rules_mix", ("rules", 30), 0, place=[rnd(0, 140), rnd(1, 140), rnd(2, 25)], walls=20, steps=30, action_seed=40),
        Scenario("rules_mix_large", ("rules", 110), 0, place=[rnd(0, 2500), rnd(1, 2500), rnd(2, 300)], steps=8, action_seed=41),
        Scenario("sector", ("sector", 44, 37), 0, walls=40, place=[rnd(0, 150), rnd(1, 40), rnd(2, 120)], steps=25, action_seed=52),
        Scenario("sector_turn", ("sector", 50, 41), 0, walls=50, place=[rnd(0, 180), rnd(1, 45), rnd(2, 150)], steps=25, action_seed=53,
                 settings={"turn_mode": True}),
        Scenario("sector_turn_large", ("sector", 130, 105), 0, walls=300, place=[rnd(0, 1800), rnd(1, 350), rnd(2, 1500)], steps=8, action_seed=54,
                 settings={"turn_mode": True}),
        Scenario("rules_search", ("search", 26), 0, place=[rnd(0, 60), rnd(1, 60), (2, "custom", {"pos": [(5, 3), (5, 4), (5, 5), (5, 6)]})],
                 walls=10, steps=30, action_seed=44),
        Scenario("rules_search_grow", ("search", 30), 0, place=[rnd(0, 40), rnd(1, 40), (2, "custom", {"pos": [(8, 20), (9, 20), (10, 20)]})],
                 steps=20, action_seed=45, clear_every=2,
                 events={4: [("add", 0, "random", {"n": 30})], 9: [("add", 1, "random", {"n": 25}), ("add", 2, "custom", {"pos": [(11, 20)]})]}),
        Scenario("battle_turn", "battle", 26, place=[rnd(0, 120), rnd(1, 120), (0, "custom", {"pos": [(1, 1, 0), (3, 1, 1), (1, 3, 2), (3, 3, 3)]})],
                 steps=25, action_seed=42, settings={"turn_mode": True}),
        Scenario("battle_turn_large", "battle", 130, place=[rnd(0, 3500), rnd(1, 3500)], steps=10, action_seed=46, settings={"turn_mode": True},
                 over={"small": {"hp": 4, "damage": 3}}),
        Scenario("gather_turn", "gather", 50, place=[rnd(0, 200), rnd(1, 700)], acting=[1], steps=20, action_seed=47, settings={"turn_mode": True}),
        Scenario("tri_turn", ("tri", 60, 41), 0, place=[rnd(0, 400), rnd(1, 300), rnd(2, 350)], walls=60, steps=25, action_seed=48,
                 settings={"turn_mode": True}),
        Scenario("bodies_turn", ("bodies", 48, 37), 0, walls=40, place=[rnd(0, 50), rnd(1, 80), rnd(2, 150),
                 (0, "fill", {"pos": (30, 20), "size": (8, 9), "dir": 2})], steps=25, action_seed=43, settings={"turn_mode": True}),
        Scenario("pursuit_turn", "pursuit", 36, walls=40, place=[rnd(0, 50), rnd(1, 100)], steps=30, action_seed=49, settings={"turn_mode": True}),
        Scenario("bodies_turn_large", ("bodies", 120, 101), 0, walls=250, place=[rnd(0, 450), rnd(1, 800), rnd(2, 1300)], steps=10, action_seed=50,
                 settings={"turn_mode": True}),
        Scenario("arrange_turn", ("arrange", 40, True), 0, place=[rnd(0, 200), rnd(1, 300), rnd(2, 35)], walls=30, steps=25, acting=[1, 2], action_seed=51,
                 settings={"turn_mode": True}),
        Scenario("battle_one_side", "battle", 12, place=[rnd(0, 60), rnd(1, 3)], steps=40, action_seed=14,
                 over={"small": {"damage": 12}}),
    ]
    return {s.name: s for s in S}


# ---------------------------------------------------------------------------------------------------- caller-owned output buffers under guard
# (tests/test_engine_buffers.py, tools/mutation_buffers.py)
GUARD_BYTES = 64 * 1024            # a workgroup's worth of stray 16-byte stores (256 x 16 B = 4 KiB) lands well inside
# a word no correct output holds: a NaN with a payload for float32 (the engine's own NaN is 0xFFC00000) -- as an id, a position or a
# float's bits in int32 it is 2,141,570,017; a bf16 NaN with a payload; a byte that is neither 0 nor 1
SENTINEL = {4: 0x7FA5C3E1, 2: 0x7FA5, 1: 0xA5}
_GUARD_TYPES = {"float32": (4, np.float32), "int32": (4, np.int32), "bfloat16": (2, np.uint16), "bool": (1, np.uint8)}
_WORD_TYPES = {4: np.uint32, 2: np.uint16, 1: np.uint8}


class Guarded(object):
    """one allocation [guard | interior | guard] of sentinel words (guarded): `words` the whole allocation as integer words from a 16-byte
    boundary on, `front` the interior's first word, `n` rows of `row` words in use of `cap`, `interior` the n rows as a contiguous view, `ptr`
    its address (valid for zero rows too)"""


def guarded(shape, dtype, lib_or_dev, offset_elems=0, capacity_rows=None):
    """A caller-owned output buffer of `shape` (rows first) between two guards of at least 64 KiB, everything prefilled with the sentinel of the
    element size (SENTINEL).  dtype: "float32", "int32", "bfloat16" or "bool" (one byte per element).  lib_or_dev: "numpy" (the host ABI), a
    torch.device, or an engine library's path / None (the device its *_device calls take: helpers.is_emu -> CPU tensors, else cuda:0).  The
    interior starts `offset_elems` elements behind a 16-byte boundary; capacity_rows >= shape[0] makes it that many rows long, as the
    wrapper's cached observation buffers are (buf[:n]) -- the rows past shape[0] count as guard.  A zero-row interior is a valid pointer
    into the allocation."""
    word, np_type = _GUARD_TYPES[dtype]
    n, row = int(shape[0]), int(np.prod(shape[1:], dtype=np.int64))
    cap = n if capacity_rows is None else int(capacity_rows)
    assert cap >= n and 0 <= offset_elems * word < 4096
    front = GUARD_BYTES // word + offset_elems
    total = front + cap * row + GUARD_BYTES // word
    g = Guarded()
    g.word, g.sentinel, g.front, g.n, g.row, g.cap, g.dtype, g.offset = word, SENTINEL[word], front, n, row, cap, dtype, offset_elems
    if isinstance(lib_or_dev, str) and lib_or_dev == "numpy":
        raw = np.full(total + 16 // word, g.sentinel, dtype=_WORD_TYPES[word])
        shift = (-raw.ctypes.data % 16) // word
        g.words = raw[shift:shift + total]
        assert g.words.ctypes.data % 16 == 0
        g.interior = g.words[front:front + n * row].view(np_type).reshape(tuple(shape))
        g.ptr = g.words.ctypes.data + front * word
        assert n * row == 0 or g.interior.ctypes.data == g.ptr
    else:
        import torch
        dev = lib_or_dev if isinstance(lib_or_dev, torch.device) else torch.device("cpu") if is_emu(lib_or_dev) else torch.device("cuda", 0)
        wt = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[word]
        raw = torch.full((total + 16 // word,), g.sentinel, dtype=wt, device=dev)
        shift = (-raw.data_ptr() % 16) // word
        g.words = raw[shift:shift + total]
        assert g.words.data_ptr() % 16 == 0
        tt = {"float32": torch.float32, "int32": torch.int32, "bfloat16": torch.bfloat16, "bool": torch.uint8}[dtype]
        g.interior = g.words[front:front + n * row].view(tt).view(tuple(shape))
        g.ptr = g.words.data_ptr() + front * word      # (a zero-row view of torch's or NumPy's does not keep its address: the calls take this)
        assert g.interior.is_contiguous() and (n * row == 0 or g.interior.data_ptr() == g.ptr)
    return g


def _guard_words(g):
    """the whole allocation on the host, as unsigned integer words"""
    w = g.words if isinstance(g.words, np.ndarray) else g.words.cpu().numpy()
    return w.view(_WORD_TYPES[g.word])


def assert_guards_intact(g, tag):
    """both guards and the rows past n still hold the sentinel -- compared as integer words"""
    w = _guard_words(g)
    end = g.front + g.n * g.row
    bad = np.flatnonzero(w != g.sentinel)
    bad = bad[(bad < g.front) | (bad >= end)]
    assert bad.size == 0, ("%s: %d words outside the %d x %d-word interior (offset %d elements, %d rows of capacity) were written: first %+d, last %+d "
                           "words from the interior's end (0 is the first word behind it; below %d: in front of the buffer), first value 0x%X"
                           % (tag, bad.size, g.n, g.row, g.offset, g.cap, bad[0] - end, bad[-1] - end, -g.n * g.row, int(w[bad[0]])))


def assert_interior(g, want, tag):
    """the interior, bit for bit `want` (an array of the oracle's: it must not hold the sentinel itself, so that a word still holding it was
    never written) -- compared as integer words"""
    got = _guard_words(g)[g.front:g.front + g.n * g.row]
    ww = np.ascontiguousarray(want).reshape(-1).view(_WORD_TYPES[g.word])
    assert ww.size == got.size, "%s: the oracle has %d words, the buffer %d" % (tag, ww.size, got.size)
    assert not bool((ww == g.sentinel).any()), "%s: the oracle's output holds the sentinel word" % tag
    bad = np.flatnonzero(got != ww)
    assert bad.size == 0, ("%s: %d of %d interior words differ from the oracle's, %d of them were never written (sentinel); first at word %d (row %d): "
                           "0x%X, oracle 0x%X; last at word %d" % (tag, bad.size, got.size, int((got[bad] == g.sentinel).sum()), bad[0], bad[0] // max(g.row, 1),
                                                                   int(got[bad[0]]), int(ww[bad[0]]), bad[-1]))


def assert_all_written(g, tag):
    """no word of the interior still holds the sentinel (outputs without a host getter of the oracle's to compare with)"""
    got = _guard_words(g)[g.front:g.front + g.n * g.row]
    left = np.flatnonzero(got == g.sentinel)
    assert left.size == 0, "%s: %d of %d interior words were never written, first at word %d" % (tag, left.size, got.size, left[0])


BUFFER_BATTLE_PAIRS = [(1, 2), (63, 65), (64, 257), (255, 256), (509, 3)]
BUFFER_BATTLES = ["battle_%d_%d" % p for p in BUFFER_BATTLE_PAIRS]
BUFFER_SHAPES = ["gather", "pursuit_dense", "quad", "battle_turn", "bodies", "arrange", "arrange_turn", "arrange_two_turn", "battle_empty_side"]
# (view offset, feature offset) in floats: both 16-byte aligned (the vector path and its tail), both not (the scalar path), one of each (the
# stand-alone k_features launch)
BUFFER_OFFSETS = [(0, 0), (4, 4), (1, 1), (2, 2), (3, 3), (0, 1), (1, 0)]
# bf16 cells: the view 16-byte aligned always (the engine refuses another with fatal()); the feature pointer is free -- Env::prepare_render
# compares the two alignments and Env::observe_device sends a feature pointer of another alignment to the stand-alone launch
BUFFER_OFFSETS_BF16 = [(0, 0), (8, 4), (0, 1), (8, 3)]


def buffer_worlds():
    """the worlds of tests/test_engine_buffers.py, three steps each: battle 45 x 45 at group sizes around the render kernels' edges (a wave's 64
    cells, a workgroup's 256 threads, odd n -- n x 1183 floats is then no multiple of 4 --, the smallest world; hp 4 / damage 3 so that
    clear_dead shrinks the dense ones), one world per shape launch_render tells apart (scenarios(): gather -- two windows, 7 channels;
    pursuit_dense -- 5 channels, no minimap; quad -- unpacked view cells, 13 channels; battle_turn -- the packed TURN forms; bodies -- three
    groups of multi-cell bodies; arrange -- two groups with a can_absorb type: unpacked cells AND 7 channels, the only way to
    k_render_cells16<PACKED = false>; arrange_turn -- three such groups under turn_mode: k_render<PACKED = false, TURN = true>;
    arrange_two_turn -- arrange's two groups under turn_mode: k_render_cells16<false, true>), a world whose second group is empty, and battle60
    (2400 agents: beyond the two-launch cycle)"""
    import copy
    rnd = lambda g, n: (g, "random", {"n": n})
    W = {}
    for a, b in BUFFER_BATTLE_PAIRS:
        W["battle_%d_%d" % (a, b)] = Scenario("battle_%d_%d" % (a, b), "battle", 45, seed=700 + a, place=[rnd(0, a), rnd(1, b)], steps=3,
                                              action_seed=7 * a + b, over={"small": {"hp": 4, "damage": 3}})
    for name in ("gather", "pursuit_dense", "quad", "battle_turn", "bodies", "arrange", "arrange_turn", "battle60"):
        W[name] = copy.copy(scenarios()[name])
        W[name].steps, W[name].events = 3, {}
    W["arrange_two_turn"] = Scenario("arrange_two_turn", ("arrange", 40, False), 0, place=[rnd(0, 180), rnd(1, 300)], walls=60, acting=[1], steps=3,
                                     action_seed=79, settings={"turn_mode": True})
    W["battle_empty_side"] = Scenario("battle_empty_side", "battle", 12, seed=77, place=[rnd(0, 40)], steps=3, action_seed=78)
    return W


def tune_settings():
    """this process's MAGENT_TUNE as a dict of ints"""
    return {k: int(v) for k, v in (e.split("=") for e in os.environ.get("MAGENT_TUNE", "").split(",") if e)}


def play_buffer_world(sc, lib, clear_last=True):
    """`sc` on library `lib`, played for its steps with the scenario's random actions through the host calls, clear_dead behind every step (behind
    the last one only with clear_last).  Returns the environment, its handles, the group sizes at the start and the action generator."""
    env, handles = sc.build(lib)
    n0 = [env.get_num(h) for h in handles]
    rs = np.random.RandomState(sc.action_seed)
    acting = sc.acting if sc.acting is not None else list(range(len(handles)))
    for step in range(sc.steps):
        for g, h in enumerate(handles):
            if g in acting:
                env.set_action(h, sc.draw(rs, env, g, h, env.get_num(h)))
        env.step()
        if clear_last or step + 1 < sc.steps:
            env.clear_dead()
    return env, handles, n0, rs


_BUFFER_WANT = {}


def buffer_expectations(name):
    """what the oracle returns for buffer world `name` through the plain host calls (computed once per process, never changed):
    "n0" the sizes at the start (capacity of the guarded buffers: n0 + 1 rows); "pre": behind the third step, the dead still there -- reward, id,
    alive, pos per group; "post": behind its clear_dead -- view, feat, reward, id, alive, pos, view2attack per group, mean_info of the acting
    non-empty ones, the 5 x 6 global minimap; "acts" / "cycle_reward": the fourth step's actions and the rewards behind it (what
    env_cycle_many hands out for the observations of "post")"""
    if name in _BUFFER_WANT:
        return _BUFFER_WANT[name]
    sc = buffer_worlds()[name]
    env, hs, n0, rs = play_buffer_world(sc, ensure_oracle(), clear_last=False)
    acting = sc.acting if sc.acting is not None else list(range(len(hs)))
    state = lambda h: {"reward": np.array(env.get_reward(h), dtype=np.float32), "id": env.get_agent_id(h).copy(), "alive": env.get_alive(h).astype(np.uint8),
                       "pos": env.get_pos(h).copy(), "n": env.get_num(h)}
    want = {"n0": n0, "pre": [state(h) for h in hs], "acting": acting}
    for g, h in enumerate(hs):         # (the dead still in the arrays: what the hp getter's rows of the living are compared with)
        if want["pre"][g]["n"] > 0:
            want["pre"][g]["view"] = env.get_observation(h)[0].copy()
    env.clear_dead()
    want["post"] = [state(h) for h in hs]
    for g, h in enumerate(hs):
        p = want["post"][g]
        if p["n"] > 0:
            v, f = env.get_observation(h)
            p["view"], p["feat"] = v.copy(), f.copy()
            if g in acting:
                p["mean_info"] = env.get_mean_info(h).copy()
        else:
            p["view"] = np.zeros((0,) + env.get_view_space(h), dtype=np.float32)
            p["feat"] = np.zeros((0,) + env.get_feature_space(h), dtype=np.float32)
        p["view2attack"] = env.get_view2attack(h)[1].copy()
    want["global_minimap"] = env.get_global_minimap(5, 6).copy()
    want["acts"] = [sc.draw(rs, env, g, h, env.get_num(h)) if g in acting else None for g, h in enumerate(hs)]
    for g, h in enumerate(hs):
        if want["acts"][g] is not None:
            env.set_action(h, want["acts"][g])
    want["cycle_done"] = env.step()
    want["cycle_reward"] = [np.array(env.get_reward(h), dtype=np.float32) for h in hs]
    env.clear_dead()
    want["cycle_n"] = [env.get_num(h) for h in hs]
    _BUFFER_WANT[name] = want
    return want


def bf16_cells(view):
    """the bf16-cell form of a float32 view [n, H, W, C <= 7] as uint16 [n, H, W, 8]: the channels rounded to nearest even on the bits (a NaN
    keeps its sign and the upper half of its payload, quiet: the IEEE conversion -- the engine's 0xFFC00000 of an empty group's minimap becomes
    0xFFC0; torch's own conversions disagree with each other on NaNs), zeros up to channel 6, 1.0 in channel 7 (include/magent_policy.h)"""
    C = view.shape[-1]
    out = np.zeros(view.shape[:-1] + (8,), dtype=np.uint16)
    if view.size:
        u = np.ascontiguousarray(view).view(np.uint32).astype(np.uint64)
        rne = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
        out[..., :C] = np.where((u & 0x7FFFFFFF) > 0x7F800000, (u >> 16) | 0x40, rne).astype(np.uint16)
    out[..., 7] = 0x3F80
    return out


def expected_render_kernel(sc, env, handles, g, n, aligned, cells16):
    """launch_render (render.hip) restated: the kernel engine_stats()[6] must name for a render of group g -- 0 k_render / k_render_cells16,
    1 k_render_fast, 4 k_render_sweep2 -- under this process's MAGENT_TUNE.  A second copy of the dispatch, to be kept in step with
    render.hip: render_fast_ok (its render_fast_lds(VHW) <= 48 KiB term holds for every window of these worlds and is left out), sweep5_ok
    and the `mode` selection in launch_render"""
    cfg = sc.config()
    turn, food, minimap = (bool(cfg.config_dict.get(k)) for k in ("turn_mode", "food_mode", "minimap_mode"))
    H, W, C = env.get_view_space(handles[g])
    packed = len(handles) <= 3 and not any(t.get("can_absorb") for t in cfg.agent_type_dict.values())
    shape = aligned and len(handles) == 2 and not food and not turn and packed and 16 <= H * W <= 1024
    fast_ok = shape and minimap and C == 7
    sweep5_ok = shape and not minimap and C == 5 and not cells16
    if not (fast_ok or sweep5_ok):
        return 0
    mode = tune_settings().get("render", -1)
    if mode < 0:
        mode = 1 if cells16 else 4 if (n * H * W + 63) // 64 >= 256 * 4 * 2 * 8 else 0
    return 4 if mode == 4 else 1 if mode == 1 and fast_ok else 0


def check_observation_buffers(lib, name, offsets=None, offsets_bf16=None):
    """env_get_observation_device and ..._bf16 of buffer world `name` on library `lib` into guarded views and feature rows at every offset
    pair: interior == the oracle's bits, guards and the rows past n untouched; which render kernel ran and whether the feature rows took a
    launch of their own is asserted from the engine's own counters.  Returns the set of (kernel, cells16) pairs seen."""
    sc, want = buffer_worlds()[name], buffer_expectations(name)
    env, hs, n0, _ = play_buffer_world(sc, lib)
    dev = torch_device(env, lib)
    env.profile_enable(1)
    seen = set()
    for g, h in enumerate(hs):
        n, p = env.get_num(h), want["post"][g]
        assert n == p["n"], (name, g, n, p["n"])
        vs, fs, cap = env.get_view_space(h), env.get_feature_space(h), n0[g] + 1
        forms = [(False, vo, fo) for vo, fo in (BUFFER_OFFSETS if offsets is None else offsets)]
        if vs[2] <= 7:        # (the wrapper refuses bf16 cells for more channels; the engine would abort)
            forms += [(True, vo, fo) for vo, fo in (BUFFER_OFFSETS_BF16 if offsets_bf16 is None else offsets_bf16)]
        for cells16, vo, fo in forms:
            tag = "%s group %d (n %d) %s view+%d feat+%d" % (name, g, n, "bf16 cells" if cells16 else "float32", vo, fo)
            gv = guarded((n,) + vs[:2] + (8,), "bfloat16", dev, vo, cap) if cells16 else guarded((n,) + vs, "float32", dev, vo, cap)
            gf = guarded((n,) + fs, "float32", dev, fo, cap)
            v_aligned, f_aligned = gv.ptr % 16 == 0, gf.ptr % 16 == 0
            assert v_aligned == (vo * gv.word % 16 == 0) and f_aligned == (fo % 4 == 0) and (v_aligned or not cells16), tag
            device_sync(lib)
            env.profile_read("render"), env.profile_read("features")
            (env._lib.env_get_observation_device_bf16 if cells16 else env._lib.env_get_observation_device)(env.game, g, (ctypes.c_void_p * 2)(gv.ptr, gf.ptr))
            env.sync()
            assert_interior(gv, bf16_cells(p["view"]) if cells16 else p["view"], tag + " view")
            assert_guards_intact(gv, tag + " view")
            assert_interior(gf, p["feat"], tag + " feat")
            assert_guards_intact(gf, tag + " feat")
            renders, own_features = env.profile_read("render")[0], env.profile_read("features")[0]
            if n == 0:
                assert renders == 0 and own_features == 0, tag
                continue
            kernel = env.engine_stats()[6]
            assert kernel == expected_render_kernel(sc, env, hs, g, n, v_aligned, cells16), (tag, "render kernel", kernel)
            assert renders == 1 and own_features == (1 if v_aligned != f_aligned else 0), (tag, renders, own_features)
            seen.add((kernel, cells16))
    return seen


def check_getter_buffers(lib, name):
    """env_get_reward_device and env_get_info_device (every name Env::info_device takes: id, hp, pos, alive) of buffer world `name` into
    guarded buffers, behind the third step with the dead still in the arrays and again behind clear_dead, against the oracle's host getters.
    The oracle has no getter for hp: every byte must have been written, and where every agent is one cell and nobody turns the window's
    centre cell of the oracle's observation, hp / type hp, must be the float32 quotient of what was written -- in both phases, for every agent
    that is alive."""
    sc, want = buffer_worlds()[name], buffer_expectations(name)
    env, hs, n0, _ = play_buffer_world(sc, lib, clear_last=False)
    dev = torch_device(env, lib)
    cfg = sc.config()
    for phase in ("pre", "post"):
        if phase == "post":
            env.clear_dead()
        for g, h in enumerate(hs):
            n, p, cap = env.get_num(h), want[phase][g], n0[g] + 1
            assert n == p["n"], (name, phase, g, n, p["n"])
            tag = "%s %s group %d (n %d)" % (name, phase, g, n)
            for off in (0, 1):
                bufs = {"reward": guarded((n,), "float32", dev, off, cap), "id": guarded((n,), "int32", dev, off, cap),
                        "hp": guarded((n,), "float32", dev, off, cap), "pos": guarded((n, 2), "int32", dev, 2 * off, cap),
                        "alive": guarded((n,), "bool", dev, off, cap)}
                device_sync(lib)
                env._lib.env_get_reward_device(env.game, g, ctypes.c_void_p(bufs["reward"].ptr))
                for key in ("id", "hp", "pos", "alive"):
                    env._lib.env_get_info_device(env.game, g, key.encode(), ctypes.c_void_p(bufs[key].ptr))
                env.sync()
                for key, b in bufs.items():
                    if key == "hp":
                        assert_all_written(b, "%s hp+%d" % (tag, off))
                    else:
                        assert_interior(b, p[key], "%s %s+%d" % (tag, key, off))
                    assert_guards_intact(b, "%s %s+%d" % (tag, key, off))
                t = cfg.agent_type_dict[cfg.groups[g]]
                if n > 0 and t.get("width") == t.get("length") == 1 and "hp" in t and not cfg.config_dict.get("turn_mode") and isinstance(t.get("view_range"), gw.CircleRange):
                    hp = _guard_words(bufs["hp"])[bufs["hp"].front:bufs["hp"].front + n].view(np.float32)
                    vh, vw = p["view"].shape[1:3]
                    own = 1 + (1 if cfg.config_dict.get("food_mode") else 0) + 1      # [wall | (food) | own has, own hp ...]
                    ratio = (hp / np.float32(t["hp"])).astype(np.float32)
                    live = p["alive"].astype(bool)                                    # (a dead agent has left its cell)
                    assert ratio[live].view(np.uint32).tobytes() == np.ascontiguousarray(p["view"][live, vh // 2, vw // 2, own]).view(np.uint32).tobytes(), tag + " hp"


def check_cycle_buffers(lib, names, leave_out=None):
    """one env_cycle_many call (EnvBatch.cycle) over buffer worlds `names` behind their three steps, with caller-owned views, feature rows and
    rewards under guard (float offset 0: the batched forms take 16-byte aligned buffers only): the observations of "post" and the rewards behind
    the fourth step, bit for bit the oracle's; guards and rows past n untouched.  leave_out: a group whose view / feat / reward entries are
    NULL (it still acts).  Which form the call took -- the two-launch cycle, the call sequence, the batched pipeline, its sweeping render, a
    world's own render launches -- is asserted from the engine's counters under this process's MAGENT_TUNE."""
    import torch
    tune = tune_settings()
    worlds = [(buffer_worlds()[nm], buffer_expectations(nm)) + play_buffer_world(buffer_worlds()[nm], lib) for nm in names]
    envs = [w[2] for w in worlds]
    dev = torch_device(envs[0], lib)
    batch = magent_amd.EnvBatch(envs, n_threads=1)
    batch.order_streams = not is_emu(lib)
    views, feats, acts, rews, keep = [], [], [], [], []
    for sc, want, env, hs, n0, _ in worlds:
        nums = [env.get_num(h) for h in hs]
        assert nums == [p["n"] for p in want["post"]], (sc.name, nums)
        seen = [g != leave_out for g in range(len(hs))]
        views.append([guarded((nums[g],) + env.get_view_space(h), "float32", dev, 0, n0[g] + 1) if seen[g] else None for g, h in enumerate(hs)])
        feats.append([guarded((nums[g],) + env.get_feature_space(h), "float32", dev, 0, n0[g] + 1) if seen[g] else None for g, h in enumerate(hs)])
        rews.append([guarded((nums[g],), "float32", dev, 0, n0[g] + 1) if seen[g] else None for g in range(len(hs))])
        acts.append([None if a is None else torch.from_numpy(a).to(dev) for a in want["acts"]])
        env.profile_enable(1)
        env.profile_read("render")
        keep.append(nums)
    device_sync(lib)
    def inner(rows):      # (EnvBatch.pointers, from the guarded buffers' own addresses)
        arr = (ctypes.c_void_p * (len(envs) * batch.n_group))()
        for e, row in enumerate(rows):
            for g, b in enumerate(row):
                arr[e * batch.n_group + g] = None if b is None else b.ptr
        return arr
    dones = batch.cycle(inner(views), inner(feats), acts, inner(rews))
    out = []
    for k, (sc, want, env, hs, n0, _) in enumerate(worlds):
        env.sync()
        assert bool(dones[k]) == bool(want["cycle_done"]) and [env.get_num(h) for h in hs] == want["cycle_n"], sc.name
        for g in range(len(hs)):
            if views[k][g] is None:
                continue
            tag = "%s group %d (n %d) env_cycle_many of %d%s" % (sc.name, g, keep[k][g], len(names), "" if leave_out is None else ", group %d left out" % leave_out)
            for b, w, what in ((views[k][g], want["post"][g]["view"], "view"), (feats[k][g], want["post"][g]["feat"], "feat"), (rews[k][g], want["cycle_reward"][g], "reward")):
                assert_interior(b, w, tag + " " + what)
                assert_guards_intact(b, tag + " " + what)
        renders, piped, swept = env.profile_read("render")[0], env.pipeline_stats()[6], env.pipeline_stats()[7]
        observed = sum(1 for g in range(len(hs)) if views[k][g] is not None and keep[k][g] > 0)
        cells = max([keep[k][g] * int(np.prod(env.get_view_space(h)[:2])) for g, h in enumerate(hs) if views[k][g] is not None] + [0])
        out.append((sc.name, renders, piped, swept))
        if sc.name not in BUFFER_BATTLES + ["battle60"]:      # (the plain two-group worlds: their forms are restated here)
            continue
        # (Env::cycle_many: the pipeline takes a plain world that cannot step in one launch, or one of batch_pipe_min agents or more)
        in_pipe = len(names) >= 2 and (tune.get("batch_pipe_min", 1537) <= sum(keep[k]) or tune.get("solo_step", 1) == 0)
        assert piped == (1 if in_pipe else 0), (sc.name, "batched pipeline", out)
        if in_pipe:         # a world of a group of pipe_own x 65536 window cells renders by launches of its own, the others in the batch's launch
            own = cells >= 65536 * tune.get("pipe_own", 48)
            assert renders == (observed if own else 0) and swept == (1 if tune.get("pipe_sweep", -1) != 0 and not own else 0), (sc.name, "pipeline render", out)
        elif len(names) == 1:
            two_launch = tune.get("solo_step", 1) != 0 and sum(keep[k]) <= 1536
            assert renders == (1 if two_launch else observed), (sc.name, "two-launch cycle" if two_launch else "call sequence", out)
            if not two_launch and sum(keep[k]) > 0:
                assert (env.engine_stats()[7] > 0) == (sum(keep[k]) > 1536 or tune.get("solo_step", 1) == 0), (sc.name, "plain pipeline", env.engine_stats())
    return out


def check_host_abi_buffers(lib, name):
    """the host ABI of library `lib` (reached through the wrapper's own handle) with NumPy interiors carved from guarded arrays: env_get_observation,
    env_get_reward, env_get_info for id, alive, pos, mean_info, view2attack and a 5 x 6 global_minimap -- the device-to-host copies have sizes of
    their own"""
    sc, want = buffer_worlds()[name], buffer_expectations(name)
    env, hs, n0, _ = play_buffer_world(sc, lib)
    L = env._lib
    ptr = lambda b: ctypes.c_void_p(b.ptr)
    for g, h in enumerate(hs):
        n, p, cap = env.get_num(h), want["post"][g], n0[g] + 1
        assert n == p["n"], (name, g, n, p["n"])
        for off in (0, 1):
            tag = "%s group %d (n %d) host ABI +%d" % (name, g, n, off)
            gv = guarded((n,) + env.get_view_space(h), "float32", "numpy", off, cap)
            gf = guarded((n,) + env.get_feature_space(h), "float32", "numpy", off, cap)
            L.env_get_observation(env.game, g, (ctypes.c_void_p * 2)(ptr(gv), ptr(gf)))
            gr = guarded((n,), "float32", "numpy", off, cap)
            L.env_get_reward(env.game, g, ptr(gr))
            checks = [(gv, p["view"], "view"), (gf, p["feat"], "feat"), (gr, p["reward"], "reward")]
            for key, shape, dtype in (("id", (n,), "int32"), ("alive", (n,), "bool"), ("pos", (n, 2), "int32")):
                b = guarded(shape, dtype, "numpy", off * (2 if key == "pos" else 1), cap)
                L.env_get_info(env.game, g, key.encode(), ptr(b))
                checks.append((b, p[key], key))
            b = guarded(p["view2attack"].shape, "int32", "numpy", off)
            L.env_get_info(env.game, g, b"view2attack", ptr(b))
            checks.append((b, p["view2attack"], "view2attack"))
            if "mean_info" in p:
                b = guarded(p["mean_info"].shape, "float32", "numpy", off)
                L.env_get_info(env.game, g, b"mean_info", ptr(b))
                checks.append((b, p["mean_info"], "mean_info"))
            for b, w, what in checks:
                assert_interior(b, w, tag + " " + what)
                assert_guards_intact(b, tag + " " + what)
    for off in (0, 3):
        b = guarded((5, 6, len(hs)), "float32", "numpy", off)
        b.interior.reshape(-1)[:2] = 5, 6          # (the in-params travel in the out-buffer's first two floats, GridWorld.cc:741-742)
        L.env_get_info(env.game, -1, b"global_minimap", ptr(b))
        assert_interior(b, want["global_minimap"], "%s host ABI global_minimap 5 x 6 +%d" % (name, off))
        assert_guards_intact(b, "%s host ABI global_minimap 5 x 6 +%d" % (name, off))


def check_engine_buffer_forms(lib):
    """what a child process of tests/test_engine_buffers.py runs under its MAGENT_TUNE (read once per process): the battle pairs, gather and
    pursuit_dense through the observation check (aligned at two offsets, one unaligned pair, the stand-alone feature launch; bf16 cells) and the
    cycle check alone, then three battle worlds in one EnvBatch -- the checks assert which kernel and which form ran.  Returns what ran."""
    ran = {"renders": set(), "cycles": []}
    for name in BUFFER_BATTLES + ["gather", "pursuit_dense"]:
        ran["renders"] |= check_observation_buffers(lib, name, offsets=[(0, 0), (4, 4), (3, 3), (0, 1)], offsets_bf16=[(0, 0), (8, 1)])
        ran["cycles"] += check_cycle_buffers(lib, [name])
    ran["cycles"] += check_cycle_buffers(lib, ["battle_63_65", "battle_509_3", "battle_255_256"])
    tune = tune_settings()
    if "render" in tune:
        assert (tune["render"] if tune["render"] in (1, 4) else 0, False) in ran["renders"], ran
    ran["renders"] = sorted(ran["renders"])
    return ran


# ---------------------------------------------------------------------------------------------------- the DQN in float64
def qnet_tf_params(qnet):
    """a dueling conv _QNet's parameters in TensorFlow's layout (tf_model/dqn.py:151-189), float64: conv kernels HWIO, dense kernels
    [in, out] (torch keeps OIHW and [out, in])"""
    sd = {k: v.detach().cpu().double().numpy() for k, v in qnet.state_dict().items()}
    return {"conv1/kernel": sd["conv1.weight"].transpose(2, 3, 1, 0), "conv1/bias": sd["conv1.bias"],
            "conv2/kernel": sd["conv2.weight"].transpose(2, 3, 1, 0), "conv2/bias": sd["conv2.bias"],
            "dense_view/kernel": sd["dense_view.weight"].T, "dense_view/bias": sd["dense_view.bias"],
            "dense_emb/kernel": sd["dense_emb.weight"].T, "dense_emb/bias": sd["dense_emb.bias"],
            "value/kernel": sd["value.weight"].T, "value/bias": sd["value.bias"],
            "advantage/kernel": sd["advantage.weight"].T}


def round_bf16(a):
    """a rounded to bfloat16 (nearest even; a NaN stays a NaN), returned as float64"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.bfloat16).double().numpy()


def np_qnet(params, view, feature, use_dueling=True, dtype=np.float64, magnitude=False, bf16=False):
    """NumPy restatement of the reference network (tf_model/dqn.py:151-189): conv3x3(32) -> conv3x3(32), both VALID, NHWC, relu ->
    flatten (h, w, c order) -> dense 256 relu || dense 256 relu on the features -> concat -> dueling head (value + advantage(no bias) -
    mean advantage).  `params` in TensorFlow's layout (qnet_tf_params).

    Computed in `dtype` throughout.  relu is np.maximum(x, 0), which keeps a NaN a NaN, as torch.relu does.
    magnitude=True: the same network on |weights|, |biases| and |inputs|, with the dueling head's value + adv - mean(adv) taken as a sum
      of magnitudes -- per entry the scale that float rounding errors of the real network are bounded by (see f32_error_bound).
    bf16=True: rounded to bfloat16 where policy.hip's kernels round (inputs, weights, conv1's bias -- it rides in the MFMA as a weight --
      and the activations between layers); the other biases and every sum stay in `dtype`."""
    mag = np.abs if magnitude else (lambda a: a)
    rnd = round_bf16 if bf16 else (lambda a: a)
    relu = (lambda a: a) if magnitude else (lambda a: np.maximum(a, 0))
    P = {k: mag(np.asarray(v, dtype=np.float64)).astype(dtype) for k, v in params.items()}
    for k in ("conv1/kernel", "conv1/bias", "conv2/kernel", "dense_view/kernel", "dense_emb/kernel", "value/kernel", "advantage/kernel"):
        P[k] = rnd(P[k]).astype(dtype)

    def conv_valid(x, k, b):                       # x [N,H,W,C], k [3,3,C,O]
        n, h, w, c = x.shape
        out = np.zeros((n, h - 2, w - 2, k.shape[3]), dtype=dtype)
        for dy in range(3):
            for dx in range(3):
                out += np.tensordot(x[:, dy:dy + h - 2, dx:dx + w - 2, :], k[dy, dx], axes=([3], [0])).astype(dtype)
        return rnd(relu(out + b)).astype(dtype)
    x = rnd(mag(np.asarray(view, dtype=np.float64))).astype(dtype)
    f = rnd(mag(np.asarray(feature, dtype=np.float64))).astype(dtype)
    h1 = conv_valid(x, P["conv1/kernel"], P["conv1/bias"])
    h2 = conv_valid(h1, P["conv2/kernel"], P["conv2/bias"])
    flat = h2.reshape(h2.shape[0], -1)
    h_view = rnd(relu(flat @ P["dense_view/kernel"] + P["dense_view/bias"]))
    h_emb = rnd(relu(f @ P["dense_emb/kernel"] + P["dense_emb/bias"]))
    dense = np.concatenate([h_view, h_emb], axis=1).astype(dtype)
    value = dense @ P["value/kernel"] + P["value/bias"]
    if not use_dueling:
        return value
    adv = dense @ P["advantage/kernel"]
    if magnitude:
        return value + adv + adv.mean(axis=1, keepdims=True)
    return value + adv - adv.mean(axis=1, keepdims=True)


def qnet_f64(qnet, view, feature, bf16=False):
    """(Q, Qmag) of a _QNet on torch / NumPy inputs, float64 (np_qnet)"""
    p = qnet_tf_params(qnet)
    v = view.detach().cpu().double().numpy() if hasattr(view, "detach") else np.asarray(view, np.float64)
    f = feature.detach().cpu().double().numpy() if hasattr(feature, "detach") else np.asarray(feature, np.float64)
    return np_qnet(p, v, f, bf16=bf16), np_qnet(p, v, f, magnitude=True, bf16=bf16)


def f32_error_bound(view_space, feat, n_action):
    """c of the per-entry bound |Q_f32 - Q_64| <= c * 2^-24 * Qmag of a float32 evaluation of the network, in any summation order.

    A float32 dot product of length K with a bias is within gamma_(K+1) ~ (K + 1) u of the exact one, relative to the same sum of
    MAGNITUDES (u = 2^-24, Higham's bound for any order -- an MFMA chain, a blocked GEMM, a Winograd-free convolution).  relu is
    1-Lipschitz and the later layers multiply an earlier layer's error by at most their |weights|, so each layer's error reaches Q
    within (K_l + 1) u Qmag, Qmag = the network on |weights|, |biases|, |inputs| (np_qnet magnitude=True).  The layers' reduction
    lengths: conv1 9 x 8 (the kernels pad the channels to 8), conv2 9 x 32, dense_view H2 x W2 x 32 (up to 15 x 15 x 32 = 7200 in the
    supported region), dense_emb FK = feat rounded up to 8, the head 512; the dueling head adds the value and the mean of n_action
    advantages (a sum of n_action terms, one division, two additions).  The two hidden halves are parallel paths; both are counted."""
    h, w, _ = view_space
    fk = (feat + 7) // 8 * 8
    return (72 + 1) + (288 + 1) + ((h - 4) * (w - 4) * 32 + 1) + (fk + 1) + 512 + (n_action + 4)


# ---------------------------------------------------------------------------------------------------- the DRQN and the A2C networks in float64
def _sd64(module):
    return {k: v.detach().cpu().double().numpy() for k, v in module.state_dict().items()}


def rqnet_tf_params(qnet):
    """a _RecurrentQNet's parameters in TensorFlow's layout (tf_model/drqn.py:140-187), float64.  The trunk as qnet_tf_params.  The GRU as
    tf.contrib.rnn.GRUCell (drqn.py:168) keeps it: `gates/kernel` [x | h stacked on the input axis: 1024][r | u: 1024], `gates/bias` [1024],
    `candidate/kernel` [x | h: 1024][512], `candidate/bias` [512]; torch keeps weight_ih / weight_hh [r | z | n: 1536][512] and two bias
    vectors.  The gates' two biases add up to one; the candidate's recurrent bias b_hn has no counterpart in the reference's cell and is
    kept apart as `candidate/recurrent_bias` (np_rqnet says where each convention adds it).  Heads: `dense_value`, `dense_advantage`
    (no bias) for the dueling network (drqn.py:178-180), `dense` for the plain one (drqn.py:184)."""
    sd, S = _sd64(qnet), qnet.STATE
    wih, whh, bih, bhh = sd["rnn.weight_ih_l0"], sd["rnn.weight_hh_l0"], sd["rnn.bias_ih_l0"], sd["rnn.bias_hh_l0"]
    p = {"conv1/kernel": sd["conv1.weight"].transpose(2, 3, 1, 0), "conv1/bias": sd["conv1.bias"],
         "conv2/kernel": sd["conv2.weight"].transpose(2, 3, 1, 0), "conv2/bias": sd["conv2.bias"],
         "dense_view/kernel": sd["dense_view.weight"].T, "dense_view/bias": sd["dense_view.bias"],
         "dense_emb/kernel": sd["dense_emb.weight"].T, "dense_emb/bias": sd["dense_emb.bias"],
         "gru_cell/gates/kernel": np.concatenate([wih[:2 * S].T, whh[:2 * S].T], axis=0), "gru_cell/gates/bias": bih[:2 * S] + bhh[:2 * S],
         "gru_cell/candidate/kernel": np.concatenate([wih[2 * S:].T, whh[2 * S:].T], axis=0), "gru_cell/candidate/bias": bih[2 * S:],
         "gru_cell/candidate/recurrent_bias": bhh[2 * S:]}
    if qnet.use_dueling:
        p.update({"dense_value/kernel": sd["value.weight"].T, "dense_value/bias": sd["value.bias"], "dense_advantage/kernel": sd["advantage.weight"].T})
    else:
        p.update({"dense/kernel": sd["value.weight"].T, "dense/bias": sd["value.bias"]})
    return p


def np_rqnet(params, view, feature, batch, unroll, state=None, use_dueling=True, reset_after=False, dueling_reads="rnn", dtype=np.float64):
    """NumPy restatement of the reference's recurrent network (tf_model/drqn.py:140-187) -> (Q [batch * unroll][A], state [batch][512]).
    `params` in TensorFlow's layout (rqnet_tf_params); view / feature hold batch * unroll rows, a batch entry's steps one after another
    (drqn.py:170: reshape to [batch, unroll, 512]); `state` None: zeros (drqn.py:171).

    Trunk (drqn.py:153-164): as np_qnet.  GRU (drqn.py:168-174), the two conventions side by side:
      reset_after=False -- tf.contrib.rnn.GRUCell, the reference's cell:  [r | u] = sigmoid([x, h] W_g + b_g);
                           c = tanh([x, r * h] W_c + b_c);  h' = u * h + (1 - u) * c.  (b_c here is candidate/bias + candidate/recurrent_bias:
                           one bias vector, as that cell has; TensorFlow initialises b_g to 1, torch draws it like the weights.)
      reset_after=True  -- torch.nn.GRU (and cuDNN / MIOpen, Keras' reset_after=True): the same gates;
                           c = tanh(x W_cx + b_c + r * (h W_ch + b_rc));  the same h'.
    Head: the plain one reads the GRU's output (drqn.py:184).  The dueling one, as the reference writes it, reads `dense`, the GRU's INPUT
    (drqn.py:178-179): dueling_reads="dense".  dueling_reads="rnn" reads the GRU's output like the plain head (ours does)."""
    P = {k: np.asarray(v, dtype=np.float64).astype(dtype) for k, v in params.items()}
    S = P["gru_cell/candidate/kernel"].shape[1]
    relu = lambda a: np.maximum(a, 0)
    sigmoid = lambda a: 1.0 / (1.0 + np.exp(-a))

    def conv_valid(x, k, b):
        n, h, w, c = x.shape
        out = np.zeros((n, h - 2, w - 2, k.shape[3]), dtype=dtype)
        for dy in range(3):
            for dx in range(3):
                out += np.tensordot(x[:, dy:dy + h - 2, dx:dx + w - 2, :], k[dy, dx], axes=([3], [0])).astype(dtype)
        return relu(out + b)
    x = np.asarray(view, dtype=np.float64).astype(dtype)
    f = np.asarray(feature, dtype=np.float64).astype(dtype)
    h2 = conv_valid(conv_valid(x, P["conv1/kernel"], P["conv1/bias"]), P["conv2/kernel"], P["conv2/bias"])
    flat = h2.reshape(h2.shape[0], -1)
    dense = np.concatenate([relu(flat @ P["dense_view/kernel"] + P["dense_view/bias"]), relu(f @ P["dense_emb/kernel"] + P["dense_emb/bias"])], axis=1)
    seq = dense.reshape(batch, unroll, S)
    h = np.zeros((batch, S), dtype=dtype) if state is None else np.asarray(state, dtype=np.float64).astype(dtype).reshape(batch, S)
    Wg, bg, Wc = P["gru_cell/gates/kernel"], P["gru_cell/gates/bias"], P["gru_cell/candidate/kernel"]
    bc, brc = P["gru_cell/candidate/bias"], P["gru_cell/candidate/recurrent_bias"]
    outs = []
    for t in range(unroll):
        xt = seq[:, t]
        g = sigmoid(np.concatenate([xt, h], axis=1) @ Wg + bg)
        r, u = g[:, :S], g[:, S:]
        if reset_after:
            c = np.tanh(xt @ Wc[:S] + bc + r * (h @ Wc[S:] + brc))
        else:
            c = np.tanh(np.concatenate([xt, r * h], axis=1) @ Wc + (bc + brc))
        h = u * h + (1 - u) * c
        outs.append(h)
    rnn = np.stack(outs, axis=1).reshape(batch * unroll, S)
    if not use_dueling:
        return rnn @ P["dense/kernel"] + P["dense/bias"], h
    top = {"rnn": rnn, "dense": dense}[dueling_reads]
    adv = top @ P["dense_advantage/kernel"]
    return top @ P["dense_value/kernel"] + P["dense_value/bias"] + adv - adv.mean(axis=1, keepdims=True), h


def actor_critic_tf_params(net):
    """an _ActorCritic's parameters in TensorFlow's layout (tf_model/a2c.py:94-161), float64, under the names TensorFlow gives the unnamed
    layers in the order a2c.py creates them: dense (view), dense_1 (feature), dense_2 (512), step_0_C / _H, step_1_C / _H (the CommNet
    block multiplies from the right, a2c.py:102: [in, out]), dense_3 (policy), dense_4 (value)"""
    sd = _sd64(net)
    p = {}
    for tf_name, ours in (("dense", "dense_view"), ("dense_1", "dense_emb"), ("dense_2", "dense"), ("dense_3", "policy"), ("dense_4", "value")):
        p[tf_name + "/kernel"], p[tf_name + "/bias"] = sd[ours + ".weight"].T, sd[ours + ".bias"]
    if net.comm is not None:
        for s in range(2):
            p["step_%d_C" % s], p["step_%d_H" % s] = sd["comm.%d.C.weight" % s].T, sd["comm.%d.H.weight" % s].T
    return p


def np_actor_critic(params, view, feature, use_comm, dtype=np.float64):
    """NumPy restatement of the reference's actor-critic (tf_model/a2c.py:76-162) -> (policy [n][A], value [n]); `params` in TensorFlow's
    layout (actor_critic_tf_params); num_agent = the number of rows, as infer_action and train feed it (a2c.py:213, 282).
    Flattened view -> dense 256 relu || dense 256 relu on the features -> concat -> dense 512 relu (a2c.py:148-154); the CommNet block as
    a2c.py:94-102 writes it: mask = (ones - eye) * (1 / (n - 1) if n > 1 else 0), message = mask @ hidden,
    tanh(message C + hidden H + skip), twice, skip = the dense layer's output both times (a2c.py:120-124); softmax, then
    clip_by_value(1e-10, 1 - 1e-10) (a2c.py:159-160); value = dense 1 on the same hidden units (a2c.py:161-162)."""
    P = {k: np.asarray(v, dtype=np.float64).astype(dtype) for k, v in params.items()}
    relu = lambda a: np.maximum(a, 0)
    n = len(view)
    flat = np.asarray(view, dtype=np.float64).astype(dtype).reshape(n, -1)
    f = np.asarray(feature, dtype=np.float64).astype(dtype)
    dense = np.concatenate([relu(flat @ P["dense/kernel"] + P["dense/bias"]), relu(f @ P["dense_1/kernel"] + P["dense_1/bias"])], axis=1)
    dense = relu(dense @ P["dense_2/kernel"] + P["dense_2/bias"])
    if use_comm:
        mask = (np.ones((n, n), dtype=dtype) - np.eye(n, dtype=dtype)) * dtype(1.0 / (n - 1.0) if n > 1 else 0.0)
        skip, h = dense, dense
        for s in range(2):
            h = np.tanh((mask @ h) @ P["step_%d_C" % s] + h @ P["step_%d_H" % s] + skip)
        dense = h
    logits = dense @ P["dense_3/kernel"] + P["dense_3/bias"]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    policy = np.clip(e / e.sum(axis=1, keepdims=True), dtype(1e-10), dtype(1 - 1e-10))
    return policy, (dense @ P["dense_4/kernel"] + P["dense_4/bias"]).reshape(-1)


# ---------------------------------------------------------------------------------------------------- one training step in float64
def np_q_target(t_q, q, rewards, terminal, gamma, use_double):
    """tf_model/dqn.py:233-248 = drqn.py:247-277: the target network's value of the successor at the online network's greedy action
    (double DQN) or its own maximum; terminal transitions take the reward alone"""
    n = len(rewards)
    nxt = t_q[np.arange(n), np.argmax(q, axis=1)] if use_double else t_q.max(axis=1)
    return np.where(terminal, rewards, rewards + gamma * nxt)


def np_masked_td_loss(target, q, action, mask):
    """dqn.py:105-107 = drqn.py:102-107 -> (loss, dloss/dq): sum(mask * (target - q[i, action_i])^2) / sum(mask)"""
    n = len(target)
    td = target - q[np.arange(n), action]
    grad = np.zeros_like(q)
    grad[np.arange(n), action] = -2.0 * td * mask / mask.sum()
    return float((td ** 2 * mask).sum() / mask.sum()), grad


def np_drqn_window(item_terminal, start, unroll):
    """drqn.py:360-372: the rows of an episode a window takes and its mask -> (real steps, mask [real]): every taken step counts, except
    the last one when the episode goes on behind it (its successor is not in the window)"""
    real = min(len(item_terminal) - start, unroll)
    mask = np.ones(real)
    if not item_terminal[start + real - 1]:
        mask[real - 1] = 0
    return real, mask


def np_discounted_returns(rewards, bootstrap, gamma):
    """a2c.py:257-265: keep = V(last observation); for i from the end: keep = keep * gamma + r[i]"""
    out, keep = np.zeros(len(rewards)), float(bootstrap)
    for i in reversed(range(len(rewards))):
        keep = keep * gamma + float(rewards[i])
        out[i] = keep
    return out


def np_a2c_losses(policy, value, action, returns, value_coef, ent_coef):
    """a2c.py:163-172 -> (pg_loss, vf_loss, neg_entropy) with log(policy + 1e-6); the advantage is a constant of the gradient"""
    n = len(action)
    log_policy = np.log(policy + 1e-6)
    advantage = returns - value
    pg = -np.mean(advantage * log_policy[np.arange(n), action])
    vf = value_coef * np.mean((returns - value) ** 2)
    ent = ent_coef * np.mean((policy * log_policy).sum(axis=1))
    return float(pg), float(vf), float(ent)


def np_clip_by_global_norm(grads, clip):
    """tf.clip_by_global_norm (dqn.py:112, drqn.py:112): every gradient times clip / max(global norm, clip) -> (grads, global norm)"""
    norm = float(np.sqrt(sum(float((g ** 2).sum()) for g in grads)))
    return [g * (clip / max(norm, clip)) for g in grads], norm


class NpAdam(object):
    """Adam (Kingma & Ba, algorithm 1; lr, 0.9, 0.999, 1e-8: the defaults of tf.train.AdamOptimizer and torch.optim.Adam) in float64.
    TensorFlow folds the bias corrections into the step size and so adds its epsilon to sqrt(v), not sqrt(v-hat): at step t that is an
    epsilon of 1e-8 / sqrt(1 - 0.999^t) in this form -- at most 3.2e-7, seen only by gradients that small."""

    def __init__(self, lr, b1=0.9, b2=0.999, eps=1e-8):
        self.lr, self.b1, self.b2, self.eps, self.t, self.m, self.v = lr, b1, b2, eps, 0, None, None

    def update(self, grads):
        """(the steps to ADD to the parameters for these gradients, the same steps with the first moment's two terms taken as magnitudes:
        what a rounding error of the float32 optimiser is relative to where b1 m and (1 - b1) g cancel)"""
        if self.m is None:
            self.m, self.v = [np.zeros_like(g) for g in grads], [np.zeros_like(g) for g in grads]
        self.t += 1
        out, mags = [], []
        for i, g in enumerate(grads):
            mag = self.b1 * np.abs(self.m[i]) + (1 - self.b1) * np.abs(g)
            self.m[i] = self.b1 * self.m[i] + (1 - self.b1) * g
            self.v[i] = self.b2 * self.v[i] + (1 - self.b2) * g * g
            mhat, vhat = self.m[i] / (1 - self.b1 ** self.t), self.v[i] / (1 - self.b2 ** self.t)
            out.append(-self.lr * mhat / (np.sqrt(vhat) + self.eps))
            mags.append(self.lr * mag / (1 - self.b1 ** self.t) / (np.sqrt(vhat) + self.eps))
        return out, mags
