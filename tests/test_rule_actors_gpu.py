"""The rule-based actors' device path on the MI355X (magent_amd/csrc/actors.hip through magent_amd/builtin/rule_model.py).

Every test runs its GPU work in a child process of its own under a time limit (`python tests/test_rule_actors_gpu.py <case>`):
* parity on device observations of pursuit, of config 4's gather 500² (100k agents) and of config 3's battle 1000² at 2 x 400k:
  every runaway action equals the compiled reference's, predator and gatherer actions equal it where nothing was drawn and lie
  in the reference's set where something was (tests/test_rule_actors.py: possible_sets);
* the device draws: the same (seed, counter) gives the same actions, another counter other draws, and a chi-square bound on
  >= 10^5 draws of each draw site kind;
* a closed loop: a 30-step pursuit episode of RushPredator against RunawayPrey that stays on the device (observations, actions,
  env_set_action_device; no host synchronisation between inference and step) against the oracle fed the actors' actions.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]      # (also when run as the child process)
import helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(case, timeout):
    env = H.merge_env(os.environ, {"OMP_NUM_THREADS": "1"})
    p = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0 and ("ok " + case) in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


@pytest.mark.skipif(not H.have_ref(), reason="compiled reference (oracle/_ref) did not travel")
@pytest.mark.parametrize("case,timeout", [("parity_pursuit", 300), ("parity_gather500", 600), ("parity_battle1000", 900)])
def test_device_actions_match_the_reference(case, timeout):
    _run(case, timeout)


def test_device_draws_are_reproducible_and_uniform():
    _run("draws", 300)


def test_closed_loop_pursuit_on_the_device_matches_the_oracle():
    _run("closed_loop", 600)


# ---------------------------------------------------------------------------------------------- the child's cases
def _device_world(game, size, counts, seed, settings=None):
    cfg = H.config_for(game, size)
    if settings:
        cfg.set(settings)
    env = H.gridworld(cfg, lib=H.HIP_LIB, device_obs=True)
    env.set_seed(seed)
    env.reset()
    for h, n in zip(env.get_handles(), counts):
        env.add_agents(h, "random", n=n)
    return env


def _random_steps(env, acting, steps, seed):
    import torch
    rs = np.random.RandomState(seed)
    hs = env.get_handles()
    for _ in range(steps):
        for g in acting:
            a = torch.from_numpy(rs.randint(env.get_action_space(hs[g])[0], size=env.get_num(hs[g])).astype(np.int32)).cuda(env.device_id)
            env.order_after_torch()
            env.set_action_device(hs[g], a)
        env.step()
        env.clear_dead()


def _check_chunked(T, kind, view, feat, act, drew, p, chunk=50000):
    """the device's actions of one call against the compiled reference, `chunk` agents at a time on the host (the feature
    pointer moves by floats, not rows: the threshold test reads the flattened array)"""
    ref = T.reference(kind)
    flat = feat.reshape(-1)
    act, drew = act.cpu().numpy(), drew.cpu().numpy()
    n = view.shape[0]
    counts = np.zeros(2, dtype=np.int64)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        v = view[s:e].cpu().numpy()
        f = flat[s:].cpu().numpy()
        if kind == "gather":
            keep = ~T.gather_divides_by_zero(v, p)
        else:
            keep = np.ones(e - s, dtype=bool)
        idx = np.nonzero(keep)[0]
        v, f_rows = v[idx], f          # (gather reads no feature)
        if kind != "gather":
            assert keep.all()
        want = T.call(ref, kind, v, f_rows, p)
        if kind == "rush":        # every predator, vectorised: drawn exactly where the reference draws
            want_drew = _rush_draws(v, f_rows[:e - s], p)
            assert (drew[s:e].astype(bool) == want_drew).all(), (kind, s)
            exact = ~want_drew
            assert (act[s:e][exact] == want[exact]).all(), (kind, s, np.nonzero(act[s:e] != want)[0][:5])
            assert ((act[s:e][~exact] >= 0) & (act[s:e][~exact] < p["base"])).all()
        else:
            T.check_device_actions(kind, v, f_rows, p, act[s:e][idx], drew[s:e][idx], want, "%s %d" % (kind, s))
        counts += [int((drew[s:e][idx] == 0).sum()), int((drew[s:e][idx] == 1).sum())]
    return counts


def _rush_draws(v, f, p):
    hit = (v[:, :, :, p["channel"]] > 0.5) | (v[:, :, :, 1] > 0.5)
    v2a = np.asarray(p["v2a"])
    att = (hit & (v2a != -1)[None]).any(axis=(1, 2))
    h, w = v.shape[1:3]
    fwd = (v[:, h - 1, w // 2, 0].astype(np.float64) + 0.5).astype(np.int64) != 1
    passed = f < np.float32(p["threshold"])
    return ~passed | (~att & ~(hit.any(axis=(1, 2)) & fwd))


def case_parity_pursuit():
    import test_rule_actors as T
    from magent.builtin.rule_model import RunawayPrey, RushPredator
    env = _device_world("pursuit", 40, (40, 80), seed=5)
    pred, prey = env.get_handles()
    a, b = RushPredator(env, pred, prey, seed=1), RunawayPrey(env, prey, pred, seed=2)
    total = np.zeros(2, dtype=np.int64)
    for t in range(6):
        vp, fp = env.get_observation(pred)
        vq, fq = env.get_observation(prey)
        ap, aq = a.infer_action((vp, fp)), b.infer_action((vq, fq))
        assert ap.is_cuda and ap.dtype.is_floating_point is False and ap.shape == (vp.shape[0],)
        total += _check_chunked(T, "rush", vp, fp, ap, a.last_drew, T.actor_params(env, "rush", pred, prey))
        total += _check_chunked(T, "runaway", vq, fq, aq, b.last_drew, T.actor_params(env, "runaway", prey, pred))
        _random_steps(env, (0, 1), 1, seed=t)
    print("pursuit exact / drawn", total.tolist())


def case_parity_gather500():
    import test_rule_actors as T
    from magent.builtin.rule_model import RushGatherer
    env = _device_world("gather", 500, (20000, 100000), seed=12345)
    food, agent = env.get_handles()
    g = RushGatherer(env, agent, seed=3)
    p = T.actor_params(env, "gather", agent)
    total = np.zeros(2, dtype=np.int64)
    for t in range(2):
        v, f = env.get_observation(agent)
        assert v.shape[0] == 100000 or t > 0
        act = g.infer_action((v, f))
        total += _check_chunked(T, "gather", v, f, act, g.last_drew, p, chunk=20000)
        _random_steps(env, (1,), 3, seed=t)
    assert total[0] > 0 and total[1] > 0, total
    print("gather exact / drawn", total.tolist())


def case_parity_battle1000():
    import test_rule_actors as T
    from magent.builtin.rule_model import RunawayPrey, RushPredator
    env = _device_world("battle", 1000, (400000, 400000), seed=12345)
    g0, g1 = env.get_handles()
    for step in range(2):
        for me, other in ((g0, g1), (g1, g0)):
            v, f = env.get_observation(me)
            assert v.shape == (400000, 13, 13, 7) or step > 0
            a, b = RushPredator(env, me, other, seed=4), RunawayPrey(env, me, other, seed=5)
            ar, ab = a.infer_action((v, f)), b.infer_action((v, f))
            cr = _check_chunked(T, "rush", v, f, ar, a.last_drew, T.actor_params(env, "rush", me, other))
            cb = _check_chunked(T, "runaway", v, f, ab, b.last_drew, T.actor_params(env, "runaway", me, other))
            assert cb[1] == 0
            print("battle step %d group %d: rush exact / drawn %s, runaway %s" % (step, me.value, cr.tolist(), cb.tolist()))
            del v, f
        _random_steps(env, (0, 1), 1, seed=step)


def _device_call(kind, view, feat, p, seed, counter):
    import torch
    from magent_amd import c_lib
    from magent_amd.builtin.rule_model import MagentActorArgs
    import test_rule_actors as T
    lib = c_lib.load(H.HIP_LIB)
    n, h, w, c = view.shape
    act = torch.empty(n, dtype=torch.int32, device=view.device)
    drew = torch.empty(n, dtype=torch.uint8, device=view.device)
    v2a = torch.from_numpy(np.ascontiguousarray(p["v2a"], dtype=np.int32).reshape(-1)).to(view.device)
    args = MagentActorArgs(kind=T.KIND[kind], n=n, height=h, width=w, n_channel=c, attack_base=p["base"], channel=p["channel"],
                           move_back=p["move_back"], threshold=p["threshold"], seed=seed, counter=counter)
    assert lib.actor_infer_action_device(ctypes.byref(args), view.data_ptr(), feat.data_ptr(), v2a.data_ptr(), act.data_ptr(),
                                         drew.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    return act.cpu().numpy(), drew.cpu().numpy()


def _chi2(values, m):
    counts = np.bincount(values, minlength=m)
    assert len(counts) == m
    e = len(values) / m
    return float(((counts - e) ** 2 / e).sum())


def case_draws():
    import torch
    n, h, w, c = 200000, 7, 7, 7
    dev = torch.device("cuda", 0)
    view = torch.zeros((n, h, w, c), dtype=torch.float32, device=dev)
    v2a = -np.ones((h, w), dtype=np.int32)
    v2a[2:5, 2:5] = np.arange(9).reshape(3, 3)
    # every predator over the threshold: one draw in [0, 13) each
    p = {"base": 13, "v2a": v2a, "channel": 3, "move_back": 4, "threshold": 100.0}
    feat = torch.full((n, 3), 1000.0, device=dev)
    a1, d1 = _device_call("rush", view, feat, p, seed=7, counter=0)
    a2, d2 = _device_call("rush", view, feat, p, seed=7, counter=0)
    a3, _ = _device_call("rush", view, feat, p, seed=7, counter=1)
    a4, _ = _device_call("rush", view, feat, p, seed=8, counter=0)
    assert d1.all() and (a1 == a2).all() and (d1 == d2).all()
    assert (a1 != a3).mean() > 0.85 and (a1 != a4).mean() > 0.85, ((a1 != a3).mean(), (a1 != a4).mean())
    x = _chi2(a1, 13)
    assert x < 45.0, x                       # 12 degrees of freedom: p < 1e-5 beyond 45
    # every gatherer sees the same five attackable food cells: the k-th-of-a-set pick
    view[:, 2, 2:5, 4] = 1.0
    view[:, 4, 3:5, 4] = 1.0
    g, dg = _device_call("gather", view, feat, p, seed=9, counter=0)
    assert dg.all()
    want = sorted((v2a[2, 2:5].tolist() + v2a[4, 3:5].tolist()))
    assert sorted(np.unique(g - 13).tolist()) == want, np.unique(g)
    x = _chi2(np.searchsorted(want, g - 13), 5)
    assert x < 30.0, x                       # 4 degrees of freedom: p < 1e-5 beyond 25.5
    # the minimap pick: 11 minimap cells, no food, my position in the middle
    view.zero_()
    view[:, 0, :, 6] = 0.5
    view[:, 6, 0:4, 6] = 2.0
    view[:, 3, 3, 3] = 2.0
    m, dm = _device_call("gather", view, feat, p, seed=10, counter=0)
    assert dm.all()
    # the reference's set: get_action((row - 3, col - 3), stride) -- never 6 here -- uniform over the 11 cells
    cells = [(0, col) for col in range(7)] + [(6, col) for col in range(4)]
    import test_rule_actors as T
    expect = np.bincount([T._get_action(r - 3, cc - 3, True) for r, cc in cells], minlength=13) / len(cells)
    got = np.bincount(m, minlength=13) / n
    assert np.abs(got - expect).max() < 0.01, (got, expect)
    print("draws chi2 ok")


def case_closed_loop():
    import torch
    from magent.builtin.rule_model import RunawayPrey, RushPredator
    cfg = H.config_for("pursuit", 40)
    prod = H.gridworld(cfg, lib=H.HIP_LIB, device_obs=True)
    orac = H.gridworld(cfg, lib=H.ensure_oracle())
    envs = (prod, orac)
    for env in envs:
        env.set_seed(21)
        env.reset()
        for h, n in zip(env.get_handles(), (30, 60)):
            env.add_agents(h, "random", n=n)
    pred, prey = prod.get_handles()
    a, b = RushPredator(prod, pred, prey, seed=1), RunawayPrey(prod, prey, pred, seed=2)
    drawn = 0
    for t in range(30):
        # the device side: observation -> actors -> set_action_device -> step, with no host synchronisation in between
        vp, fp = prod.get_observation(pred)
        vq, fq = prod.get_observation(prey)
        ap, aq = a.infer_action((vp, fp)), b.infer_action((vq, fq))
        prod.order_after_torch()
        prod.set_action_device(pred, ap)
        prod.set_action_device(prey, aq)
        done_p = prod.step()
        # the oracle, fed the actions the actors chose
        acts = (ap.cpu().numpy(), aq.cpu().numpy())
        drawn += int(a.last_drew.sum().item())
        for g, (v, f) in enumerate(((vp, fp), (vq, fq))):
            ov, of = orac.get_observation(orac.get_handles()[g])
            assert np.array_equal(v.cpu().numpy(), ov) and np.array_equal(f.cpu().numpy(), of), ("observation", t, g)
            orac.set_action(orac.get_handles()[g], acts[g])
        done_o = orac.step()
        assert done_p == done_o, t
        for g in range(2):
            hp, ho = prod.get_handles()[g], orac.get_handles()[g]
            assert np.array_equal(prod.get_reward(hp), orac.get_reward(ho)), ("reward", t, g)
            assert np.array_equal(prod.get_alive(hp), orac.get_alive(ho)), ("alive", t, g)
        for env in envs:
            env.clear_dead()
        for g in range(2):
            hp, ho = prod.get_handles()[g], orac.get_handles()[g]
            assert prod.get_num(hp) == orac.get_num(ho), ("num", t, g)
            assert np.array_equal(prod.get_pos(hp), orac.get_pos(ho)), ("pos", t, g)
            assert np.array_equal(prod.get_agent_id(hp), orac.get_agent_id(ho)), ("id", t, g)
        torch.cuda.synchronize()
    print("closed loop: 30 steps equal; predators left %d, prey %d, drawn predator actions %d"
          % (prod.get_num(pred), prod.get_num(prey), drawn))


if __name__ == "__main__":
    sys.path.insert(0, H.ROOT)
    name = sys.argv[1]
    globals()["case_" + name]()
    print("ok " + name)
