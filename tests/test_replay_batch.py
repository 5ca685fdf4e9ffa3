"""magent_amd.DeviceEpisodesBuffer through the engine: tests/test_batch_ids.py's three battle worlds (hp 4, damage 3: clear_dead bites within
five cycles; one world has no second side) in one EnvBatch with packed buffers.  Per cycle: agent_ids, packed_segments, cycle, record_step
for both sides; then close on the ids after the last cycle.

The oracle is test_replay_kernels.py's numpy restatement fed with host copies of the same packed buffers: packed() is equal on bits.
Besides, a per-world host loop (the ids of get_agent_id, the actions as drawn, the rewards of each world's rows) says what every
(world, id) was given and got, cycle by cycle: every recorded episode holds exactly that.  Then the three models train from the
recorder: the DQN's replay rings equal, bit for bit, those of a twin given the restatement's arrays; the DRQN and the A2C consume every
episode."""
import numpy as np
import pytest
import torch

import helpers as H
import magent_amd
from magent_amd.builtin.torch_model import AdvantageActorCritic, DeepQNetwork, DeepRecurrentQNetwork
from magent_amd.replay import DeviceEpisodesBuffer
from test_batch_ids import lib_of, worlds
from test_replay_kernels import Restated, assert_packed, bits, leg_of

LEGS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
_rounds = {}


def play_round(leg):
    """the round of a leg, played once: (recorders, restatements, per side {(world, id): [(action, reward)]}, envs, handles)"""
    if leg in _rounds:
        return _rounds[leg]
    lib = lib_of(leg)
    scs = worlds()
    built = [sc.build(lib) for sc in scs]
    envs, handles = [b[0] for b in built], [b[1] for b in built]
    dev = H.torch_device(envs[0], lib)
    batch = magent_amd.EnvBatch(envs, n_threads=1)
    batch.order_streams = not H.is_emu(lib)
    off, tot = batch.packed_offsets()
    vs, fs = envs[0].get_view_space(handles[0][0]), envs[0].get_feature_space(handles[0][0])
    NG = 2
    filled = lambda shape, dtype, v: [torch.full((int(tot[g]),) + shape, v, dtype=dtype, device=dev) for g in range(NG)]
    ids, views, feats, acts, rews = filled((), torch.int32, 0), filled(vs, torch.float32, -7.0), filled(fs, torch.float32, -7.0), filled((), torch.int32, 0), filled((), torch.float32, -7.0)
    id_p, view_p, feat_p, act_p, rew_p = (batch.packed_pointers(t, off) for t in (ids, views, feats, acts, rews))
    replay_lib = leg_of(leg)[0]
    recs = [DeviceEpisodesBuffer(512, 2500, vs, fs, device=dev, lib=replay_lib) for g in range(NG)]
    wants = [Restated(512, 2500) for g in range(NG)]
    orders = [torch.from_numpy(np.random.RandomState(31 + g).permutation(int(tot[g])).astype(np.int32)).to(dev) for g in range(NG)]
    rss = [np.random.RandomState(sc.action_seed) for sc in scs]
    told = [{}, {}]
    sync = lambda: (H.device_sync(lib), [env.sync() for env in envs])

    def ids_now():
        sync()
        batch.agent_ids(id_p)
        sync()
        return batch.packed_segments(off), [[np.asarray(env.get_agent_id(h)).copy() for h in hs] for env, hs in zip(envs, handles)]

    for step in range(scs[0].steps):
        segs, host_ids = ids_now()
        drawn = [[sc.draw(rs, env, g, h, env.get_num(h)) for g, h in enumerate(hs)] for sc, rs, env, hs in zip(scs, rss, envs, handles)]
        for e in range(len(envs)):
            for g in range(NG):
                o = int(off[e][g])
                acts[g][o:o + len(drawn[e][g])] = torch.from_numpy(drawn[e][g]).to(dev)
        sync()
        batch.cycle(view_p, feat_p, act_p, rew_p)
        sync()
        for g in range(NG):
            recs[g].record_step(ids[g], (views[g], feats[g]), acts[g], rews[g], segments=segs[g], order=orders[g])
            wants[g].record_step(ids[g].cpu().numpy(), views[g].cpu().numpy(), feats[g].cpu().numpy(), acts[g].cpu().numpy(), rews[g].cpu().numpy(),
                                 segs[g], orders[g].cpu().tolist())
            rew_host = rews[g].cpu().numpy()
            for e in range(len(envs)):                           # the per-world host loop: what (world, id) was given and got
                o = int(off[e][g])
                for i, aid in enumerate(host_ids[e][g].tolist()):
                    told[g].setdefault((e, aid), []).append((int(drawn[e][g][i]), rew_host[o + i]))
    segs, host_ids = ids_now()
    for g in range(NG):
        recs[g].close(ids[g], segs[g])
        wants[g].close(ids[g].cpu().numpy(), segs[g])
    alive = [{(e, aid) for e in range(len(envs)) for aid in host_ids[e][g].tolist()} for g in range(NG)]
    _rounds[leg] = (recs, wants, told, alive, envs, handles, dev)
    return _rounds[leg]


@pytest.mark.parametrize("leg", LEGS)
def test_the_round_equals_the_restatement_and_the_worlds(leg):
    recs, wants, told, alive, envs, handles, dev = play_round(leg)
    for g in range(2):
        got = recs[g].packed()
        assert_packed(got, wants[g].packed(), "%s side %d" % (leg, g))
        buf = recs[g].buffer
        assert set(buf) == set(told[g]), "capacity 512 takes everybody of side %d" % g
        for key, ep in buf.items():
            assert [int(a) for a in ep.actions] == [a for a, _ in told[g][key]], key
            assert np.array_equal(bits(np.asarray(ep.rewards, dtype=np.float32)), bits(np.array([r for _, r in told[g][key]], dtype=np.float32))), key
            assert ep.terminal == (key not in alive[g]), key
        assert any(ep.terminal for ep in buf.values()) and not all(ep.terminal for ep in buf.values())
        assert not (got[0] == -7.0).all(dim=(1, 2, 3)).any()     # (every recorded view row was rendered)
    assert {k[0] for k in recs[0].buffer} == {0, 1, 2} and {k[0] for k in recs[1].buffer} == {0, 1}


class PackedOf(object):
    """the restatement's arrays behind EpisodesBuffer's packed()"""

    def __init__(self, want):
        self.want = want

    def packed(self):
        return self.want.packed()


@pytest.mark.parametrize("leg", LEGS)
def test_dqn_train_fills_the_replay_rings_of_the_restatements_twin(leg):
    recs, wants, told, alive, envs, handles, dev = play_round(leg)
    torch.manual_seed(5)
    models = [DeepQNetwork(envs[0], handles[0][0], "replay%d" % k, batch_size=64, memory_size=300, device=dev) for k in range(2)]
    models[0].train(recs[0])
    models[1].train(PackedOf(wants[0]))
    n = wants[0].transitions
    assert n > 300 and models[0].replay_len == models[1].replay_len == 300      # (the rings wrapped)
    for name in ("mem_view", "mem_feature", "mem_action", "mem_reward", "mem_terminal", "mem_mask"):
        a, b = getattr(models[0], name), getattr(models[1], name)
        assert a.head == b.head and a.buf.dtype == b.buf.dtype
        raw = lambda t: t.buf[:300].cpu().numpy().view(np.uint8)
        assert np.array_equal(raw(a), raw(b)), name


@pytest.mark.parametrize("leg", LEGS)
def test_drqn_and_a2c_train_consume_every_episode(leg, capsys):
    recs, wants, told, alive, envs, handles, dev = play_round(leg)
    torch.manual_seed(6)
    n_eps, n = sum(1 for e in wants[1].episodes if e), wants[1].transitions
    assert n_eps > 100
    drqn = DeepRecurrentQNetwork(envs[0], handles[0][1], "replay_drqn", batch_size=4, unroll_step=2, memory_size=1000, train_freq=0.02, device=dev)
    drqn.train(recs[1])
    assert len(drqn.replay_buffer) == n_eps and sum(len(item[3]) for item in drqn.replay_buffer) == n
    a2c = AdvantageActorCritic(envs[0], handles[0][1], "replay_a2c", device=dev)
    a2c.train(recs[1])
    assert "sample %d " % n in capsys.readouterr().out and a2c.train_ct == 1
