"""DeepRecurrentQNetwork over a packed EnvBatch: ONE infer_action(..., ids, segments=table) per side with the ids of EnvBatch.agent_ids,
against one model per world driven plain on that world's rows.

Three 20 x 20 battle worlds of different populations (hp 4, damage 3: side 1 attacks at random and side 0 shrinks) are cycled by one
EnvBatch into packed buffers (EnvBatch.packed_offsets); before every cycle the ids and the (begin, count) table are taken (the rows a cycle's render writes are the population at its start).  The batch model
and the three per-world models share their weights; the per-world models read their world's rows of the same packed observation and
EnvBatch-independent ids (env.get_agent_id taken at the same moment).  On the kernel paths (float32 views; bf16 cells) greedy actions
and states are equal bit for bit per world, and agent_states has the (world, id) keys of the living agents.  The PyTorch path
(MAGENT_POLICY_F32=torch on the GPU; NumPy inputs on the CPU in the GPU-less suite, on made-up observations) is compared within the bound
of test_drqn_device_path_matches_the_torch_path_in_a_battle: states within 2e-5, actions equal except at near-ties of Q."""
import os

import numpy as np
import pytest

import helpers as H
import magent_amd

S = 512
POPULATIONS = [(85, 110), (121, 62), (30, 41)]


def batch_worlds():
    envs = []
    for k, (a, b) in enumerate(POPULATIONS):
        env = magent_amd.GridWorld(H.config_for("battle", 20, small={"hp": 4, "damage": 3}))       # (dense and frail: agents die within a few cycles)
        env.set_seed(300 + k)
        env.reset()
        hs = env.get_handles()
        env.add_agents(hs[0], "random", n=a)
        env.add_agents(hs[1], "random", n=b)
        envs.append(env)
    return envs


def models(env, handle, n, scale=3.0, **kw):
    """n models of one side with the weights of the first: the default init times `scale`"""
    import torch
    from magent_amd.builtin.torch_model import DeepRecurrentQNetwork
    torch.manual_seed(9)
    out = [DeepRecurrentQNetwork(env, handle, "m%d" % k, memory_size=4, **kw) for k in range(n)]
    with torch.no_grad():
        for p in out[0].qnet.parameters():
            p.mul_(scale)             # (3: every layer matters in Q and in the gates, as helpers.make_rnet)
    for m in out[1:]:
        m.qnet.load_state_dict(out[0].qnet.state_dict())
    return out


def play(kind, cycles, check):
    """the loop of examples/battle_batch_drqn.py for side 0 (side 1 acts at random); check(cycle, e, batch model's rows, world model,
    view rows, feature rows, ids) per world with agents"""
    import torch
    envs = batch_worlds()
    handles = envs[0].get_handles()
    dev = torch.device("cuda", envs[0].device_id)
    batch = magent_amd.EnvBatch(envs, n_threads=1)
    nums = batch.nums_array().copy()
    off, tot = batch.packed_offsets(nums)
    hgt, wid, chan = envs[0].get_view_space(handles[0])
    F = envs[0].get_feature_space(handles[0])[0]
    A = envs[0].get_action_space(handles[0])[0]
    cells = kind == "cells"
    views = [torch.zeros((int(tot[g]), hgt, wid, 8), dtype=torch.bfloat16, device=dev) if cells else torch.zeros((int(tot[g]), hgt, wid, chan), device=dev)
             for g in range(2)]
    feats = [torch.zeros((int(tot[g]), F), device=dev) for g in range(2)]
    acts = [torch.zeros(int(tot[g]), dtype=torch.int32, device=dev) for g in range(2)]
    ids = [torch.full((int(tot[g]),), -1, dtype=torch.int32, device=dev) for g in range(2)]
    pv, pf, pa, pi = (batch.packed_pointers(t, off) for t in (views, feats, acts, ids))
    flags = batch.cell_flags([[views[0], views[1]]] * len(envs))
    kw = {"torch": {}, "f32": {}, "cells": {"infer_dtype": "bf16"}}[kind]
    old = os.environ.get("MAGENT_POLICY_F32")
    if kind == "torch":
        os.environ["MAGENT_POLICY_F32"] = "torch"
    try:
        whole = models(envs[0], handles[0], 1, scale=1.0 if kind == "torch" else 3.0, **kw)[0]     # (the torch test: the weights of the test whose bound it takes)
    finally:
        if kind == "torch":
            if old is None:
                del os.environ["MAGENT_POLICY_F32"]
            else:
                os.environ["MAGENT_POLICY_F32"] = old
    assert (whole._hip is None) == (kind == "torch") and (kind != "cells" or whole.bf16_kernels)
    own = models(envs[0], handles[0], len(envs), **({"infer_dtype": "bf16"} if cells else {}))
    for m in own:
        m.qnet.load_state_dict(whole.qnet.state_dict())
        assert m._hip is not None
    g = torch.Generator().manual_seed(3)
    deaths = 0
    for cycle in range(cycles):
        batch.agent_ids(pi)                                   # the population the cycle's render will write
        tables = batch.packed_segments(off)
        counts = batch.nums_array().copy()
        own_ids = [env.get_agent_id(handles[0]) for env in envs]
        batch.cycle(pv, pf, pa, None, view_cells=flags)
        q_ref = None
        if kind == "torch":       # Q of the PyTorch path's network for the states it is about to use
            prev, zero = whole.agent_states, torch.zeros(S, device=dev)
            rows = [zero] * int(tot[0])
            for e in range(len(envs)):
                for k, i in enumerate(own_ids[e]):
                    rows[int(off[e][0]) + k] = prev.get((e, int(i)), zero)
            with torch.no_grad():
                q_ref, _ = whole.qnet(views[0], feats[0], int(tot[0]), 1, torch.stack(rows).unsqueeze(0))
        best = whole.infer_action((views[0], feats[0]), ids[0], policy="greedy", segments=tables[0])
        torch.cuda.synchronize()
        keys = []
        for e, env in enumerate(envs):
            o, n = int(off[e][0]), int(counts[e][0])
            assert torch.equal(ids[0][o:o + n].cpu(), torch.as_tensor(own_ids[e], dtype=torch.int32)), (cycle, e)
            keys += [(e, int(i)) for i in own_ids[e]]
            if n:
                check(cycle, e, whole, best[o:o + n], own[e], views[0][o:o + n], feats[0][o:o + n], own_ids[e], o,
                      None if q_ref is None else q_ref[o:o + n])
        assert list(whole.agent_states.keys()) == keys, cycle
        deaths += int(nums[:, 0].sum() - counts[:, 0].sum() > 0)
        acts[0].copy_(best)
        acts[1].copy_(torch.randint(A, (int(tot[1]),), generator=g).to(torch.int32))
    assert deaths > 0, "no agent of side 0 died: the segments never shrank"
    for env in envs:
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f32", "cells"])
def test_one_segmented_call_per_side_equals_the_models_per_world(kind):
    """greedy actions and the states of every world's rows: bit for bit those of that world's own model, plain, on the same rows"""
    import torch

    def check(cycle, e, whole, best, model, view, feat, ids, o, q_ref):
        a = model.infer_action((view.contiguous(), feat.contiguous()), ids, policy="greedy")
        assert torch.equal(best, a), (kind, cycle, e, int((best != a).sum()))
        assert torch.equal(whole._hip._states[o:o + len(ids)], model._hip._states), (kind, cycle, e)
    play(kind, 16, check)


@pytest.mark.gpu
def test_the_torch_path_keeps_the_same_semantics():
    """MAGENT_POLICY_F32=torch with segments= against the per-world kernel models: states within 2e-5, greedy actions equal except at
    near-ties of Q (the bound of test_drqn_device_path_matches_the_torch_path_in_a_battle)"""
    import torch
    near, total = [0], [0]

    def check(cycle, e, whole, best, model, view, feat, ids, o, q_ref):
        a = model.infer_action((view.contiguous(), feat.contiguous()), ids, policy="greedy")
        sw, sm = whole.agent_states, model.agent_states
        for i in ids[:: max(1, len(ids) // 10)]:
            assert torch.allclose(sw[(e, int(i))], sm[int(i)], atol=2e-5, rtol=0), (cycle, e, int(i))
        differ = (best != a).cpu().numpy()
        if differ.any():
            gap = np.sort(q_ref.cpu().numpy(), axis=1)
            gap = gap[:, -1] - gap[:, -2]
            assert (gap[differ] <= 1e-4 * float(q_ref.abs().max()) + 1e-6).all(), (cycle, e, gap[differ])
            near[0] += int(differ.sum())
        total[0] += len(ids)
    play("torch", 16, check)
    assert near[0] <= total[0] * 1e-3, (near, total)


def test_numpy_inputs_on_the_cpu_key_their_states_by_world():
    """the PyTorch path without a GPU: NumPy observations of two made-up worlds in one packed call with a pad row and a stale row; every
    world equals a model of its own over three calls (shrinking, an id reused across worlds), rows in no segment start from zeros, return
    an action and are not stored; forget_segments; a plain call afterwards keeps world 0's states"""
    import torch
    from magent_amd.builtin.torch_model import DeepRecurrentQNetwork
    env = H.SpacesEnv((5, 5, 3), 7, 9)
    torch.manual_seed(4)
    whole, w0, w1 = [DeepRecurrentQNetwork(env, None, "m%d" % k, memory_size=4, device="cpu") for k in range(3)]
    for m in (w0, w1):
        m.qnet.load_state_dict(whole.qnet.state_dict())
    plans = [([0, 1, 2], [0, 1, 2, 3]), ([2, 0], [3, 1, 0]), ([0, 5], [1, 5])]
    for call, (a, b) in enumerate(plans):
        seg = np.asarray([[0, len(a)], [4, len(b)]], dtype=np.int32)
        n = 9
        view, featv = H.make_policy_inputs((5, 5, 3), 7, n, 40 + call)
        ids = np.full(n, 1, dtype=np.int32)          # (gap rows carry id 1)
        ids[0:len(a)], ids[4:4 + len(b)] = a, b
        out = whole.infer_action((view.numpy(), featv.numpy()), ids, policy="greedy", segments=seg)
        assert isinstance(out, np.ndarray) and out.shape == (n,) and ((out >= 0) & (out < 9)).all()
        for m, o, w in ((w0, 0, a), (w1, 4, b)):
            own = m.infer_action((view[o:o + len(w)].numpy(), featv[o:o + len(w)].numpy()), np.asarray(w, dtype=np.int32), policy="greedy")
            assert np.array_equal(out[o:o + len(w)], own), (call, o)
        got = whole.agent_states
        assert list(got.keys()) == [(0, i) for i in a] + [(1, i) for i in b]
        for s, m, w in ((0, w0, a), (1, w1, b)):
            for i in w:
                assert torch.allclose(got[(s, i)], m.agent_states[i], atol=1e-6, rtol=0), (call, s, i)
        # a gap row starts from zeros whatever its id
        zero = DeepRecurrentQNetwork(env, None, "z", memory_size=4, device="cpu")
        zero.qnet.load_state_dict(whole.qnet.state_dict())
        assert zero.infer_action((view[8:9].numpy(), featv[8:9].numpy()), [1], policy="greedy")[0] == out[8]
    with pytest.raises(ValueError, match="segment 1"):
        whole.infer_action((view.numpy(), featv.numpy()), ids, policy="greedy", segments=[[0, 3], [2, 2]])
    whole.forget_segments([1])
    assert list(whole.agent_states.keys()) == [(0, 0), (0, 5)]
    view, featv = H.make_policy_inputs((5, 5, 3), 7, 2, 50)
    out = whole.infer_action((view.numpy(), featv.numpy()), [5, 1], policy="greedy")           # plain: world 0's 5 carries on, 1 is new
    own = w0.infer_action((view.numpy(), featv.numpy()), [5, 1], policy="greedy")
    assert np.array_equal(out, own) and list(whole.agent_states.keys()) == [5, 1]
    assert torch.allclose(whole.agent_states[5], w0.agent_states[5], atol=1e-6, rtol=0)
