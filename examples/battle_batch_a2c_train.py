"""K battle worlds in one EnvBatch, one CommNet actor-critic call per side and cycle -- and the transitions LEARNED from: one device
recorder per side (magent_amd.DeviceEpisodesBuffer), one AdvantageActorCritic.train per side every --round_len cycles.

    python examples/battle_batch_a2c_train.py [--envs 8] [--map_size 60] [--n 500] [--steps 60] [--round_len 25] [--capacity 256]
                                              [--infer_dtype bf16]

The loop is examples/battle_batch_a2c.py's, the recording examples/battle_batch_train.py's: per cycle the packed agent ids and the
(begin, count) table are taken BEFORE the cycle, and after it the recorder is handed the packed buffers as they are.  At a round's end
close() takes the ids once more, train(rec) reads the round where it lies -- packed()'s tensors as they are, ONE batched forward pass for
the bootstrap values of all episodes, the discounted returns computed on the device (DeviceEpisodesBuffer.returns) -- and reset() starts
the next round.  Worlds are not reset inside a round.

The one-cycle action lag, and what it means HERE.  EnvBatch.cycle reads the actions computed from the observations of the cycle BEFORE
(the first cycle plays zeros), as in every batch example.  The action stored beside an observation is the one the engine played in the
cycle that rendered it and produced the reward -- and it was sampled from the agent's observation of the cycle before, not from the one
stored beside it.  For the DQN (battle_batch_train.py) that does not matter: an off-policy learner takes any action.  A policy-gradient
learner weights log pi(action | stored observation) by the advantage, as if the action had been drawn from that observation's policy: the
round is therefore slightly off-policy, by one cycle's change of the observation.  The lag is the batch loop's property; this example
shows the data path and does not correct for it."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import magent_amd  # noqa: E402
from magent_amd.builtin.torch_model import AdvantageActorCritic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--map_size", type=int, default=60)
    ap.add_argument("--n", type=int, default=500, help="agents per side and world")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--round_len", type=int, default=25, help="cycles between two train() calls")
    ap.add_argument("--capacity", type=int, default=256, help="agents a side's recorder tracks per round")
    ap.add_argument("--infer_dtype", choices=("f32", "bf16"), default="bf16")
    args = ap.parse_args()

    envs = []
    for k in range(args.envs):
        env = magent_amd.GridWorld("battle", map_size=args.map_size)
        env.set_seed(k)
        env.reset()
        for h in env.get_handles():
            env.add_agents(h, "random", n=args.n)
        envs.append(env)
    handles = envs[0].get_handles()
    dev = torch.device("cuda", envs[0].device_id)
    batch = magent_amd.EnvBatch(envs)
    models = [AdvantageActorCritic(envs[0], h, "side%d" % i, use_comm=True, infer_dtype=args.infer_dtype) for i, h in enumerate(handles)]
    cells = all(m.bf16_kernels for m in models)

    off, rows = batch.packed_offsets()
    H, W, C = envs[0].get_view_space(handles[0])
    F = envs[0].get_feature_space(handles[0])[0]
    views = [torch.zeros((int(r), H, W, 8), dtype=torch.bfloat16, device=dev) if cells else torch.zeros((int(r), H, W, C), device=dev) for r in rows]
    feats = [torch.zeros((int(r), F), device=dev) for r in rows]
    acts = [torch.zeros(int(r), dtype=torch.int32, device=dev) for r in rows]
    rews = [torch.zeros(int(r), device=dev) for r in rows]
    ids = [torch.zeros(int(r), dtype=torch.int32, device=dev) for r in rows]
    view_p, feat_p, act_p, rew_p, id_p = (batch.packed_pointers(t, off) for t in (views, feats, acts, rews, ids))
    flags = batch.cell_flags([views] * args.envs)
    # the training pass takes float32 views: the recorder hands the cells' channels back as float32 (exact), view_channels
    recorders = [magent_amd.DeviceEpisodesBuffer(args.capacity, args.capacity * args.round_len, tuple(views[0].shape[1:]), (F,), view_dtype=views[0].dtype,
                                                 view_channels=C if cells else None, device=dev) for _ in handles]

    agent_steps, trained, t0 = 0, 0, time.perf_counter()
    for step in range(args.steps):
        agent_steps += int(batch.nums_array().sum())
        batch.agent_ids(id_p)                                   # the ids and the table of the rows this cycle renders
        segments = batch.packed_segments(off)
        dones = batch.cycle(view_p, feat_p, act_p, rew_p, view_cells=flags)
        for g, rec in enumerate(recorders):                     # before acts[g] is overwritten: the actions the cycle read
            rec.record_step(ids[g], (views[g], feats[g]), acts[g], rews[g], segments=segments[g],
                            order=torch.randperm(int(rows[g]), dtype=torch.int32, device=dev))
        tables = batch.packed_segments(off)                     # the counts behind this cycle's deaths: who acts next
        for g, m in enumerate(models):
            acts[g].copy_(m.infer_action((views[g], feats[g]), None, segments=tables[g]))
        if (step + 1) % args.round_len == 0 or all(dones):
            batch.agent_ids(id_p)                               # who is still there: the others' last transition is terminal
            for g, (rec, m) in enumerate(zip(recorders, models)):
                rec.close(ids[g], tables[g])
                s = rec.stats()
                (pg, vf, ent), value = m.train(rec)
                print("step %4d  side %d  recorded %d transitions of %d agents%s  pg %.5f  vf %.5f  ent %.5f  value %.5f"
                      % (step, g, s["transitions"], s["tracked"], " (OVERFLOW)" if s["overflow"] else "", pg, vf, ent, value))
                rec.reset()
            trained += 1
            print("step %4d  alive per side %s" % (step, batch.nums_array().sum(axis=0).tolist()))
        if all(dones):
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d agent-steps in %.2f s = %.2e agent-steps/s (%d worlds, %d train rounds per side)" % (agent_steps, dt, agent_steps / dt, args.envs, trained))


if __name__ == "__main__":
    main()
