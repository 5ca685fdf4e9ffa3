"""K battle worlds in one EnvBatch, one bf16 policy call per side and cycle.

    python examples/battle_batch_bf16.py [--envs 8] [--map_size 60] [--n 500] [--steps 50]

Per side ONE packed tensor of bf16 observation cells, one of feature rows and one of actions for all worlds
(EnvBatch.packed_offsets / packed_pointers: every world's segment starts on a multiple of 4 rows, i.e. 16-byte aligned, so the
worlds keep their batched form).  EnvBatch.cycle renders every world's cells into its segment, and DeepQNetwork(infer_dtype="bf16")
reads the whole tensor as it is: the MFMA kernels take the cells as operands (magent_amd/csrc/policy.hip).  The <= 3 pad rows
between two segments are zeroed once and never written; the actions computed for them are never read."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import magent_amd  # noqa: E402
from magent_amd.builtin.torch_model import DeepQNetwork  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--map_size", type=int, default=60)
    ap.add_argument("--n", type=int, default=500, help="agents per side and world")
    ap.add_argument("--steps", type=int, default=50)
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
    models = [DeepQNetwork(envs[0], h, "side%d" % i, memory_size=16, infer_dtype="bf16") for i, h in enumerate(handles)]

    # the buffers and their pointer arrays, once: a world's segment is sized for its agents at the start (worlds only shrink) and stays
    # where it is; the rows behind a segment's n living agents are stale and, like the pad rows, never read
    off, rows = batch.packed_offsets()
    H, W, _ = envs[0].get_view_space(handles[0])
    F = envs[0].get_feature_space(handles[0])[0]
    views = [torch.zeros((int(r), H, W, 8), dtype=torch.bfloat16, device=dev) for r in rows]
    feats = [torch.zeros((int(r), F), device=dev) for r in rows]
    acts = [torch.zeros(int(r), dtype=torch.int32, device=dev) for r in rows]
    rews = [torch.zeros(int(r), device=dev) for r in rows]
    view_p, feat_p, act_p, rew_p = (batch.packed_pointers(t, off) for t in (views, feats, acts, rews))
    cells = batch.cell_flags([views] * args.envs)

    agent_steps, t0 = 0, time.perf_counter()
    for step in range(args.steps):
        agent_steps += int(batch.nums_array().sum())
        # one library call: observe (cells into the packed tensors), act, step, rewards, clear_dead for every world.  The actions it
        # reads were computed from the observations of the cycle before (include/magent_runtime_api.h); the first cycle plays zeros
        dones = batch.cycle(view_p, feat_p, act_p, rew_p, view_cells=cells)
        for g, m in enumerate(models):        # ONE policy call per side for all worlds
            acts[g].copy_(m.infer_action((views[g], feats[g]), None, policy="e_greedy", eps=0.1))
        if step % 10 == 0 or all(dones):
            print("step %4d  alive per side %s" % (step, batch.nums_array().sum(axis=0).tolist()))
        if all(dones):
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d agent-steps in %.2f s = %.2e agent-steps/s (%d worlds, one bf16 policy call per side and cycle)" % (agent_steps, dt, agent_steps / dt, args.envs))


if __name__ == "__main__":
    main()
