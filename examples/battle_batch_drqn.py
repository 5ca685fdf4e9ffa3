"""K battle worlds in one EnvBatch, one recurrent Q network call per side and cycle.

    python examples/battle_batch_drqn.py [--envs 8] [--map_size 60] [--n 500] [--steps 50] [--infer_dtype bf16]

battle_batch_a2c.py with DeepRecurrentQNetwork: per side ONE packed tensor of observations (bf16 cells for --infer_dtype bf16, float32
views for f32), one of feature rows, one of actions and one of agent ids for all worlds (EnvBatch.packed_offsets / packed_pointers).  The
network keeps a GRU state per agent id, and every world numbers its agents from 0, so the call is told where the worlds lie:
EnvBatch.packed_segments(off)[g] is side g's (begin, count) table, EnvBatch.agent_ids writes every world's ids into the packed id buffers
in one launch, and infer_action(..., ids[g], segments=table) keys the states by (world, id) -- one call of five kernel launches and a sort
per side whatever K is.  The pad rows between two segments and the stale rows behind a world's living agents start from zeros and leave no
state; their actions are never read.

Order.  cycle() renders the observation of the population as it stands when the cycle STARTS, then steps and compacts.  The ids and the
table that describe a cycle's observations are therefore taken BEFORE that cycle."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import magent_amd  # noqa: E402
from magent_amd.builtin.torch_model import DeepRecurrentQNetwork  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--map_size", type=int, default=60)
    ap.add_argument("--n", type=int, default=500, help="agents per side and world")
    ap.add_argument("--steps", type=int, default=50)
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
    models = [DeepRecurrentQNetwork(envs[0], h, "side%d" % i, memory_size=1, infer_dtype=args.infer_dtype) for i, h in enumerate(handles)]
    cells = all(m.bf16_kernels for m in models)

    # the buffers and their pointer arrays, once: a world's segment is sized for its agents at the start (worlds only shrink) and stays
    # where it is; the rows behind a segment's living agents are stale
    off, rows = batch.packed_offsets()
    H, W, C = envs[0].get_view_space(handles[0])
    F = envs[0].get_feature_space(handles[0])[0]
    views = [torch.zeros((int(r), H, W, 8), dtype=torch.bfloat16, device=dev) if cells else torch.zeros((int(r), H, W, C), device=dev) for r in rows]
    feats = [torch.zeros((int(r), F), device=dev) for r in rows]
    acts = [torch.zeros(int(r), dtype=torch.int32, device=dev) for r in rows]
    rews = [torch.zeros(int(r), device=dev) for r in rows]
    ids = [torch.full((int(r),), -1, dtype=torch.int32, device=dev) for r in rows]
    view_p, feat_p, act_p, rew_p, id_p = (batch.packed_pointers(t, off) for t in (views, feats, acts, rews, ids))
    flags = batch.cell_flags([views] * args.envs)

    agent_steps, t0 = 0, time.perf_counter()
    for step in range(args.steps):
        agent_steps += int(batch.nums_array().sum())
        # the population this cycle's render will write: its ids (one launch for all worlds and sides) and its (begin, count) tables
        batch.agent_ids(id_p)
        tables = batch.packed_segments(off)
        # one library call: observe into the packed tensors, act, step, rewards, clear_dead for every world.  The actions it reads were
        # computed from the observations of the cycle before (include/magent_runtime_api.h); the first cycle plays zeros
        dones = batch.cycle(view_p, feat_p, act_p, rew_p, view_cells=flags)
        for g, m in enumerate(models):            # ONE policy call per side for all worlds, the states keyed by (world, id)
            acts[g].copy_(m.infer_action((views[g], feats[g]), ids[g], eps=0.05, segments=tables[g]))
        if step % 10 == 0 or all(dones):
            print("step %4d  alive per side %s" % (step, batch.nums_array().sum(axis=0).tolist()))
        if all(dones):
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d agent-steps in %.2f s = %.2e agent-steps/s (%d worlds, one %s DRQN call per side and cycle, %d states kept)" % (
        agent_steps, dt, agent_steps / dt, args.envs, args.infer_dtype, sum(len(m.agent_states) for m in models)))


if __name__ == "__main__":
    main()
