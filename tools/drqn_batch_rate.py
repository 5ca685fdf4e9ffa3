"""Development helper (GPU box): what the segmented DRQN call buys a batch of worlds.  K battle-shaped worlds (13 x 13 x 7 views, 34 features,
21 actions) of 2000 agents a side; one SIDE's observations and ids (arange(2000) in every world: they collide) of all worlds in one packed
buffer (every world's segment starts on a multiple of 4 rows).  Timed against each other, in one process:

    segmented        ONE policy.infer(..., ids, segments=table) over the packed buffer: the look-up launch, four launches, one sort
    per environment  K plain policy.infer calls, one policy object per world (each carries its world's id table) on that world's rows of
                     the same buffer: four launches and a sort each -- the only way without `segments`

for the float32 kernels, the bf16 kernels on float32 views and the bf16 kernels on bf16 cells (hip_policy's classes on one network).
Before any timing two steps of either way are compared bit for bit (actions, Q, h').  Every timed call is a real step on a full table.
Timing: after --warm seconds of both, blocks of rounds of either way alternate, each block between two device events on torch's stream
(the host enqueues ahead; the events see when the device finished); the figure is the median block, per round of one side, with the
fastest and slowest block beside it.  Rounds per block: --reps for the segmented call (blocks x reps >= 1000 calls), and for the
per-environment way as many as make blocks x rounds x K >= 1000 calls (at least 4).

Then EnvBatch.agent_ids against the K x 2 GridWorld.get_info_device(handle, "id", out) calls it replaces, on K real battle worlds of
2 x 2000 agents, the same way (1000 calls of agent_ids; rounds of K x 2 calls).

    python tools/drqn_batch_rate.py [K ...] [--agents 2000] [--reps 150] [--blocks 7] [--warm 1.0] [--skip_ids]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

VS, F, A = (13, 13, 7), 34, 21


def block_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def race(ways, reps, blocks, warm):
    """{name: fn} timed in alternating blocks of reps[name] rounds -> {name: (median, fastest, slowest) ms per round}"""
    for fn in ways.values():
        t_end = time.perf_counter() + warm
        while time.perf_counter() < t_end:
            fn()
            torch.cuda.synchronize()
    times = {k: [] for k in ways}
    for _ in range(blocks):
        for k, fn in ways.items():
            times[k].append(block_ms(fn, reps[k]))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in times.items()}


def policy_rates(args, dev):
    from magent_amd.builtin.torch_model import hip_policy
    from magent_amd.builtin.torch_model.drqn import _RecurrentQNet
    torch.manual_seed(0)
    net = _RecurrentQNet(VS, (F,), A, True).to(dev)
    for kind, cls in (("f32", hip_policy.HipDrqnPolicyF32), ("bf16", hip_policy.HipDrqnPolicy), ("bf16 cells", hip_policy.HipDrqnPolicy)):
        for K in args.worlds:
            pad = (args.agents + 3) // 4 * 4
            n = K * pad
            seg = np.stack([np.arange(K) * pad, np.full(K, args.agents)], axis=1).astype(np.int32)
            spans = [(int(b), int(c)) for b, c in seg]
            g = torch.Generator(device=dev).manual_seed(K)
            view = (torch.rand((n,) + VS, device=dev, generator=g) < 0.3).float()
            feat = torch.rand((n, F), device=dev, generator=g)
            if kind == "bf16 cells":                            # the engine's cells of the same views
                cells = torch.zeros((n,) + VS[:2] + (8,), dtype=torch.bfloat16, device=dev)
                cells[..., :VS[2]] = view.to(torch.bfloat16)
                cells[..., 7] = 1.0
                view = cells
            ids = torch.full((n,), -1, dtype=torch.int32, device=dev)
            for b, c in spans:
                ids[b:b + c] = torch.arange(c, dtype=torch.int32, device=dev)
            whole = cls(net, VS, (F,), A, dev)
            own = [cls(net, VS, (F,), A, dev) for _ in spans]
            one = lambda: whole.infer(view, feat, ids, segments=seg)
            per_env = lambda: [p.infer(view[b:b + c], feat[b:b + c], ids[b:b + c]) for p, (b, c) in zip(own, spans)]
            for step in range(2):                               # the same results first: an empty table, then a full one
                a, q = whole.infer(view, feat, ids, want_q=True, segments=seg)
                for p, (b, c) in zip(own, spans):
                    a1, q1 = p.infer(view[b:b + c], feat[b:b + c], ids[b:b + c], want_q=True)
                    same = torch.equal(a[b:b + c], a1) and torch.equal(q[b:b + c].view(torch.int32), q1.view(torch.int32)) and \
                        torch.equal(whole._states[b:b + c].view(torch.int32), p._states.view(torch.int32))
                    assert same, "segmented and per-environment calls differ (%s, K %d, step %d)" % (kind, K, step)
            reps = {"segmented": args.reps, "per environment": max(4, -(-1000 // (K * args.blocks)))}
            res = race({"segmented": one, "per environment": per_env}, reps, args.blocks, args.warm)
            print("%-10s %3d worlds x %d agents a side (%d rows): one side's round" % (kind, K, args.agents, n))
            for k, launches in (("segmented", "5 launches + 1 sort"), ("per environment", "%d launches + %d sorts" % (4 * K, K))):
                print("    %-16s %8.3f ms  (blocks %.3f .. %.3f; %d calls timed; %s)" % (
                    (k,) + res[k] + (reps[k] * args.blocks * (1 if k == "segmented" else K), launches)))
            print("    per environment / segmented = %.2f" % (res["per environment"][0] / res["segmented"][0]), flush=True)
            del view, feat, whole, own
            torch.cuda.empty_cache()


def id_rates(args, dev):
    import magent_amd
    for K in args.worlds:
        envs = []
        for k in range(K):
            env = magent_amd.GridWorld("battle", map_size=100)
            env.set_seed(k)
            env.reset()
            for h in env.get_handles():
                env.add_agents(h, "random", n=args.agents)
            envs.append(env)
        handles = envs[0].get_handles()
        batch = magent_amd.EnvBatch(envs)
        off, rows = batch.packed_offsets()
        bufs = [torch.full((int(r),), -1, dtype=torch.int32, device=dev) for r in rows]
        ptrs = batch.packed_pointers(bufs, off)
        outs = [[bufs[g][int(off[e][g]):int(off[e][g]) + args.agents] for g in range(2)] for e in range(K)]
        batch.cycle(None, None, None, None)     # (as in a loop: environments cycled together share one engine stream from their first cycle on)
        one = lambda: batch.agent_ids(ptrs)

        def per_env():                          # the copies on the engine's stream(s), then torch's stream ordered behind them, as agent_ids does
            for e, env in enumerate(envs):
                for g, h in enumerate(handles):
                    env.get_info_device(h, "id", outs[e][g])
            for env in batch._distinct():
                env.order_torch_after()
        one()
        torch.cuda.synchronize()
        want = [b.clone() for b in bufs]
        for b in bufs:
            b.fill_(-1)
        per_env()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(want, bufs)), "agent_ids and get_info_device differ"
        reps = {"agent_ids": args.reps, "per environment": max(4, -(-1000 // (2 * K * args.blocks)))}
        res = race({"agent_ids": one, "per environment": per_env}, reps, args.blocks, args.warm)
        print("ids        %3d worlds x 2 x %d agents" % (K, args.agents))
        for k, what in (("agent_ids", "%d launches" % (-(-2 * K // 192))), ("per environment", "%d copies" % (2 * K))):
            print("    %-16s %8.3f ms  (blocks %.3f .. %.3f; %s)" % ((k,) + res[k] + (what,)))
        print("    per environment / agent_ids = %.2f" % (res["per environment"][0] / res["agent_ids"][0]), flush=True)
        for env in envs:
            env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("worlds", nargs="*", type=int, default=[8, 32, 128])
    ap.add_argument("--agents", type=int, default=2000, help="agents per side and world")
    ap.add_argument("--reps", type=int, default=150, help="rounds of the one-call way per timed block")
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks of either way (they alternate)")
    ap.add_argument("--warm", type=float, default=1.0, help="seconds of warm-up rounds of either way")
    ap.add_argument("--skip_ids", action="store_true")
    ap.add_argument("--skip_policy", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if not args.skip_policy:
        policy_rates(args, dev)
    if not args.skip_ids:
        id_rates(args, dev)


if __name__ == "__main__":
    main()
