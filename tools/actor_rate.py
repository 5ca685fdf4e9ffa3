"""Rate of the rule-based actors' device entry (actor_infer_action_device, magent_amd/csrc/actors.hip) on device observations,
against the host symbols on the same observations.

  python tools/actor_rate.py [--reps 20]

Worlds: config 3's battle 1000² at 2 x 400k (13 x 13 x 7 views: RushPredator and RunawayPrey of group 0 against group 1) and
config 4's gather 500² (100k agents, 20k food: RushGatherer).  One JSON line per actor: ms per call (HIP events on torch's stream,
mean of --reps calls after two warm-up calls), read GB/s of the whole view (the bytes predator and gatherer scan; runaway reads
nine cells of one channel per agent, its figure is the equivalent rate), and the host symbol's ms per call on a host copy.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def world(game, size, counts, seed=12345):
    import magent_amd
    env = magent_amd.GridWorld(game, map_size=size, device_obs=True)
    env.set_seed(seed)
    env.reset()
    for h, n in zip(env.get_handles(), counts):
        env.add_agents(h, "random", n=n)
    return env


def time_actor(name, actor, view, feat, reps):
    import torch
    for _ in range(2):
        actor.infer_action((view, feat))
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        actor.infer_action((view, feat))
    stop.record()
    stop.synchronize()
    ms = start.elapsed_time(stop) / reps
    hv, hf = view.cpu().numpy(), feat.cpu().numpy()
    t = time.perf_counter()
    actor.infer_action((hv, hf))
    host_ms = (time.perf_counter() - t) * 1e3
    view_bytes = view.numel() * 4
    drew = float(actor.last_drew.float().mean().item())
    print(json.dumps({"actor": name, "n": int(view.shape[0]), "view": list(view.shape[1:]), "ms_per_call": round(ms, 4),
                      "view_GBps": round(view_bytes / ms / 1e6, 1), "host_ms_per_call": round(host_ms, 2),
                      "speedup_vs_host": round(host_ms / ms, 1), "share_drawn": round(drew, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from magent.builtin.rule_model import RunawayPrey, RushGatherer, RushPredator
    env = world("battle", 1000, (400000, 400000))
    g0, g1 = env.get_handles()
    view, feat = env.get_observation(g0)
    time_actor("RushPredator battle 1000 2x400k", RushPredator(env, g0, g1), view, feat, args.reps)
    time_actor("RunawayPrey battle 1000 2x400k", RunawayPrey(env, g0, g1), view, feat, args.reps)
    env.close()
    del view, feat, env
    env = world("gather", 500, (20000, 100000))
    food, agent = env.get_handles()
    view, feat = env.get_observation(agent)
    time_actor("RushGatherer gather 500 100k", RushGatherer(env, agent), view, feat, args.reps)


if __name__ == "__main__":
    main()
