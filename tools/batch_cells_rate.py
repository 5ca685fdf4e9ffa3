"""Development helper (GPU box): K battle worlds cycled by ONE magent_amd.EnvBatch with float32 views and with bf16 cells.

    python tools/batch_cells_rate.py 200 2000 32 [--regions 9] [--rounds 20] [--formats f32,cells] [--no-views]
    python tools/batch_cells_rate.py 600 20000 8

One set of K worlds per format, same seeds and same actions (they evolve alike), cycled in turn region by region in ONE process: a region is
`rounds` cycles between two env.sync().  Prints one JSON line: per format the median, the lowest and the highest ms per round over the
regions.  --no-views adds a third set cycled without observations: the round minus the render.  The engine reads MAGENT_TUNE once per
process (pipe_sweep=0: the generic render workgroups for both formats): one run per variant,
variants in turn.  --root DIR imports magent_amd from another checkout (float32 only there if it has no cells)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("map", type=int)
ap.add_argument("n", type=int)
ap.add_argument("k", type=int)
ap.add_argument("--regions", type=int, default=9)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--formats", default="f32,cells")
ap.add_argument("--no-views", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, args.root)
import numpy as np      # noqa: E402
import torch            # noqa: E402
import magent_amd       # noqa: E402
from magent_amd.builtin.config import _games      # noqa: E402

dev = torch.device("cuda", 0)
torch.manual_seed(0)          # (the same actions in every process)
formats = args.formats.split(",") + (["none"] if args.no_views else [])


def make(fmt):
    envs = []
    for k in range(args.k):
        env = magent_amd.GridWorld(_games.make("battle", args.map))
        env.set_seed(1000 + k); env.reset()
        for h in env.get_handles():
            env.add_agents(h, "random", n=args.n)
        envs.append(env)
    hs = envs[0].get_handles()
    H, W, C = envs[0].get_view_space(hs[0])
    shape, dtype = ((H, W, 8), torch.bfloat16) if fmt == "cells" else ((H, W, C), torch.float32)
    views = None if fmt == "none" else [[torch.empty((args.n,) + shape, dtype=dtype, device=dev) for _ in hs] for _ in envs]
    feats = None if fmt == "none" else [[torch.empty((args.n,) + envs[0].get_feature_space(h), device=dev) for h in hs] for _ in envs]
    rews = [[torch.empty(args.n, device=dev) for _ in hs] for _ in envs]
    batch = magent_amd.EnvBatch(envs, n_threads=8)
    batch.order_streams = False       # (this loop orders by env.sync(); no torch work touches the buffers in between)
    S = {"envs": envs, "batch": batch, "keep": (views, feats, rews), "ptrs": [batch.pointers(t) for t in (views, feats, rews)]}
    S["cells"] = batch.cell_flags(views) if fmt == "cells" else None
    return S


def cycle(S, acts):
    v, f, r = S["ptrs"]
    if S["cells"] is not None:
        S["batch"].cycle(v, f, acts, r, view_cells=S["cells"])
    else:
        S["batch"].cycle(v, f, acts, r)


sets = {fmt: make(fmt) for fmt in formats}
na = sets[formats[0]]["envs"][0].get_action_space(sets[formats[0]]["envs"][0].get_handles()[0])[0]
acts_t = [[[torch.randint(na, (args.n,), dtype=torch.int32, device=dev) for _ in range(2)] for _ in range(args.k)] for _ in range(4)]
acts = {fmt: [sets[fmt]["batch"].pointers(a) for a in acts_t] for fmt in formats}
torch.cuda.synchronize()
for fmt in formats:           # preheat: clocks, first-cycle paints and minimaps, grown buffers
    for s in range(10):
        cycle(sets[fmt], acts[fmt][s % 4])
    for e in sets[fmt]["envs"]:
        e.sync()
ms = {fmt: [] for fmt in formats}
for region in range(args.regions):
    for fmt in formats:
        S = sets[fmt]
        t0 = time.perf_counter()
        for s in range(args.rounds):
            cycle(S, acts[fmt][s % 4])
        for e in S["envs"]:
            e.sync()
        ms[fmt].append((time.perf_counter() - t0) / args.rounds * 1e3)
out = {"map": args.map, "agents_per_side": args.n, "envs": args.k, "regions": args.regions, "rounds": args.rounds, "tune": os.environ.get("MAGENT_TUNE", ""),
       "root": os.path.basename(os.path.abspath(args.root))}
for fmt in formats:
    S = sets[fmt]
    stats = np.array([e.pipeline_stats() for e in S["envs"]])
    out[fmt] = {"ms_per_round_median": round(float(np.median(ms[fmt])), 4), "min": round(min(ms[fmt]), 4), "max": round(max(ms[fmt]), 4),
                "cycles_in_pipeline": int(stats[:, 6].min()), "of_which_swept": int(stats[:, 7].min()), "agents_left_env0": S["batch"].nums()[0]}
print(json.dumps(out))
