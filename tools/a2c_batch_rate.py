"""Development helper (GPU box): what the segmented A2C call buys a batch of worlds.  K battle-shaped worlds (13 x 13 x 7 views, 34 features,
21 actions) of 2 x 2000 agents, CommNet on; one SIDE's observations of all worlds in one packed buffer (every world's segment starts on a
multiple of 4 rows).  Timed against each other, in one process:

    segmented        ONE AdvantageActorCritic.infer_action(..., segments=table) over the packed buffer
    per environment  K plain infer_action calls, one on each world's rows of the same buffer -- the only way without `segments`

for the float32 kernels on float32 views and the bf16 kernels on bf16 cells.  Before any timing the two ways are compared bit for bit
(the policy object's calls with one fixed u).  Timing: after --warm seconds of both, blocks of --reps rounds of either way alternate,
each block between two device events on torch's stream (the host enqueues ahead; the events see when the device finished); the figure is
the median block, per round of one side, with the fastest and slowest block beside it.

    python tools/a2c_batch_rate.py [K ...] [--agents 2000] [--reps 50] [--blocks 7] [--warm 1.0]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

VS, F, A = (13, 13, 7), 34, 21


class _Env(object):      # the model's constructor reads the spaces only
    device_id = 0

    def get_view_space(self, h):
        return VS

    def get_feature_space(self, h):
        return (F,)

    def get_action_space(self, h):
        return (A,)


def block_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("worlds", nargs="*", type=int, default=[8, 32, 128])
    ap.add_argument("--agents", type=int, default=2000, help="agents per side and world")
    ap.add_argument("--reps", type=int, default=50, help="rounds per timed block")
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks of either way (they alternate)")
    ap.add_argument("--warm", type=float, default=1.0, help="seconds of warm-up rounds of either way")
    args = ap.parse_args()
    from magent_amd.builtin.torch_model.a2c import AdvantageActorCritic
    dev = torch.device("cuda", 0)
    for dtype in ("f32", "bf16"):
        torch.manual_seed(0)
        model = AdvantageActorCritic(_Env(), 0, "rate", use_comm=True, infer_dtype=dtype)
        assert model._hip is not None and model.bf16_kernels == (dtype == "bf16"), "the kernel path is not taken"
        for K in args.worlds:
            pad = (args.agents + 3) // 4 * 4
            n = K * pad
            seg = np.stack([np.arange(K) * pad, np.full(K, args.agents)], axis=1).astype(np.int32)
            g = torch.Generator(device=dev).manual_seed(K)
            view = (torch.rand((n,) + VS, device=dev, generator=g) < 0.3).float()
            feat = torch.rand((n, F), device=dev, generator=g)
            if dtype == "bf16":                                 # the engine's cells of the same views
                cells = torch.zeros((n,) + VS[:2] + (8,), dtype=torch.bfloat16, device=dev)
                cells[..., :VS[2]] = view.to(torch.bfloat16)
                cells[..., 7] = 1.0
                view = cells
            assert model._on_kernels(view, feat)
            spans = [(int(b), int(c)) for b, c in seg]
            one = lambda: model.infer_action((view, feat), None, segments=seg)
            per_env = lambda: [model.infer_action((view[b:b + c], feat[b:b + c]), None) for b, c in spans]
            # the same results first
            u = torch.rand(n, device=dev, generator=g)
            whole = model._hip.infer(view, feat, u=u, want_policy=True, want_value=True, segments=seg)
            for b, c in spans:
                own = model._hip.infer(view[b:b + c], feat[b:b + c], u=u[b:b + c], want_policy=True, want_value=True)
                assert all(torch.equal(w[b:b + c].view(torch.int32), o.view(torch.int32)) for w, o in zip(whole, own)), "segmented and per-environment calls differ"
            for fn in (one, per_env):
                t_end = time.perf_counter() + args.warm
                while time.perf_counter() < t_end:
                    fn()
                    torch.cuda.synchronize()
            times = {"segmented": [], "per environment": []}
            for _ in range(args.blocks):
                times["segmented"].append(block_ms(one, args.reps))
                times["per environment"].append(block_ms(per_env, args.reps))
            med = {k: float(np.median(v)) for k, v in times.items()}
            print("%s  %3d worlds x %d agents a side (%d rows), CommNet: one side's round" % (dtype, K, args.agents, n))
            for k, launches in (("segmented", 10), ("per environment", 9 * K)):
                print("    %-16s %8.3f ms  (blocks %.3f .. %.3f; %d launches)" % (k, med[k], min(times[k]), max(times[k]), launches))
            print("    per environment / segmented = %.2f" % (med["per environment"] / med["segmented"]), flush=True)
            del view, feat
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
