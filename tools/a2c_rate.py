"""Development helper (GPU box): time of AdvantageActorCritic.infer_action on device observations of the battle shape (13 x 13 x 7, 34
features, 21 actions), with and without CommNet -- the float32 kernel path (magent_amd/csrc/policy_a2c_f32.hip), the opt-in bf16 kernel
path (infer_dtype="bf16", magent_amd/csrc/policy_a2c_bf16.hip) on the same float32 views and on the engine's bf16 cells of them, and the
PyTorch path (MAGENT_POLICY_F32=torch: the network's forward pass, then torch.multinomial) of the same network on the same inputs, all in
one session.

Each size and path: a warm-up of --warm seconds of calls first (code objects load, libraries pick their algorithms, clocks settle), then
the calls of one timed region (at least 1000) behind a synchronize.  Useful FLOP are those of the network's matrix products, 2 K N per layer and agent.

    python tools/a2c_rate.py [n ...] [--reps R] [--no-torch]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK = 157.3e12          # f32 matrix peak of the MI355X (v_mfma_f32_32x32x2_f32)
VS, F, A = (13, 13, 7), 34, 21


class _Env(object):      # the model's constructor reads the spaces only
    device_id = 0

    def get_view_space(self, h):
        return VS

    def get_feature_space(self, h):
        return (F,)

    def get_action_space(self, h):
        return (A,)


def flops(comm):
    k = VS[0] * VS[1] * VS[2]
    return 2 * (k * 256 + F * 256 + 512 * 512 + (2 * 1024 * 512 if comm else 0) + 512 * (A + 1))


def timed(fn, reps, warm_s):
    t_end = time.perf_counter() + warm_s
    while time.perf_counter() < t_end:
        fn()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[40000, 131072, 400000])
    ap.add_argument("--reps", type=int, default=0, help="timed calls per size and path (default: ~3 s of calls, at least 1000)")
    ap.add_argument("--warm", type=float, default=2.0, help="seconds of warm-up calls per size and path")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from magent_amd.builtin.torch_model.a2c import AdvantageActorCritic
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    env = _Env()
    for comm in (False, True):
        torch.manual_seed(0)
        model = AdvantageActorCritic(env, 0, "rate", use_comm=comm)
        assert model._hip is not None, "the kernel path is not taken"
        os.environ["MAGENT_POLICY_F32"] = "torch"
        ref = AdvantageActorCritic(env, 0, "torch", use_comm=comm)
        del os.environ["MAGENT_POLICY_F32"]
        ref.net.load_state_dict(model.net.state_dict())
        assert ref._hip is None
        bf16 = AdvantageActorCritic(env, 0, "bf16", use_comm=comm, infer_dtype="bf16")
        bf16.net.load_state_dict(model.net.state_dict())
        assert bf16.bf16_kernels, "the bf16 kernel path is not taken"
        per_agent = flops(comm)
        for n in args.sizes:
            g = torch.Generator(device=dev).manual_seed(n)
            view = (torch.rand((n,) + VS, device=dev, generator=g) < 0.3).float()
            feat = torch.rand((n, F), device=dev, generator=g)
            cells = torch.zeros((n,) + VS[:2] + (8,), dtype=torch.bfloat16, device=dev)       # the engine's cells of the same views
            cells[..., :VS[2]] = view.to(torch.bfloat16)
            cells[..., 7] = 1.0
            assert bf16._on_kernels(cells, feat) and bf16._on_kernels(view, feat) and model._on_kernels(view, feat)
            row = "n %7d  %s" % (n, "CommNet" if comm else "plain  ")
            paths = (("f32 kernels", model, view), ("bf16 kernels, f32 views", bf16, view), ("bf16 kernels, bf16 cells", bf16, cells))
            for name, m, v in paths + (() if args.no_torch else (("PyTorch", ref, view),)):
                call = lambda: m.infer_action((v, feat), None)
                call()
                torch.cuda.synchronize()
                reps = args.reps or max(1000, int(3.0 / max(1e-4, n * per_agent / (0.3 * PEAK))))
                dt = timed(call, reps, args.warm)
                row += "\n    %-26s infer_action %8.3f ms (%d calls) = %6.1f TFLOP/s useful, %.3f of the f32 matrix peak" % (
                    name, dt * 1e3, reps, n * per_agent / dt / 1e12, n * per_agent / dt / PEAK)
            print(row, flush=True)
            del view, feat, cells
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
