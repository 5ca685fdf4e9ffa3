"""Development helper (GPU box): time of DeepRecurrentQNetwork.infer_action on device observations of the battle shape (13 x 13 x 7, 34
features, 21 actions) -- the kernel path (magent_amd/csrc/policy_drqn_f32.hip: the DQN's trunk, the GRU cell, the head, the id-keyed
state table) at each size, the DQN's f32 kernels on the same inputs beside it (their difference is the GRU + head), and the PyTorch path
(MAGENT_POLICY_F32=torch: the per-id dict, torch's GRU) timed once per size.  Then the opt-in bf16 kernels (infer_dtype="bf16",
magent_amd/csrc/policy_drqn_bf16.hip) on the same float32 views and on the engine's bf16 cells of them.

Each size: ids of a whole side, calls keep their states (the ids of an episode).  Warm-up of WARM_S seconds of calls first (clocks and
power settle: /opt guides' "measuring" advice), then REPS calls timed as one region behind a synchronize.

    python tools/drqn_rate.py [n ...] [--reps R] [--no-torch] [--no-bf16]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK = 157.3e12          # f32 matrix peak of the MI355X (v_mfma_f32_32x32x2_f32)


class _Env(object):      # the model's constructor reads the spaces only
    device_id = 0

    def get_view_space(self, h):
        return (13, 13, 7)

    def get_feature_space(self, h):
        return (34,)

    def get_action_space(self, h):
        return (21,)


def flops(vs=(13, 13, 7), F=34, A=21):
    h, w, _ = vs
    trunk = 2 * ((h - 2) * (w - 2) * 32 * 63 + (h - 4) * (w - 4) * 32 * 288 + (h - 4) * (w - 4) * 32 * 256 + F * 256)
    gru = 2 * 3 * 512 * 1024
    head = 2 * 512 * (A + 1)
    return trunk, gru, head


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
    ap.add_argument("--reps", type=int, default=0, help="timed calls per size (default: ~5 s of calls, at least 100)")
    ap.add_argument("--warm", type=float, default=2.0, help="seconds of warm-up calls per size")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-bf16", action="store_true")
    args = ap.parse_args()
    from magent_amd.builtin.torch_model.drqn import DeepRecurrentQNetwork
    from magent_amd.builtin.torch_model.hip_policy import HipDqnPolicyF32
    from magent_amd.builtin.torch_model.dqn import _QNet
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    env = _Env()
    torch.manual_seed(0)
    model = DeepRecurrentQNetwork(env, 0, "rate", memory_size=4)
    assert model._hip is not None, "the kernel path is not taken"
    dqn = _QNet((13, 13, 7), (34,), 21, True, True).to(dev)
    dqn.load_state_dict({k: v for k, v in model.qnet.state_dict().items() if not k.startswith("rnn")})
    dqn_pol = HipDqnPolicyF32(dqn, (13, 13, 7), (34,), 21, dev)
    trunk, gru, head = flops()
    bf16 = None
    if not args.no_bf16:
        bf16 = DeepRecurrentQNetwork(env, 0, "rate16", memory_size=4, infer_dtype="bf16")
        assert bf16.bf16_kernels, "the bf16 kernel path is not taken"
        bf16.qnet.load_state_dict(model.qnet.state_dict())
    for n in args.sizes:
        g = torch.Generator(device=dev).manual_seed(n)
        view = (torch.rand((n, 13, 13, 7), device=dev, generator=g) < 0.3).float()
        feat = torch.rand((n, 34), device=dev, generator=g)
        ids = torch.arange(n, dtype=torch.int32, device=dev)
        call = lambda: model.infer_action((view, feat), ids, policy="greedy")
        call()
        torch.cuda.synchronize()
        reps = args.reps or max(100, int(5.0 / max(1e-4, n * 6.5e-8)))
        dt = timed(call, reps, args.warm)
        dq = timed(lambda: dqn_pol.infer(view, feat), reps, args.warm)
        total = n * (trunk + gru + head)
        rest = dt - dq
        print("n %7d  DRQN device infer_action %8.3f ms (%d calls) = %.1f TFLOP/s useful, %.3f of the f32 matrix peak;  DQN f32 kernels %.3f ms;"
              "  difference (GRU + head + table) %.3f ms = %.3f of the peak for the GRU's %.2f MFLOP per agent" % (
                  n, dt * 1e3, reps, total / dt / 1e12, total / dt / PEAK, dq * 1e3, rest * 1e3, n * (gru + head) / max(rest, 1e-9) / PEAK, gru / 1e6), flush=True)
        if bf16 is not None:
            cells = torch.zeros((n, 13, 13, 8), dtype=torch.bfloat16, device=dev)       # the engine's cells: channels, zeros, 1.0 in channel 7
            cells[..., :7] = view.to(torch.bfloat16)
            cells[..., 7] = 1.0
            for what, v in (("float32 views", view), ("bf16 cells", cells)):
                call16 = lambda: bf16.infer_action((v, feat), ids, policy="greedy")
                call16()
                torch.cuda.synchronize()
                d16 = timed(call16, reps, args.warm)
                print("n %7d  DRQN bf16 kernels, %-13s %8.3f ms (%d calls) = %.1f TFLOP/s useful;  %.2f x the f32 kernels" % (
                    n, what + ":", d16 * 1e3, reps, total / d16 / 1e12, dt / d16), flush=True)
            bf16.agent_states = {}
            del cells
        if not args.no_torch:
            os.environ["MAGENT_POLICY_F32"] = "torch"
            ref = DeepRecurrentQNetwork(env, 0, "torch", memory_size=4)
            del os.environ["MAGENT_POLICY_F32"]
            ref.qnet.load_state_dict(model.qnet.state_dict())
            ref.infer_action((view[:1024], feat[:1024]), ids[:1024], policy="greedy")       # (library warm-up)
            ref.agent_states = {}
            ref.infer_action((view, feat), ids, policy="greedy")                        # the table of a running episode
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref.infer_action((view, feat), ids, policy="greedy")
            torch.cuda.synchronize()
            print("n %7d  DRQN PyTorch path (dict of states, torch GRU) %.1f ms (one call)" % (n, (time.perf_counter() - t0) * 1e3), flush=True)
            del ref
        del view, feat, ids
        model.agent_states = {}
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
