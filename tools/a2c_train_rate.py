"""Development helper (GPU box): what AdvantageActorCritic.train costs from a device recorder.  Battle-shaped worlds as in
tools/replay_rate.py (13 x 13 x 7 float32 views, 34 features, 2 x 2000 agents a world, each side's rows in one packed buffer).  One
process, the same recorded round for every route:

(a) train(rec): the packed route -- packed()'s tensors, one batched bootstrap pass, DeviceEpisodesBuffer.returns.
(b) train(wrapper that offers episodes() only): the episodes route, what train(rec) did before the packed route existed; the recorder's
    per-agent view is dropped before every run, as a fresh round would find it.
    Both at K = 8 and 32 worlds, capacity 1000, a round of --round_len cycles (50,000 transitions: a full autograd step over all of them).
    Host clock around the call between two device synchronisations; --runs + 1 calls, the first left out.
(c) returns() alone between device events, the C entries replay_returns (LDS-staged) and replay_returns_direct beside it, in blocks of
    `reps` back-to-back calls after --warm seconds of the same calls (the clocks ramp during the first milliseconds of work); the blocks
    of the two entries alternate.  At capacity 1000 and with everybody tracked at 8, 32 and 128 worlds; a world loses 1 % of its agents
    per cycle, so episodes are 1 to --round_len transitions long.  The kernel reads lengths, bases and rewards only: these recorders
    take 1 x 1 x 1 views, and 128 worlds x 4000 agents fit.

    python tools/a2c_train_rate.py [--round_len 50] [--runs 5] [--warm 1.0] [--skip_train]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from magent_amd.builtin.torch_model import AdvantageActorCritic  # noqa: E402
from magent_amd.replay import DeviceEpisodesBuffer  # noqa: E402
from replay_rate import A, F, VS, side_buffers, timed  # noqa: E402


class Spaces(object):
    """the model's constructor reads the spaces only"""
    device_id = 0
    get_view_space = lambda self, h: VS
    get_feature_space = lambda self, h: (F,)
    get_action_space = lambda self, h: (A,)


class EpisodesOnly(object):
    def __init__(self, rec):
        self.rec = rec

    def episodes(self):
        self.rec._entries = None
        return self.rec.episodes()


def line(what, ms):
    print("    %-58s median %9.4f ms   raw %s" % (what, float(np.median(ms[1:])), " ".join("%.4f" % m for m in ms)), flush=True)


def train_rates(args, K, dev):
    ids, view, feat, acts, rews, seg = side_buffers(K, 2000, False, dev, 10 * K)
    rec = DeviceEpisodesBuffer(1000, 1000 * args.round_len, VS, (F,), device=dev)
    order = torch.randperm(ids.shape[0], dtype=torch.int32, device=dev)
    for t in range(args.round_len):
        rec.record_step(ids, (view, feat), acts, rews * (t % 7 - 3), segments=seg, order=order)
    rec.close(ids, seg)
    n = rec.packed()[0].shape[0]
    print("float32  %3d worlds x 2 x 2000 agents, capacity 1000, %d cycles: %d transitions of %d agents" % (K, args.round_len, n, rec.tracked), flush=True)
    out = {}
    for name, buf in (("(a) train(rec), packed route", rec), ("(b) train(episodes() only), the route before", EpisodesOnly(rec))):
        torch.manual_seed(1)
        model = AdvantageActorCritic(Spaces(), 0, "rate", device=dev)
        ms = []
        for _ in range(args.runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with open(os.devnull, "w") as null:
                stdout, sys.stdout = sys.stdout, null
                try:
                    model.train(buf)
                finally:
                    sys.stdout = stdout
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        line(name, ms)
        out[name[:3]] = float(np.median(ms[1:]))
        del model
    print("    (b) / (a) = %.1f" % (out["(b)"] / out["(a)"]), flush=True)
    del rec
    torch.cuda.empty_cache()


def returns_rates(args, K, capacity, dev):
    agents = 2000
    pad = (agents + 3) // 4 * 4
    n = K * pad
    ids = (torch.arange(n, dtype=torch.int32, device=dev) % pad).contiguous()
    view, feat = torch.zeros((n, 1, 1, 1), device=dev), torch.zeros((n, 1), device=dev)
    acts, rews = torch.zeros(n, dtype=torch.int32, device=dev), torch.randn(n, device=dev)
    rec = DeviceEpisodesBuffer(capacity, capacity * args.round_len, (1, 1, 1), (1,), device=dev)
    count = lambda t: agents - t * agents // 100
    for t in range(args.round_len):
        seg = np.stack([np.arange(K) * pad, np.full(K, count(t))], axis=1).astype(np.int32)
        rec.record_step(ids, (view, feat), acts, rews, segments=seg)
    rec.close(ids, np.stack([np.arange(K) * pad, np.full(K, count(args.round_len))], axis=1).astype(np.int32))
    p = rec.packed()
    n_trans, tracked = int(p[3].shape[0]), rec.tracked
    boot = torch.randn(tracked, device=dev)
    out, lib, stream = torch.empty(n_trans, device=dev), rec._lib, torch.cuda.current_stream(dev).cuda_stream
    entries = {"replay_returns (staged)": lib.replay_returns}
    if hasattr(lib, "replay_returns_direct"):
        entries["replay_returns_direct"] = lib.replay_returns_direct
    call = lambda fn: fn(rec._st_ref, tracked, n_trans, rec._base.data_ptr(), p[3].data_ptr(), boot.data_ptr(), 0.99, out.data_ptr(), stream)
    fns = {name: (lambda fn=fn: call(fn)) for name, fn in entries.items()}
    fns["rec.returns() (allocates its output)"] = lambda: rec.returns(boot, 0.99)
    results = []
    for name, fn in fns.items():
        got = rec.returns(boot, 0.99) if name.startswith("rec.") else (out.fill_(0), fn(), out.clone())[2]
        results.append(got)
    assert all(torch.equal(results[0].view(torch.int32), r.view(torch.int32)) for r in results[1:]), "the entries disagree"
    reps = max(10, min(1000, int(4e7 / max(n_trans, 1))))
    t_end = time.perf_counter() + args.warm
    while time.perf_counter() < t_end:
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(args.runs + 1):
        for name, fn in fns.items():
            times[name].append(timed(lambda: [fn() for _ in range(reps)]) / reps)
    print("returns  %3d worlds, capacity %6d: %8d transitions of %6d agents, blocks of %d calls" % (K, capacity, n_trans, tracked, reps), flush=True)
    for name, ms in times.items():
        line(name, ms)
    del rec, out, p
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--round_len", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5, help="timed runs behind the first, which is left out")
    ap.add_argument("--warm", type=float, default=1.0, help="seconds of warm-up before (c)'s figures")
    ap.add_argument("--skip_train", action="store_true", help="(c) only")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if not args.skip_train:
        for K in (8, 32):
            train_rates(args, K, dev)
    for K, capacity in ((8, 1000), (32, 1000), (8, 16000), (32, 64000), (128, 256000)):
        returns_rates(args, K, capacity, dev)


if __name__ == "__main__":
    main()
