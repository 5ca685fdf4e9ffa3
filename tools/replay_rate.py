"""Development helper (GPU box): what recording a packed batch costs.  K battle-shaped worlds (13 x 13 x 7 views, 34 features) of 2 x 2000
agents; each side's rows of all worlds in one packed buffer (every world's segment starts on a multiple of 4 rows), float32 views or bf16
cells.  One process, three measurements:

1. record_step for BOTH sides per cycle (magent_amd.DeviceEpisodesBuffer), capacity 1000 and capacity = everybody, against what it
   replaces: one utility.EpisodesBuffer.record_step per world and side on the same buffers (its ids read back per call, as np.asarray(ids)
   of a device tensor does).  Rounds of --round_len cycles (shorter where the log would pass --log_gb) between two device events on
   torch's stream, reset outside the events; >= --calls recorder calls per figure after --warm seconds; the figure is the median round per
   cycle with the fastest and slowest beside it, and the median of the cycles behind a round's first (admission done) on their own.
2. the copy kernel alone (replay_copy) at k = 1000 and k = 64,000 rows against torch.index_select of the same rows from the same four
   tensors into preallocated outputs: blocks of either alternate; GB/s of rows moved (each byte is read once and written once), the
   spread of the blocks, the ratio of the medians and the fraction of 8 TB/s that the traffic (twice the rows) comes to.
3. packed() at the end of a 50-cycle round, with its read-back.

    python tools/replay_rate.py [K ...] [--agents 2000] [--calls 1000] [--round_len 50] [--warm 1.0] [--skip_host]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from magent_amd import utility  # noqa: E402
from magent_amd.replay import DeviceEpisodesBuffer  # noqa: E402

VS, F, A = (13, 13, 7), 34, 21
HBM = 8e12


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def side_buffers(K, agents, cells, dev, seed):
    pad = (agents + 3) // 4 * 4
    n = K * pad
    g = torch.Generator(device=dev).manual_seed(seed)
    if cells:
        view = torch.zeros((n,) + VS[:2] + (8,), dtype=torch.bfloat16, device=dev)
        view[..., :VS[2]] = (torch.rand((n,) + VS, device=dev, generator=g) < 0.3).to(torch.bfloat16)
        view[..., 7] = 1.0
    else:
        view = (torch.rand((n,) + VS, device=dev, generator=g) < 0.3).float()
    feat = torch.rand((n, F), device=dev, generator=g)
    acts = torch.randint(A, (n,), dtype=torch.int32, device=dev, generator=g)
    rews = torch.rand(n, device=dev, generator=g)
    ids = (torch.arange(n, dtype=torch.int32, device=dev) % pad).contiguous()
    seg = np.stack([np.arange(K) * pad, np.full(K, agents)], axis=1).astype(np.int32)
    return ids, view, feat, acts, rews, seg


def summary(ms):
    return "%8.3f ms  (%.3f .. %.3f)" % (float(np.median(ms)), min(ms), max(ms))


def record_rates(args, K, cells, sides, dev):
    n_all = K * args.agents
    row_bytes = sides[0][1][0].numel() * sides[0][1].element_size() + F * 4 + 16
    for capacity in (1000, n_all):
        round_len = max(4, min(args.round_len, int(args.log_gb * 1e9 / 2 / (capacity * row_bytes))))
        recs = [DeviceEpisodesBuffer(capacity, capacity * round_len, s[1].shape[1:], (F,), view_dtype=s[1].dtype, device=dev) for s in sides]
        orders = [torch.randperm(s[0].shape[0], dtype=torch.int32, device=dev) for s in sides]

        def cycle():
            for rec, (ids, view, feat, acts, rews, seg), order in zip(recs, sides, orders):
                rec.record_step(ids, (view, feat), acts, rews, segments=seg, order=order)

        def a_round(out_round, out_steady):
            for rec in recs:
                rec.reset()
            torch.cuda.synchronize()
            first = timed(cycle)
            rest = timed(lambda: [cycle() for _ in range(round_len - 1)])
            out_round.append((first + rest) / round_len)
            out_steady.append(rest / (round_len - 1))
        t_end = time.perf_counter() + args.warm
        while time.perf_counter() < t_end:
            a_round([], [])
        whole, steady = [], []
        for _ in range(max(3, -(-args.calls // (2 * round_len)))):
            a_round(whole, steady)
        st = [rec.stats() for rec in recs]
        assert all(s["tracked"] == capacity and s["transitions"] == capacity * round_len and not s["overflow"] for s in st), st
        print("    capacity %7d, rounds of %2d cycles: record_step x 2 sides per cycle %s; behind the admitting cycle %s"
              % (capacity, round_len, summary(whole), summary(steady)), flush=True)
        del recs
        torch.cuda.empty_cache()
        if args.skip_host:
            continue
        # what it replaces: one EpisodesBuffer per world and side, fed with each world's rows of the same buffers
        per_world = -(-capacity // K) if capacity < n_all else args.agents
        alive = np.ones(args.agents, dtype=bool)
        host_len = min(round_len, 10)

        def host_round():
            bufs = [[utility.EpisodesBuffer(per_world) for _ in range(K)] for _ in sides]
            t0 = time.perf_counter()
            for _ in range(host_len):
                for per_side, (ids, view, feat, acts, rews, seg) in zip(bufs, sides):
                    for buf, (b, c) in zip(per_side, seg.tolist()):
                        buf.record_step(ids[b:b + c].cpu().numpy(), (view[b:b + c], feat[b:b + c]), acts[b:b + c], rews[b:b + c].cpu().numpy(), alive)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / host_len
        host_round()
        host = [host_round() for _ in range(3)]
        print("    capacity %7d: EpisodesBuffer.record_step x %d worlds x 2 sides per cycle %s  = %.0f x" %
              (capacity, K, summary(host), float(np.median(host)) / float(np.median(whole))), flush=True)


def copy_rates(args, cells, side, dev):
    ids, view, feat, acts, rews, seg = side
    n = view.shape[0]
    for k in (1000, 64000):
        if k > n:
            continue
        rec = DeviceEpisodesBuffer(k, k, view.shape[1:], (F,), view_dtype=view.dtype, device=dev)
        idx = torch.sort(torch.randperm(n, device=dev)[:k]).values
        idx32 = idx.to(torch.int32)
        counters = torch.zeros(8, dtype=torch.int32, device=dev)
        counters[4] = k                                          # (REPLAY_C_FILL(1): the fill behind call 0)
        outs = [torch.empty((k,) + t.shape[1:], dtype=t.dtype, device=dev) for t in (view, feat, acts, rews)]
        stream = torch.cuda.current_stream(dev).cuda_stream

        def kernel():
            rc = rec._lib.replay_copy(rec._st_ref, counters.data_ptr(), 0, k, view.data_ptr(), feat.data_ptr(), acts.data_ptr(), rews.data_ptr(),
                                      idx32.data_ptr(), stream)
            assert rc == 0

        def gathers():
            for t, o in zip((view, feat, acts, rews), outs):
                torch.index_select(t, 0, idx, out=o)
        kernel(); gathers()
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.uint8), o.view(torch.uint8)) for a, o in zip((rec._log_view, rec._log_feat, rec._log_act, rec._log_rew), outs))
        reps = max(20, min(2000, int(2e9 / (k * 5000))))
        for fn in (kernel, gathers):
            t_end = time.perf_counter() + args.warm
            while time.perf_counter() < t_end:
                fn()
                torch.cuda.synchronize()
        times = {"replay_copy": [], "index_select x 4": []}
        for _ in range(9):
            times["replay_copy"].append(timed(lambda: [kernel() for _ in range(reps)]) / reps)
            times["index_select x 4"].append(timed(lambda: [gathers() for _ in range(reps)]) / reps)
        moved = k * (view[0].numel() * view.element_size() + F * 4 + 8)
        for name, ms in times.items():
            med = float(np.median(ms))
            print("    k = %5d  %-17s %8.4f ms (%.4f .. %.4f, spread %4.1f %%)  %7.1f GB/s of rows, traffic %.1f %% of 8 TB/s"
                  % (k, name, med, min(ms), max(ms), 100 * (max(ms) - min(ms)) / med, moved / med / 1e6, 100 * 2 * moved / (med * 1e-3) / HBM))
        print("    k = %5d  replay_copy / index_select = %.3f" % (k, float(np.median(times["replay_copy"])) / float(np.median(times["index_select x 4"]))), flush=True)
        del rec, outs
        torch.cuda.empty_cache()


def packed_rates(args, K, sides, dev):
    n_all = K * args.agents
    row_bytes = sides[0][1][0].numel() * sides[0][1].element_size() + F * 4 + 16
    for capacity in (1000, n_all):
        if capacity * 50 * row_bytes * 2 > args.log_gb * 1e9:
            print("    capacity %7d: a 50-cycle round's log would pass %.0f GB -- not taken" % (capacity, args.log_gb))
            continue
        ids, view, feat, acts, rews, seg = sides[0]
        rec = DeviceEpisodesBuffer(capacity, capacity * 50, view.shape[1:], (F,), view_dtype=view.dtype, view_channels=VS[2], device=dev)
        ms = []
        for _ in range(6):
            rec.reset()
            for _ in range(50):
                rec.record_step(ids, (view, feat), acts, rews, segments=seg)
            rec.close(ids, seg)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = rec.packed()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            assert p[0].shape[0] == capacity * 50
            del p
        print("    capacity %7d: packed() of a 50-cycle round, %d transitions of one side %s (host clock, first call left out)"
              % (capacity, capacity * 50, summary(ms[1:])), flush=True)
        del rec
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("worlds", nargs="*", type=int, default=[8, 32, 128])
    ap.add_argument("--agents", type=int, default=2000, help="agents per side and world")
    ap.add_argument("--calls", type=int, default=1000, help="recorder calls per figure, at least")
    ap.add_argument("--round_len", type=int, default=50)
    ap.add_argument("--log_gb", type=float, default=24.0, help="the most device memory the two sides' logs may take")
    ap.add_argument("--warm", type=float, default=1.0, help="seconds of warm-up before a figure")
    ap.add_argument("--skip_host", action="store_true", help="leave out the EpisodesBuffer comparison")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for cells in (False, True):
        for K in args.worlds:
            sides = [side_buffers(K, args.agents, cells, dev, 10 * K + g) for g in range(2)]
            print("%s  %3d worlds x 2 x %d agents (%d rows a side)" % ("bf16 cells" if cells else "float32   ", K, args.agents, sides[0][0].shape[0]), flush=True)
            record_rates(args, K, cells, sides, dev)
            packed_rates(args, K, sides, dev)
            if K == max(args.worlds):
                copy_rates(args, cells, sides[0], dev)
            del sides
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
