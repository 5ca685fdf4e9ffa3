"""Development helper: the bits of the policy kernels.  A fixed, seeded list of cases goes through all twelve inference entries of
include/magent_policy.h -- the nine plain ones and the three segmented A2C ones --, called through the C-ABI as they are (the policy
classes of hip_policy.py only pack the weights), and every output array -- actions, Q, p, value, new states --, every packed weight
tensor and the seven *_act_bytes / *_workspace_bytes / *_workspace_bytes_seg sizes are written to an .npz as raw integer words.  Two such files of two builds (a commit and its parent; the emulated build and itself after a
refactor) must agree word for word: the kernels use no atomics, so their results are a function of the call's inputs alone.

    python tools/policy_bits.py LIB emu|cuda OUT.npz       LIB: a library with all of the entries -- the product library, or the emulated
                                                           build of all six policy sources (tests/helpers.py: policy_emu("policy"))
    python tools/policy_bits.py --compare A.npz B.npz      exit status 1 and the names of the arrays that differ, if any do

The cases are the smallest at which each shared block can still go wrong: n = 1, 33 (past a wave's 32 agents), 257 (past a workgroup's
256) and 2305 (10 agent groups: the XCD placement wraps past its first round of 8, the column sums take 10 blocks); for the DQN / DRQN
both view classes (13 x 13: the F13 kernels) with dueling on and off and every DRQN case called twice -- an empty table, then one that
holds duplicated ids, ids absent from the call and ids new to it; for the A2C an odd H W (the cell path's zero half k-step), rows that
are only 4-byte aligned, a shape without a cell entry, 1 and 64 features, 1, 16 and 31 actions, CommNet on and off and alone (n = 1); for the segmented A2C entries no segment at all over 33
rows, the table of tests/test_a2c_segments.py LAYOUTS["a"] (an agent alone, an empty segment, a segment across a 32-agent tile, one
whose sum blocks start off a multiple of 256), 256 one-row segments (the cap), and one table on a network without CommNet (ignored)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

# (view space, features, actions, n): DQN (dueling, as its kernels require)
DQN_CASES = [((13, 13, 7), 34, 21, 1), ((9, 9, 5), 20, 5, 33), ((13, 13, 7), 34, 21, 257), ((9, 9, 5), 20, 5, 2305)]
# (view space, features, actions, dueling, n): DRQN, two calls each
DRQN_CASES = [((9, 9, 5), 20, 5, False, 1), ((13, 13, 7), 34, 21, True, 33), ((13, 13, 7), 34, 21, False, 257), ((9, 9, 5), 20, 5, True, 2305)]
# (view space, features, actions, CommNet, n): A2C
A2C_CASES = [((5, 5, 5), 1, 1, True, 1), ((13, 13, 7), 64, 16, False, 33), ((3, 3, 9), 64, 1, True, 257), ((13, 13, 7), 1, 31, True, 257),
             ((3, 3, 9), 1, 16, False, 2305), ((5, 5, 5), 64, 31, True, 2305)]
# (view space, features, actions, CommNet, n, [(begin, count)]): the segmented A2C entries
A2C_SEG_CASES = [((5, 5, 5), 1, 16, True, 33, []), ((5, 5, 3), 7, 9, True, 322, [(4, 1), (8, 0), (8, 33), (52, 257), (312, 2)]),
                 ((3, 3, 9), 64, 31, True, 256, [(r, 1) for r in range(256)]), ((13, 13, 7), 34, 21, False, 33, [(1, 8), (12, 20)])]


def words(t):
    """a tensor's bits as an unsigned integer array of its element size"""
    import torch
    t = t.detach().contiguous().cpu()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy().view("u%d" % t.element_size())


def inputs(vs, feat, n, seed, dev):
    """observation-like views (sparse, fractions), their bf16 cells where a cell holds the channels, features and uniform numbers"""
    import torch
    g = torch.Generator().manual_seed(seed)
    view = (torch.rand((n,) + vs, generator=g) < 0.3).float() * torch.rand((n,) + vs, generator=g)
    featv = torch.rand((n, feat), generator=g) * 2 - 0.5
    u = torch.rand(n, generator=g)
    cells = None
    if vs[2] <= 7:
        cells = torch.zeros((n,) + vs[:2] + (8,), dtype=torch.bfloat16)
        cells[..., :vs[2]] = view.to(torch.bfloat16)
        cells[..., 7] = 1.0
        cells = cells.to(dev)
    return view.to(dev), cells, featv.to(dev), u.to(dev)


def scaled(net, seed_scale=3.0):
    """larger weights than the default init: every layer matters in the outputs (the tests' networks)"""
    import torch
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(seed_scale)
    return net


def second_ids(ids, n):
    """the ids of a second call against the table of `ids`: every other one of the first call's (the duplicated one among them), then
    ids new to the table; the rest of the first call's are absent"""
    import torch
    keep = ids[::2]
    return torch.cat([keep, torch.arange(n - keep.numel(), dtype=torch.int32) + 100000])[torch.randperm(n, generator=torch.Generator().manual_seed(n))]


def run(lib, dev, out):
    import torch
    from magent_amd.builtin.torch_model import hip_policy as hp
    from magent_amd.builtin.torch_model.a2c import _ActorCritic
    from magent_amd.builtin.torch_model.dqn import _QNet
    from magent_amd.builtin.torch_model.drqn import _RecurrentQNet
    ref, ptr = ctypes.byref, lambda t: None if t is None else t.data_ptr()

    def check(rc, what):
        if dev.type == "cuda":
            torch.cuda.synchronize()
        if rc != 0:
            raise RuntimeError("%s failed (%d)" % (what, rc))

    def size(name, shape, *args):
        nb = ctypes.c_size_t(0)
        check(getattr(lib, name)(ref(shape), *args, ref(nb)), name)
        out["%s/%s" % (name, "-".join(str(a) for a in (shape.view_h, shape.view_w, shape.view_c, shape.feat, shape.n_action) + args))] = np.uint64(nb.value)
        return torch.zeros(nb.value + 256, dtype=torch.uint8, device=dev)

    def packed(pol, tag):
        pol.pack()
        for k, t in pol._packed.items():
            out["%s/packed/%s" % (tag, k)] = words(t)
        return pol

    def entries(pol, pairs, cells):
        """(entry, views) for the float32 views and, where the shape has them, the cells"""
        return [(e, v) for e, v in pairs if v is not None and (not e.endswith("_bf16") or cells)]

    for k, (vs, feat, A, n) in enumerate(DQN_CASES):
        torch.manual_seed(100 + k)
        net = scaled(_QNet(vs, (feat,), A, True, True)).to(dev)
        view, cells, featv, _ = inputs(vs, feat, n, 200 + k, dev)
        for cls, pairs, bytes_fn in ((hp.HipDqnPolicy, [("policy_dqn_infer", view), ("policy_dqn_infer_bf16", cells)], "policy_dqn_act_bytes"),
                                     (hp.HipDqnPolicyF32, [("policy_dqn_infer_f32", view)], "policy_dqn_f32_act_bytes")):
            pol = packed(cls(net, vs, (feat,), A, dev), "dqn%d/%s" % (k, cls.__name__))
            work = size(bytes_fn, pol.shape, n)
            for entry, v in pairs:
                actions, q = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros((n, A), device=dev)
                check(getattr(lib, entry)(ref(pol.shape), ref(pol._w), ptr(v), ptr(featv), n, ptr(work), ptr(actions), ptr(q), None), entry)
                out["%s/dqn%d/actions" % (entry, k)], out["%s/dqn%d/q" % (entry, k)] = words(actions), words(q)

    for k, (vs, feat, A, dueling, n) in enumerate(DRQN_CASES):
        torch.manual_seed(300 + k)
        net = scaled(_RecurrentQNet(vs, (feat,), A, dueling)).to(dev)
        ids1 = torch.arange(n, dtype=torch.int32) * 3 + 5
        if n > 4:
            ids1[n // 2 + 1] = ids1[2]         # a duplicated id: the table keeps both rows, a look-up takes the last
        calls = [(ids1, inputs(vs, feat, n, 400 + k, dev)), (second_ids(ids1, n), inputs(vs, feat, n, 500 + k, dev))]
        for cls, names, bytes_fn in ((hp.HipDrqnPolicy, ["policy_drqn_infer", "policy_drqn_infer_bf16"], "policy_drqn_workspace_bytes"),
                                     (hp.HipDrqnPolicyF32, ["policy_drqn_infer_f32"], "policy_drqn_f32_workspace_bytes")):
            pol = packed(cls(net, vs, (feat,), A, dev), "drqn%d/%s" % (k, cls.__name__))
            work = size(bytes_fn, pol.shape, n)
            for entry in names:
                table = (None, None, None, 0)
                for c, (ids, (view, cells, featv, _)) in enumerate(calls):
                    ids = ids.to(dev)
                    actions, q = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros((n, A), device=dev)
                    states = torch.zeros((n, 512), device=dev)
                    v = cells if entry.endswith("_bf16") else view
                    check(getattr(lib, entry)(ref(pol.shape), ref(pol._w), ptr(v), ptr(featv), n, ptr(ids), ptr(table[0]), ptr(table[1]), ptr(table[2]),
                                              table[3], ptr(states), ptr(work), ptr(actions), ptr(q), None), entry)
                    tag = "%s/drqn%d/call%d" % (entry, k, c)
                    out[tag + "/actions"], out[tag + "/q"], out[tag + "/states"] = words(actions), words(q), words(states)
                    srt, perm = torch.sort(ids, stable=True)
                    table = (srt, perm.to(torch.int32), states, n)

    def a2c(tag, seed, vs, feat, A, comm, n, suffix="", table=()):
        """every A2C entry (+ suffix) on one seeded network and n rows; table: a segmented entry's begin, count, n_seg"""
        torch.manual_seed(seed)
        net = scaled(_ActorCritic(vs, (feat,), A, comm)).to(dev)
        view, cells, featv, u = inputs(vs, feat, n, seed + 100, dev)
        for cls, pairs, bytes_fn in ((hp.HipA2cPolicy, [("policy_a2c_infer", view), ("policy_a2c_infer_bf16", cells)], "policy_a2c_workspace_bytes"),
                                     (hp.HipA2cPolicyF32, [("policy_a2c_infer_f32", view)], "policy_a2c_f32_workspace_bytes")):
            pol = packed(cls(net, vs, (feat,), A, dev), "%s/%s" % (tag, cls.__name__))
            work = size(bytes_fn + suffix, pol.shape, n, int(comm), *table[2:])
            for entry, v in entries(pol, pairs, getattr(pol, "cells", False)):
                actions, p, value = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros((n, A), device=dev), torch.zeros(n, device=dev)
                check(getattr(lib, entry + suffix)(ref(pol.shape), ref(pol._w), ptr(v), ptr(featv), n, ptr(u), ptr(work), ptr(actions), ptr(p),
                                                   ptr(value), None, *table), entry + suffix)
                out["%s%s/%s/actions" % (entry, suffix, tag)], out["%s%s/%s/p" % (entry, suffix, tag)] = words(actions), words(p)
                out["%s%s/%s/value" % (entry, suffix, tag)] = words(value)

    for k, (vs, feat, A, comm, n) in enumerate(A2C_CASES):
        a2c("a2c%d" % k, 600 + k, vs, feat, A, comm, n)
    for k, (vs, feat, A, comm, n, seg) in enumerate(A2C_SEG_CASES):
        ints = lambda v: (ctypes.c_int32 * max(len(v), 1))(*v)
        a2c("a2cseg%d" % k, 800 + k, vs, feat, A, comm, n, "_seg", (ints([b for b, _ in seg]), ints([c for _, c in seg]), len(seg)))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        if A[k].shape != B[k].shape or A[k].dtype != B[k].dtype or not np.array_equal(A[k], B[k]):
            bad.append(k)
    print("%d arrays in %s, %d in %s: %s" % (len(A.files), a, len(B.files), b, "equal word for word" if not bad else "%d DIFFER" % len(bad)))
    for k in bad:
        print("  differs:", k)
    return 1 if bad else 0


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 4 or sys.argv[2] not in ("emu", "cuda"):
        sys.exit(__doc__)
    import torch
    from magent_amd import c_lib
    lib = c_lib.declare_policy(ctypes.CDLL(os.path.abspath(sys.argv[1]), mode=os.RTLD_LOCAL))
    out = {}
    run(lib, torch.device("cpu") if sys.argv[2] == "emu" else torch.device("cuda", 0), out)
    np.savez(sys.argv[3], **out)
    print("%d arrays -> %s" % (len(out), sys.argv[3]))


if __name__ == "__main__":
    main()
