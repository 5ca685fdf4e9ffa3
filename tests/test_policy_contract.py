"""The DQN inference kernels (magent_amd/csrc/policy_f32.hip, policy.hip) against a float64 NumPy restatement of the network
(helpers.np_qnet), over the whole supported shape region, on non-finite inputs and weights, on exact ties, and at the edges of the
buffers they are given.  Every check runs twice: on the CPU emulator (tests/hipemu, the `emu` leg, no GPU needed) and on the MI355X
(`gpu`, marked).  Both legs call the C-ABI through ctypes directly (policy_dqn_infer_f32 / policy_dqn_infer / policy_dqn_infer_bf16),
chunked as HipDqnPolicy*.infer chunks; the GPU leg also goes through the wrappers.

The non-finite contract: an agent's Q row from the kernels is non-finite exactly where the network's row is (NaN where
it is NaN); its action is torch.argmax of that row -- the first NaN, 0 for a row of NaNs --, always in [0, n_action), and equal to the
argmax of the kernel's own Q output."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H

HERE = os.path.dirname(os.path.abspath(__file__))
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------- the two legs
# `emu`: the engine-wide emulated build on CPU tensors (three workgroups walk every tile); `gpu`: the product library on cuda:0
leg, LEGS = H.policy_legs(H.ensure_emu, tune="policy_grid=3")
make_inputs, cells_of = H.make_policy_inputs, H.cells_of


def make_qnet(view_space, feat, n_action, seed, dev="cpu", scale=3.0):
    import torch
    from magent_amd.builtin.torch_model.dqn import _QNet
    torch.manual_seed(seed)
    q = _QNet(view_space, (feat,), n_action, True, True)
    with torch.no_grad():
        for p in q.parameters():          # larger weights than the default init: every layer's output matters in Q
            p.mul_(scale)
    return q.to(dev)


def policy(lg, kind, qnet, view_space, feat, n_action):
    from magent_amd.builtin.torch_model.hip_policy import HipDqnPolicy, HipDqnPolicyF32
    cls = HipDqnPolicyF32 if kind == "f32" else HipDqnPolicy
    pol = cls(qnet, view_space, (feat,), n_action, lg.dev)
    pol.pack()
    assert all(t.device.type == lg.dev.type for t in pol._packed.values())       # (the kernels dereference these addresses)
    return pol


def act_bytes(lg, kind, pol, n):
    nb = ctypes.c_size_t(0)
    (lg.lib.policy_dqn_f32_act_bytes if kind == "f32" else lg.lib.policy_dqn_act_bytes)(ctypes.byref(pol.shape), ctypes.c_int(n), ctypes.byref(nb))
    return nb.value


def call(lg, kind, pol, view, featv, n, work, actions, q):
    """one C-ABI call on raw addresses (view/feat/actions/q: tensors or ints)"""
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    fn = {"f32": lg.lib.policy_dqn_infer_f32, "bf16": lg.lib.policy_dqn_infer, "cells": lg.lib.policy_dqn_infer_bf16}[kind]
    rc = fn(ctypes.byref(pol.shape), ctypes.byref(pol._w), ctypes.c_void_p(ptr(view)), ctypes.c_void_p(ptr(featv)), ctypes.c_int(n),
            ctypes.c_void_p(ptr(work)), ctypes.c_void_p(ptr(actions)), ctypes.c_void_p(ptr(q)), None)
    return rc


def infer(lg, kind, pol, view, featv, n, want_q=True, chunk=None):
    """actions (int32 [n]) and Q ([n][A] or None) of the first n agents, in chunks of `chunk` agents as the wrappers call the library"""
    import torch
    chunk = chunk or n
    view = view.to(lg.dev).contiguous()
    featv = featv.to(lg.dev).contiguous()
    if kind == "cells":
        view = cells_of(view)
    A = pol.shape.n_action
    actions = torch.full((n,), -7, dtype=torch.int32, device=lg.dev)
    q = torch.full((n, A), -77.0, device=lg.dev) if want_q else None
    work = torch.empty(act_bytes(lg, kind, pol, min(n, chunk)), dtype=torch.uint8, device=lg.dev)
    for beg in range(0, n, chunk):
        m = min(chunk, n - beg)
        rc = call(lg, kind, pol, view[beg:].data_ptr(), featv[beg:].data_ptr(), m, work, actions[beg:].data_ptr(),
                  q[beg:].data_ptr() if want_q else None)
        assert rc == 0, rc
    lg.sync()
    return actions.cpu(), (q.cpu() if want_q else None)


# ---------------------------------------------------------------------------------------------------- comparison with float64
WORST = {}


def check(kind, qnet, view, featv, n, actions, q, tag=""):
    """the kernel's (actions, Q) of n agents against the float64 network: the non-finite contract, then per entry

      f32 : |Q - Q64| <= c 2^-24 Qmag   (helpers.f32_error_bound: holds for ANY float32 evaluation order -- a theorem, loose: Qmag sums
                                          magnitudes through five layers) and
            |Q - Q64| <= 1e-5 max|Q64| + 1e-7 (the working bound, batch-wide as in tests/test_policy_emu.py: the Qmag bound above is a
                                               theorem but three to four orders of magnitude above what float32 round-off reaches)
      bf16: |Q - Q64(bf16 rounding points)| <= 2e-3 max|Q64| + 2e-3 (tests/test_policy.py's bound)"""
    import torch
    vs = tuple(view.shape[1:])
    F, A = featv.shape[1], q.shape[1]
    q64, qmag = H.qnet_f64(qnet, view[:n].cpu(), featv[:n].cpu(), bf16=(kind != "f32"))
    qk = q.double().numpy()
    a = actions.long()
    # every action in range, and the argmax (torch's: the first NaN, the first of equal maxima) of the kernel's own Q
    assert bool(((a >= 0) & (a < A)).all()), (tag, a.min().item(), a.max().item())
    assert torch.equal(a, q.argmax(dim=1)), tag
    # Q is non-finite exactly where the network's is, NaN exactly where it is NaN; such rows act like the PyTorch path
    fin64 = np.isfinite(q64)
    assert np.array_equal(np.isfinite(qk), fin64), (tag, np.argwhere(np.isfinite(qk) != fin64)[:8])
    assert np.array_equal(np.isnan(qk), np.isnan(q64)), tag
    assert np.array_equal(np.isposinf(qk), np.isposinf(q64)) and np.array_equal(np.isneginf(qk), np.isneginf(q64)), tag
    bad_rows = ~fin64.all(axis=1)
    if bad_rows.any():
        assert torch.equal(a[torch.from_numpy(bad_rows)], torch.from_numpy(q64[bad_rows]).argmax(dim=1)), tag
    ok = fin64.all(axis=1)
    if not ok.any():
        return
    d = np.abs(qk[ok] - q64[ok])
    if kind == "f32":
        c = H.f32_error_bound(vs, F, A)
        bound = c * 2.0 ** -24 * qmag[ok]
        ratio = float((d / bound).max())
        assert ratio <= 1.0, (tag, ratio)
        tight = float((d / (1e-5 * np.abs(q64[ok]).max() + 1e-7)).max())
        assert tight <= 1.0, (tag, tight, float(d.max()))
        WORST[kind] = max(WORST.get(kind, (0, 0)), (ratio, tight))
        print("%s %s: worst |Q - Q64| / (c 2^-24 Qmag) = %.2e (c = %d), / (1e-5 max|Q64|) = %.2e" % (tag, kind, ratio, c, tight))
    else:
        scale = float(np.abs(q64[ok]).max())
        err = float(d.max())
        assert err <= 2e-3 * scale + 2e-3, (tag, err, scale)
        print("%s %s: max |Q - Q64| = %.2e of max |Q64| %.3f" % (tag, kind, err, scale))


# ---------------------------------------------------------------------------------------------------- 2. the supported region
def _pitch_for(least, ta):
    want = 16 // ta
    return least + ((want - least % 16) % 16 + 16) % 16


def f32_conv_ta(h, w):
    """policy_f32.hip's conv_lds / conv_ta: agents per conv tile (4, or 2 where four agents' LDS images pass 160 KB)"""
    lds = lambda ta: (2 * ta * _pitch_for(h * w + 2, ta) + 8 * ta * _pitch_for((h - 2) * w, ta) + 45 * 64) * 16 + 128
    return 4 if lds(4) <= 160 * 1024 else 2


def f32_supported(h, w, c, feat, n_action):
    """policy_dqn_f32_supported, restated"""
    ta = f32_conv_ta(h, w)
    lds = (2 * ta * _pitch_for(h * w + 2, ta) + 8 * ta * _pitch_for((h - 2) * w, ta) + 45 * 64) * 16 + 128
    return 1 <= c <= 7 and h >= 5 and w >= 5 and h * w * ta <= 2 * 512 and 1 <= feat and (feat + 7) // 8 * 8 <= 56 and 1 <= n_action <= 31 and lds <= 160 * 1024


def bf16_supported(h, w, c, feat, n_action):
    """policy_dqn_supported, restated"""
    return 1 <= c <= 7 and h >= 5 and w >= 5 and h * w * 4 <= 4 * 256 and 1 <= feat <= 64 and 1 <= n_action <= 31


# (view_space, feat, n_action, n, chunk): the edges of policy_dqn_f32_supported.  TA = 4 up to 13 x 13 / 5 x 51 (H W <= 255), TA = 2 from
# 14 x 14 / 39 x 5 on; H W > 256 (the second window cell per thread of the TA = 2 prefetch) from 17 x 16 to 510 cells; H2 W2 odd (a half
# last K-chunk of the head) and even; feat 1, 8, 9, 55, 56; n_action 1, 2, 15, 16, 17, 31 (the head's two 16-output halves); n of 1,
# TA +- 1, 128 +- 1 (one head group) and a partial last chunk
F32_CASES = [((5, 5, 1), 1, 1, 1, None), ((13, 13, 7), 34, 21, 5, None), ((9, 9, 2), 8, 2, 3, None), ((13, 12, 3), 9, 15, 129, 100),
             ((5, 51, 4), 55, 16, 7, None), ((12, 13, 5), 56, 17, 127, None), ((14, 14, 6), 17, 31, 3, 2), ((39, 5, 2), 49, 31, 5, None),
             ((15, 15, 7), 34, 33 - 2, 10, None), ((17, 16, 6), 33, 9, 3, None), ((19, 19, 7), 34, 21, 9, 4), ((11, 38, 3), 56, 1, 4, None),
             ((31, 11, 5), 25, 17, 2, None), ((5, 102, 7), 8, 16, 2, None), ((74, 5, 1), 3, 15, 1, None), ((21, 18, 4), 12, 30, 3, None)]
BF16_CASES = [((5, 5, 1), 1, 1, 1, None), ((13, 13, 7), 34, 21, 5, None), ((9, 9, 2), 16, 2, 3, None), ((13, 12, 3), 17, 15, 129, 100),
              ((5, 51, 4), 63, 16, 7, None), ((16, 16, 7), 64, 17, 5, 4), ((51, 5, 6), 1, 31, 3, None), ((12, 21, 5), 40, 31, 127, None)]


def _sweep(lg, kind, case, seed):
    vs, feat, A, n, chunk = case
    assert (f32_supported if kind == "f32" else bf16_supported)(vs[0], vs[1], vs[2], feat, A), case
    qnet = make_qnet(vs, feat, A, seed, lg.dev)
    view, featv = make_inputs(vs, feat, n, seed, extra=3, fill=NAN)       # (rows behind the n agents: NaN -- none may be read)
    pol = policy(lg, "f32" if kind == "f32" else "bf16", qnet, vs, feat, A)
    actions, q = infer(lg, kind, pol, view, featv, n, chunk=chunk)
    tag = "%s %s feat %d A %d n %d chunk %s%s" % (lg.name, vs, feat, A, n, chunk, " TA %d" % f32_conv_ta(*vs[:2]) if kind == "f32" else "")
    check(kind, qnet, view, featv, n, actions, q, tag)
    a2, _ = infer(lg, kind, pol, view, featv, n, want_q=False, chunk=chunk)      # (the argmax is taken without a Q output too)
    assert torch_equal(a2, actions), tag


def torch_equal(a, b):
    import torch
    return torch.equal(a, b)


@pytest.mark.parametrize("lg", LEGS)
@pytest.mark.parametrize("case", F32_CASES, ids=lambda c: "%dx%dx%d-f%d-a%d-n%d" % (c[0] + c[1:4]))
def test_f32_policy_against_float64_over_the_supported_region(lg, case):
    _sweep(leg(lg), "f32", case, 100 + F32_CASES.index(case))


@pytest.mark.parametrize("lg", LEGS)
@pytest.mark.parametrize("case", BF16_CASES, ids=lambda c: "%dx%dx%d-f%d-a%d-n%d" % (c[0] + c[1:4]))
def test_bf16_policy_against_float64_over_the_supported_region(lg, case):
    _sweep(leg(lg), "bf16", case, 200 + BF16_CASES.index(case))
    if lg == "emu" or case[3] <= 7:      # the bf16-cell entry point: the same operands reach the same MFMAs
        _sweep(leg(lg), "cells", case, 200 + BF16_CASES.index(case))


def test_emulated_f32_policy_random_shapes():
    """seeded random shapes inside policy_dqn_f32_supported (sides 5..40, 1..7 channels, 1..56 features, 1..31 actions), agent counts that
    leave partial conv tiles and partial head groups"""
    rs = np.random.RandomState(2026)
    done = 0
    while done < 6:
        h, w = int(rs.randint(5, 41)), int(rs.randint(5, 41))
        c, feat, A = int(rs.randint(1, 8)), int(rs.randint(1, 57)), int(rs.randint(1, 32))
        if not f32_supported(h, w, c, feat, A):
            continue
        n = int(rs.randint(1, 12)) if h * w > 150 else int(rs.randint(1, 140))
        _sweep(leg("emu"), "f32", ((h, w, c), feat, A, n, None), 300 + done)
        done += 1


def test_supported_functions_are_their_restatements():
    """policy_dqn_f32_supported / policy_dqn_supported over a grid around the edges of the region: the restatements above (which the
    sweeps and the GPU leg's every-shape test enumerate) are the functions themselves"""
    lg = leg("emu")
    from magent_amd.builtin.torch_model.hip_policy import _Shape
    seen = 0
    for h in range(3, 110):
        for w in range(3, 110):
            if h * w > 700:
                continue
            for c, feat, A in ((7, 34, 21), (1, 56, 31), (8, 34, 21), (0, 34, 21), (7, 57, 21), (7, 64, 1), (7, 65, 21), (7, 34, 32), (7, 34, 0), (7, 0, 5)):
                s = _Shape(h, w, c, feat, A)
                assert bool(lg.lib.policy_dqn_f32_supported(ctypes.byref(s))) == f32_supported(h, w, c, feat, A), (h, w, c, feat, A)
                assert bool(lg.lib.policy_dqn_supported(ctypes.byref(s))) == bf16_supported(h, w, c, feat, A), (h, w, c, feat, A)
                seen += 1
    assert seen > 10000
    assert sum(f32_supported(h, w, 7, 34, 21) for h in range(5, 110) for w in range(5, 110)) == 847


@pytest.mark.gpu
def test_every_supported_view_shape_runs_on_the_gpu():
    """every (H, W) that policy_dqn_f32_supported accepts (847 of them: 5 x 5 .. 5 x 102, 74 x 5, 21 x 18 ...) and every one that
    policy_dqn_supported accepts: rc 0, and Q of two agents within the bounds of `check` against float64"""
    import torch
    lg = leg("gpu")
    shapes = [(h, w) for h in range(5, 110) for w in range(5, 110) if f32_supported(h, w, 7, 34, 21) or bf16_supported(h, w, 7, 34, 21)]
    for i, (h, w) in enumerate(shapes):
        vs = (h, w, 1 + i % 7)
        with torch.device(lg.dev):
            qnet = make_qnet(vs, 34, 21, i, lg.dev)
        view, featv = make_inputs(vs, 34, 2, i)
        for kind in ("f32", "bf16"):
            if not (f32_supported if kind == "f32" else bf16_supported)(h, w, vs[2], 34, 21):
                continue
            pol = policy(lg, kind, qnet, vs, 34, 21)
            actions, q = infer(lg, kind, pol, view, featv, 2)
            check(kind, qnet, view, featv, 2, actions, q, "%s every shape" % (vs,))


@pytest.mark.gpu
@pytest.mark.parametrize("vs,feat,A", [((13, 13, 7), 57, 21), ((13, 13, 7), 34, 32), ((13, 13, 8), 34, 21), ((22, 23, 7), 34, 21), ((19, 27, 7), 34, 21)])
def test_first_shape_past_each_limit_falls_back_to_pytorch(vs, feat, A):
    """feat 57 (f32: the embedding's LDS image holds 56), 32 actions, 8 channels, the first rejected H W (22 x 23: 506 cells but 160 KB of
    LDS exceeded; 19 x 27: 513 cells): DeepQNetwork keeps the PyTorch forward pass (m._hip is None) and its actions come out"""
    import torch
    from magent_amd.builtin.torch_model import DeepQNetwork
    assert not f32_supported(vs[0], vs[1], vs[2], feat, A)

    class _Env(object):        # (DeepQNetwork asks its environment for the action space only when the spaces are given)
        def get_action_space(self, h):
            return (A,)

        def get_view_space(self, h):
            return vs

        def get_feature_space(self, h):
            return (feat,)
    m = DeepQNetwork(_Env(), 0, "past", memory_size=16, custom_view_space=vs, custom_feature_space=(feat,))
    assert m._hip is None
    view, featv = make_inputs(vs, feat, 5, 1)
    a = m.infer_action((view.cuda(), featv.cuda()), None, policy="greedy")
    with torch.no_grad():
        ref = m.qnet(view.cuda(), featv.cuda()).argmax(dim=1)
    assert torch.equal(a.long(), ref)


# ---------------------------------------------------------------------------------------------------- 3. non-finite inputs and weights
def _poison_slots(ta, n, chunk):
    """agents at the first and last slot of a conv tile, of a 128-agent head group and of a wrapper chunk"""
    return sorted({0, ta - 1, ta, 2 * ta - 1, 127, 128, n - 1, chunk - 1, chunk} & set(range(n)))


NONFINITE_CASES = [("cell", NAN), ("channel", NAN), ("feature", NAN), ("cell", INF), ("cell", -INF), ("feature0", NAN)]


def _nonfinite_inputs(rot, vs, feat, n, seed, slots):
    """inputs with slot j's agent poisoned by NONFINITE_CASES[(j + rot) % 6]; NaN in every row behind the n agents"""
    view, featv = make_inputs(vs, feat, n, seed, extra=5, fill=NAN)
    rs = np.random.RandomState(seed)
    for j, a in enumerate(slots):
        poison, val = NONFINITE_CASES[(j + rot) % len(NONFINITE_CASES)]
        y, x, c = int(rs.randint(vs[0])), int(rs.randint(vs[1])), int(rs.randint(vs[2]))
        if poison == "cell":
            view[a, y, x, c] = val
        elif poison == "channel":                # the minimap of an empty group: 0/0 in every cell of one channel
            view[a, :, :, vs[2] - 1] = val
        elif poison == "feature":
            featv[a, feat - 1] = val
        else:                                    # feature 0: the one a read past a row's end would pick up from the row behind
            featv[a, 0] = val
    return view, featv


@pytest.mark.parametrize("lg", LEGS)
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("vs,feat,A,n,chunk", [((13, 13, 7), 34, 21, 137, 132), ((15, 15, 5), 19, 17, 137, 131)])
def test_nonfinite_inputs_stay_in_their_agents_rows(lg, kind, vs, feat, A, n, chunk):
    """NaN in one view cell, in a whole channel (the empty group's minimap), in the first or the last feature, +-inf in a cell -- at the
    first and last slot of a conv tile, of a 128-agent head group and of a chunk, with NaN in every input row behind the n agents: only the poisoned
    agents' rows are non-finite (a kernel that read a neighbour's feature into a pad column, or a cell of the next agent, would spread
    them: the zero-padded weights hide such reads from finite inputs), those rows are what the network gives, and their actions are
    torch.argmax of them"""
    lgo = leg(lg)
    ta = f32_conv_ta(*vs[:2]) if kind == "f32" else 4
    slots = _poison_slots(ta, n, chunk)
    qnet = make_qnet(vs, feat, A, 7, lgo.dev)
    pol = policy(lgo, kind, qnet, vs, feat, A)
    kinds = [kind] + (["cells"] if kind == "bf16" else [])
    for rot in range(len(NONFINITE_CASES) if lg == "gpu" else 2):       # (every slot sees every poison on the GPU, two of them on the emulator)
        view, featv = _nonfinite_inputs(rot, vs, feat, n, 50 + rot, slots)
        for k in kinds:
            actions, q = infer(lgo, k, pol, view, featv, n, chunk=chunk)
            check(k, qnet, view, featv, n, actions, q, "%s %s rotation %d" % (lg, vs, rot))
            rows = (~np.isfinite(q.numpy())).any(axis=1)
            assert sorted(np.nonzero(rows)[0].tolist()) == slots, (rot, np.nonzero(rows)[0].tolist())


@pytest.mark.parametrize("lg", LEGS)
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_nonfinite_weights(lg, kind):
    """a diverged network: NaN in value.weight, in one advantage.weight entry, in one conv1 / conv2 weight -- every Q row NaN, every
    action 0 (torch.argmax of a row of NaNs), as on the PyTorch path; +inf in the value bias: every row +inf, action 0"""
    import torch
    lgo = leg(lg)
    vs, feat, A, n = (13, 13, 7), 34, 21, 37
    view, featv = make_inputs(vs, feat, n, 3)
    for what in ("value.weight", "advantage.weight", "conv1.weight", "conv2.weight", "value.bias"):
        qnet = make_qnet(vs, feat, A, 11, lgo.dev)
        with torch.no_grad():
            p = dict(qnet.named_parameters())[what]
            if what == "value.weight":
                p.fill_(NAN)
            elif what == "value.bias":
                p.fill_(INF)
            else:
                p.view(-1)[5] = NAN
        pol = policy(lgo, kind, qnet, vs, feat, A)
        for k in [kind] + (["cells"] if kind == "bf16" else []):
            actions, q = infer(lgo, k, pol, view, featv, n)
            check(k, qnet, view, featv, n, actions, q, "%s %s" % (lg, what))
            assert bool((actions == 0).all()), (what, actions.tolist())
            assert (bool(torch.isnan(q).all()) if what != "value.bias" else bool(torch.isposinf(q).all())), what
            if what == "value.weight":
                with torch.no_grad():
                    assert bool((qnet(view.to(lgo.dev), featv.to(lgo.dev)).argmax(dim=1) == 0).all())          # (the PyTorch path acts the same)


# ---------------------------------------------------------------------------------------------------- 4. exact ties
def _tie_qnet(vs, feat, A, i, j, seed):
    """advantage rows i and j equal, every other row below them by a positive margin on every hidden unit (the hidden units are relu
    outputs, >= 0, and not all zero): the best two advantages -- and Q values -- of every agent tie exactly at i and j"""
    import torch
    qnet = make_qnet(vs, feat, A, seed)
    with torch.no_grad():
        w = qnet.advantage.weight
        g = torch.Generator().manual_seed(seed)
        base = w[i].clone()
        for r in range(A):
            w[r] = base - (0.02 + 0.05 * torch.rand(w.shape[1], generator=g))
        w[i] = base
        w[j] = base
    return qnet


TIE_PAIRS = [(1, 9), (5, 13), (2, 6), (4, 8), (0, 20)]      # one 16-output half (lane group 0, 1); across the halves either way; 0 and A - 1


def _ties(lg, kind, n=23):
    import torch
    lgo = leg(lg)
    vs, feat, A = (9, 9, 7), 13, 21
    view, featv = make_inputs(vs, feat, n, 8)
    for i, j in TIE_PAIRS:
        qnet = _tie_qnet(vs, feat, A, i, j, 40 + i).to(lgo.dev)
        q64, _ = H.qnet_f64(qnet, view[:n], featv[:n], bf16=(kind != "f32"))
        assert (q64.argmax(axis=1) == min(i, j)).all() and (q64[:, i] == q64[:, j]).all()
        pol = policy(lgo, "f32" if kind == "f32" else "bf16", qnet, vs, feat, A)
        actions, q = infer(lgo, kind, pol, view, featv, n)
        assert bool((q[:, i] == q[:, j]).all()), (kind, i, j)
        assert bool((actions == min(i, j)).all()), (kind, i, j, actions.tolist())
        assert torch.equal(actions.long(), q.argmax(dim=1))
        a2, _ = infer(lgo, kind, pol, view, featv, n, want_q=False)
        assert bool((a2 == min(i, j)).all()), (kind, i, j)


@pytest.mark.parametrize("lg", LEGS)
@pytest.mark.parametrize("kind", ["f32", "bf16", "cells"])
def test_exact_ties_go_to_the_lower_index(lg, kind):
    """the best two advantages of every agent tie exactly: the action is the lower index, as torch.argmax returns -- within one half of
    the head's outputs, across the two halves that the head merges with __shfl_xor(.., 32) in either order, at outputs 0 and A - 1"""
    _ties(lg, kind)


def test_emulated_ties_and_nonfinite_in_scrambled_order():
    """HIPEMU_SCRAMBLE: the lanes and waves run in a pseudo-random order that changes at every scheduling pass -- the tie-break and the
    non-finite contract must not care (a process of its own: the variable is read at the first launch)"""
    code = ("import sys; sys.path.insert(0, %r); import test_policy_contract as T\n"
            "for k in ('f32', 'bf16'):\n"
            "    T._ties('emu', k, n=9)\n"
            "    T.test_nonfinite_inputs_stay_in_their_agents_rows('emu', k, (9, 9, 7), 21, 17, 133, 131)\n"
            "print('scrambled ok')\n") % HERE
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HIPEMU_SCRAMBLE="31", OMP_NUM_THREADS="1"), capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0 and "scrambled ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------- 5. writes stay inside their buffers
PAD = 4096


def _guarded(lg, nbytes, pattern):
    """a uint8 tensor of nbytes + 2 PAD bytes filled with a sentinel pattern; the region handed to the kernel starts at PAD"""
    import torch
    t = torch.tensor(bytearray(pattern * ((nbytes + 2 * PAD) // len(pattern) + 1))[:nbytes + 2 * PAD], dtype=torch.uint8).to(lg.dev)
    return t


def _edges_case(lg, kind, vs, feat, A, ns):
    import torch
    lgo = leg(lg)
    qnet = make_qnet(vs, feat, A, 5, lgo.dev)
    pol = policy(lgo, "f32" if kind == "f32" else "bf16", qnet, vs, feat, A)
    nmax = max(ns)
    view, featv = make_inputs(vs, feat, nmax, 6)
    v = (cells_of(view) if kind == "cells" else view).to(lgo.dev).contiguous()
    f = featv.to(lgo.dev).contiguous()
    fresh = {}
    for n in ns:
        for want_q in (True, False):
            wb = act_bytes(lgo, kind, pol, n)
            work = _guarded(lgo, wb, b"\xA5\x5A\xC3\x3C")
            act = _guarded(lgo, 4 * n, b"\x7E\x81")
            qb = _guarded(lgo, 4 * n * A, b"\x96\x69\x0F")
            before = [t.clone() for t in (work, act, qb)]
            rc = call(lgo, kind, pol, v, f, n, work.data_ptr() + PAD, act.data_ptr() + PAD, qb.data_ptr() + PAD if want_q else None)
            lgo.sync()
            assert rc == 0
            for t, t0, size, what in ((work, before[0], wb, "workspace"), (act, before[1], 4 * n, "actions"), (qb, before[2], 4 * n * A, "q")):
                assert torch.equal(t[:PAD], t0[:PAD]), (kind, n, want_q, what, "before")
                assert torch.equal(t[PAD + size:], t0[PAD + size:]), (kind, n, want_q, what, "after")
            if not want_q:
                assert torch.equal(qb, before[2])
            acts = act[PAD:PAD + 4 * n].view(torch.int32).cpu()
            if want_q:
                fresh[n] = (acts, qb[PAD:PAD + 4 * n * A].view(torch.float32).reshape(n, A).cpu())
                check(kind, qnet, view, featv, n, fresh[n][0], fresh[n][1], "%s edges n %d" % (lg, n))
            else:
                assert torch.equal(acts, fresh[n][0])
    # one workspace, calls of different n after each other: what fresh calls give
    work = torch.empty(act_bytes(lgo, kind, pol, nmax), dtype=torch.uint8, device=lgo.dev)
    for n in sorted(ns, reverse=True) + sorted(ns):
        act = torch.empty(n, dtype=torch.int32, device=lgo.dev)
        q = torch.empty((n, A), device=lgo.dev)
        assert call(lgo, kind, pol, v, f, n, work, act, q) == 0
        lgo.sync()
        assert torch.equal(act.cpu(), fresh[n][0]) and torch.equal(q.cpu(), fresh[n][1]), (kind, n)


@pytest.mark.parametrize("lg", LEGS)
@pytest.mark.parametrize("kind,vs,feat,A,ns", [("f32", (9, 9, 3), 9, 17, (1, 3, 5, 127, 129)), ("f32", (15, 15, 7), 56, 31, (1, 3)),
                                               ("f32", (17, 16, 2), 8, 1, (1, 3)), ("bf16", (9, 9, 3), 17, 17, (1, 3, 5, 127, 129)),
                                               ("cells", (13, 13, 7), 34, 21, (1, 3, 5, 129))])
def test_writes_stay_inside_their_buffers(lg, kind, vs, feat, A, ns):
    """actions, Q and the workspace inside larger allocations filled with a sentinel pattern: after the call every byte before and after
    the region given to the kernel is unchanged (n of 1, TA +- 1, 128 +- 1; with and without Q); two calls on one workspace with
    different n give what fresh calls give"""
    _edges_case(lg, kind, vs, feat, A, ns)


# ---------------------------------------------------------------------------------------------------- 3. end to end on the GPU
@pytest.mark.gpu
def test_empty_group_minimap_end_to_end():
    """a battle world whose second group is empty: the first group's device observations carry the reference's 0/0 minimap (NaN) in
    channel 6.  DeepQNetwork.infer_action on the HIP f32 path equals the PyTorch path agent for agent (0: the first NaN of every row), the
    bf16 path on the bf16 cells does too, and set_action + step complete"""
    import torch
    import magent_amd
    from magent_amd.builtin.torch_model import DeepQNetwork
    from magent_amd.builtin.torch_model.hip_policy import HipDqnPolicy, HipDqnPolicyF32
    env = magent_amd.GridWorld("battle", map_size=40, device_obs=True)
    env.set_seed(9); env.reset()
    hs = env.get_handles()
    env.add_agents(hs[0], "random", n=150)
    torch.manual_seed(2)
    m32 = DeepQNetwork(env, hs[0], "f32", memory_size=16)
    m16 = DeepQNetwork(env, hs[0], "bf16", memory_size=16, infer_dtype="bf16")
    assert isinstance(m32._hip, HipDqnPolicyF32) and isinstance(m16._hip, HipDqnPolicy)
    for step in range(3):
        view, feat = env.get_observation(hs[0]); env.sync()
        assert bool(torch.isnan(view[..., 6]).all()) and bool(torch.isfinite(view[..., :6]).all())
        a32 = m32.infer_action((view, feat), None, policy="greedy")
        with torch.no_grad():
            q_torch = m32.qnet(view, feat)
        assert bool(torch.isnan(q_torch).all())
        assert torch.equal(a32.long(), q_torch.argmax(dim=1)) and bool((a32 == 0).all())
        _, q_hip = m32._hip.infer(view, feat, want_q=True)
        assert bool(torch.isnan(q_hip).all())
        cells, feat16 = env.get_observation_device_bf16(hs[0]); env.sync()
        a16 = m16.infer_action((cells, feat16), None, policy="greedy")
        assert torch.equal(a16, a32)
        env.set_action(hs[0], a32)
        env.step(); env.clear_dead()
    assert env.get_num(hs[0]) == 150
    env.close()
