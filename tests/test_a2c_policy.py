"""The A2C acting kernels (magent_amd/csrc/policy_a2c_f32.hip: the two input layers, dense 512, the CommNet steps with their column sums,
the heads, the softmax and the inverse-CDF draw) and their binding (hip_policy.HipA2cPolicyF32), against a float64 NumPy restatement of
a2c.py's _ActorCritic.forward and a float32 NumPy restatement of the draw.

Two legs: `emu` runs policy_a2c_f32.hip compiled as plain C++ against tests/hipemu (a library of its own, CPU tensors, no GPU needed);
`gpu` (marked) runs the product library on cuda:0.

Planted defects that an emulator test here catches: the column sum taken per chunk instead of per call, `others` divided
by n instead of n - 1 (the supported-region sweep, CommNet spans the call); the softmax without the maximum subtracted (large logits: the
one-hot rows of the draw test overflow to NaN); c_a >= t instead of c_a > t (p = [0.5, 0.5], u = 0.5); an fmaxf ReLU (a NaN in a view)."""
import ctypes
import os

import numpy as np
import pytest

import helpers as H

NAN, INF = float("nan"), float("inf")
HID = 512

# The working bounds of the probabilities (absolute) and of the value (relative to 1 + the case's largest |value|).  Measured on the CPU:
# the worst error of the PyTorch float32 CPU forward of _ActorCritic against the float64 oracle below over CASES x {plain, CommNet} was
# 6.3e-7 on a probability and 5.9e-7 on a value (test_a2c_against_float64_over_the_supported_region prints both per case); the bound is
# that times 4 -- the PyTorch forward is the same arithmetic in another summation order, the factor covers the order differences between
# two correct float32 evaluations.  The kernels' own worst ratio to these bounds is in DESIGN.md 3.18.
TORCH_P_ERR, TORCH_V_ERR, ORDER_FACTOR = 6.3e-7, 5.9e-7, 4.0
P_WORK, V_WORK = ORDER_FACTOR * TORCH_P_ERR, ORDER_FACTOR * TORCH_V_ERR


leg, LEGS = H.policy_legs(lambda: H.policy_emu("a2c"), policy_class="HipA2cPolicyF32")      # the two legs
make_inputs, net_params, _battle = H.make_policy_inputs, H.net_params, H.battle
COMM = [pytest.param(False, id="plain"), pytest.param(True, id="comm")]


def make_net(vs, feat, A, comm, seed, dev="cpu", scale=3.0):
    import torch
    from magent_amd.builtin.torch_model.a2c import _ActorCritic
    torch.manual_seed(seed)
    net = _ActorCritic(vs, (feat,), A, comm)
    with torch.no_grad():
        for p in net.parameters():          # larger weights than the default init: every layer matters in the heads (drqn: make_rnet)
            p.mul_(scale)
    return net.to(dev)


def run(lg, pol, view, featv, u=None):
    import torch
    out = pol.infer(view.to(lg.dev).contiguous(), featv.to(lg.dev).contiguous(), u=None if u is None else torch.as_tensor(u).to(lg.dev),
                    want_policy=True, want_value=True)
    lg.sync()
    return [t.cpu().numpy() for t in out]


# ---------------------------------------------------------------------------------------------------- float64 and the derived bound
def np_a2c(P, view, feature, comm):
    """_ActorCritic.forward in float64 -> (p [n][A], value [n]); relu is np.maximum (a NaN stays a NaN)"""
    p, v, _ = _np_a2c(P, view, feature, comm, False)
    return p, v


def _np_a2c(P, view, feature, comm, bounds):
    """the forward pass, and with bounds=True beside every layer a per-entry bound of a float32 evaluation in any summation order
    (u = 2^-24, Higham's gamma_k = k u / (1 - k u) per dot product of length k - 1 with its bias):
      a layer  y = act(x W^T + b), act 1-Lipschitz:   e_y = gamma_(K+2) (|x| |W|^T + |b|) (1 + 2^-20) + e_x |W|^T (+ 4 u for tanh's own evaluation)
      column sums S over n rows:                      e_S = sum_j e_h_j + gamma_n sum_j |h_j|
      others = (S - h) / (n - 1):                     e_o = (e_S + e_h) / (n - 1) + 3 u (sum_j |h_j|) / (n - 1)
      softmax: logits within e of the true ones move p_a by at most p_a (exp(2 max e) - 1); its float evaluation (the subtraction, exp,
      A adds, the division) by at most p_a (max |l - m| + A + 8) 2 u; the clamps by 2e-10 (in float32 the upper clamp is 1.0)"""
    u = 2.0 ** -24
    gam = lambda k: k * u / (1 - k * u)
    Pa = {k: np.abs(v) for k, v in P.items()}
    n = view.shape[0]

    def layer(x, ex, name, act, extra=0.0):
        w, b = P[name + ".weight"], P.get(name + ".bias")
        pre = x @ w.T + (b if b is not None else 0.0)
        if not bounds:
            return act(pre), None
        with np.errstate(invalid="ignore", over="ignore"):
            mag = np.abs(x) @ Pa[name + ".weight"].T + (Pa[name + ".bias"] if b is not None else 0.0)
            e = gam(w.shape[1] + 2) * mag * (1 + 2.0 ** -20) + ex @ Pa[name + ".weight"].T + extra
        return act(pre), e

    relu = lambda a: np.maximum(a, 0)
    ident = lambda a: a
    with np.errstate(invalid="ignore", over="ignore"):
        flat = np.asarray(view, np.float64).reshape(n, -1)
        feature = np.asarray(feature, np.float64)
        z = np.zeros_like
        xv, ev = layer(flat, z(flat), "dense_view", relu)
        xe, ee = layer(feature, z(feature), "dense_emb", relu)
        x, ex = np.concatenate([xv, xe], axis=1), (np.concatenate([ev, ee], axis=1) if bounds else None)
        h, eh = layer(x, ex, "dense", relu)
        if comm:
            skip, eskip = h, eh
            for s in range(2):
                C, Hm = P["comm.%d.C.weight" % s], P["comm.%d.H.weight" % s]
                others = (h.sum(axis=0, keepdims=True) - h) / (n - 1) if n > 1 else np.zeros_like(h)
                pre = others @ C.T + h @ Hm.T + skip
                if bounds:
                    habs = np.abs(h).sum(axis=0, keepdims=True)
                    if n > 1:
                        eS = eh.sum(axis=0, keepdims=True) + gam(n) * habs
                        eo = (eS + eh) / (n - 1) + 3 * u * habs / (n - 1)
                        omag = habs / (n - 1) + 0 * h
                    else:
                        eo, omag = np.zeros_like(h), np.zeros_like(h)
                    mag = omag @ np.abs(C).T + np.abs(h) @ np.abs(Hm).T + np.abs(skip)
                    eh = gam(2 * HID + 3) * mag * (1 + 2.0 ** -20) + eo @ np.abs(C).T + eh @ np.abs(Hm).T + eskip + 4 * u
                h = np.tanh(pre)
        logits, el = layer(h, eh, "policy", ident)
        value, evalue = layer(h, eh, "value", ident)
        m = logits.max(axis=1, keepdims=True)
        e = np.exp(logits - m)
        p = np.clip(e / e.sum(axis=1, keepdims=True), 1e-10, 1 - 1e-10)
        if not bounds:
            return p, value[:, 0], None
        A = logits.shape[1]
        emax = el.max(axis=1, keepdims=True)
        spread = np.abs(logits - m).max(axis=1, keepdims=True)
        ep = p * (np.expm1(np.minimum(2 * emax, 700.0)) + (spread + A + 8) * 2 * u) + 2e-10
    return p, value[:, 0], (ep, evalue[:, 0])


def np_draw(p, u):
    """the draw in float32, in the order include/magent_policy.h states: c_0 = p_0, c_a = c_(a-1) + p_a, t = u c_(A-1); the smallest a with
    c_a > t, else A - 1"""
    p, u = np.asarray(p, np.float32), np.asarray(u, np.float32)
    n, A = p.shape
    out = np.empty(n, np.int64)
    for i in range(n):
        c = np.empty(A, np.float32)
        c[0] = p[i, 0]
        for a in range(1, A):
            c[a] = np.float32(c[a - 1] + p[i, a])
        t = np.float32(u[i] * c[A - 1])
        with np.errstate(invalid="ignore"):
            hit = np.nonzero(c > t)[0]
        out[i] = hit[0] if len(hit) else A - 1
    return out


WORST = {"p": 0.0, "v": 0.0, "hard": 0.0, "torch_p": 0.0, "torch_v": 0.0}


def check_against_float64(P, view, featv, comm, p, value, tag, rows=None):
    """p and value against float64: non-finite entries exactly where float64 has them (NaN where it has NaN), finite ones within the derived
    bound and within the working bound"""
    p64, v64, (ep, ev) = _np_a2c(P, view.double().numpy(), featv.double().numpy(), comm, True)
    if rows is not None:
        p64, v64, ep, ev = p64[rows], v64[rows], ep[rows], ev[rows]
    vscale = 1.0 + float(np.abs(v64[np.isfinite(v64)]).max()) if np.isfinite(v64).any() else 1.0
    for got, want, bound, what, work in ((p, p64, ep, "p", P_WORK), (value, v64, ev, "v", V_WORK * vscale)):
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), (tag, what, np.argwhere(np.isfinite(got) != np.isfinite(want))[:8])
        assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, what)
        ok = np.isfinite(want)
        if not ok.any():
            continue
        d = np.abs(got[ok].astype(np.float64) - want[ok])
        hard = float((d / bound[ok]).max())
        ratio = float(d.max()) / work
        print("%s: %s worst error %.3g = %.3f of the working bound, %.3g of the derived bound" % (tag, what, float(d.max()), ratio, hard))
        assert hard <= 1.0, (tag, what, hard)
        assert ratio <= 1.0, (tag, what, ratio, float(d.max()))
        WORST[what], WORST["hard"] = max(WORST[what], ratio), max(WORST["hard"], hard)
    return p64, v64


# ---------------------------------------------------------------------------------------------------- 1. the supported region
# (view_space, feat, n_action, n): the edges of policy_a2c_f32_supported -- K = H W C of 1 (the smallest), 1183 (13 x 13 x 7: not a multiple
# of 8, rows 4-byte aligned), 48 and 4096 (multiples of 8; 4096 the largest), view_c past 7, feat 1 / 64, n_action 1 / 2 / 21 / 31;
# n of 1, 2, 31, 33 (a layer wave's 32 agents +- 1), 129 (one past a trunk workgroup's 128), 257 (one past a column-sum block's 256)
CASES = [((1, 1, 1), 1, 1, 1), ((13, 13, 7), 34, 21, 33), ((16, 16, 16), 64, 31, 2), ((4, 6, 2), 5, 2, 257), ((5, 7, 3), 64, 31, 129),
         ((13, 13, 7), 34, 21, 31), ((3, 5, 9), 1, 2, 1)]
GPU_N = {1: 1, 2: 2, 31: 31, 33: 33, 129: 385, 257: 1025}


@pytest.mark.parametrize("lg", LEGS)
@pytest.mark.parametrize("comm", COMM)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-f%d-a%d-n%d" % (c[0] + c[1:4]))
def test_a2c_against_float64_over_the_supported_region(lg, comm, case):
    import torch
    lg = leg(lg)
    vs, feat, A, n = case
    n = GPU_N[n] if lg.name == "gpu" else n
    seed = 10 + CASES.index(case) + (100 if comm else 0)
    net = make_net(vs, feat, A, comm, seed)
    view, featv = make_inputs(vs, feat, n, seed * 7)
    P = net_params(net)
    tag = "%s %s %s" % (lg.name, case, "comm" if comm else "plain")
    # the yardstick of the working bound: the PyTorch float32 CPU forward against the same float64 (printed)
    with torch.no_grad():
        tp, tv = net(view, featv)
    p64, v64 = np_a2c(P, view.double().numpy(), featv.double().numpy(), comm)
    WORST["torch_p"] = max(WORST["torch_p"], float(np.abs(tp.double().numpy() - p64).max()))
    WORST["torch_v"] = max(WORST["torch_v"], float(np.abs(tv.double().numpy() - v64).max()) / (1.0 + float(np.abs(v64).max())))
    print("%s: PyTorch float32 CPU forward so far: worst p error %.3g, worst value error %.3g (relative to 1 + max |value|)" % (tag, WORST["torch_p"], WORST["torch_v"]))
    pol = lg.policy(net.to(lg.dev), vs, feat, A)
    u = np.random.RandomState(seed).rand(n).astype(np.float32)
    actions, p, value = run(lg, pol, view, featv, u)
    assert p.shape == (n, A) and value.shape == (n,) and actions.dtype == np.int32
    check_against_float64(P, view, featv, comm, p, value, tag)
    assert ((actions >= 0) & (actions < A)).all()
    assert np.array_equal(actions, np_draw(p, u)), tag
    print("%s: kernels' worst so far: p %.3f, value %.3f of the working bounds, %.3g of the derived bound" % (tag, WORST["p"], WORST["v"], WORST["hard"]))


def test_a2c_supported_region():
    from magent_amd.builtin.torch_model.hip_policy import _Shape
    lib = leg("emu").lib
    ok = lambda *a: lib.policy_a2c_f32_supported(ctypes.byref(_Shape(*a)))
    assert ok(13, 13, 7, 34, 21) and ok(1, 1, 1, 1, 1) and ok(16, 16, 16, 64, 31) and ok(1, 4096, 1, 64, 31) and ok(13, 13, 9, 34, 21)
    for bad in ((16, 16, 17, 34, 21), (4097, 1, 1, 34, 21), (65536, 65536, 1, 34, 21), (0, 13, 7, 34, 21), (13, 0, 7, 34, 21), (13, 13, 0, 34, 21),
                (13, 13, 7, 0, 21), (13, 13, 7, 65, 21), (13, 13, 7, 34, 0), (13, 13, 7, 34, 32)):
        assert not ok(*bad), bad


# ---------------------------------------------------------------------------------------------------- 2. the draw is exact
def _set_head(net, weight_scale, bias):
    import torch
    with torch.no_grad():
        net.policy.weight.mul_(weight_scale)
        net.policy.bias.copy_(torch.as_tensor(bias, dtype=torch.float32))


@pytest.mark.parametrize("lg", LEGS)
def test_a2c_draw_is_the_float32_inverse_cdf(lg):
    """for the kernel's own p rows and the supplied u, the float32 restatement of the draw gives the same action for every agent"""
    lg = leg(lg)
    below_one = np.nextafter(np.float32(1), np.float32(0))
    vs, feat = (4, 5, 3), 6

    def draw(net, A, n, u, seed, poison=None):
        view, featv = make_inputs(vs, feat, n, seed)
        if poison is not None:
            view[poison, 1, 2, 0] = NAN
        pol = lg.policy(net.to(lg.dev), vs, feat, A)
        actions, p, _ = run(lg, pol, view, featv, np.asarray(u, np.float32))
        assert ((actions >= 0) & (actions < A)).all()
        assert np.array_equal(actions, np_draw(p, u)), (A, actions, np_draw(p, u))
        return actions, p

    # random policies: spread rows (small head weights) and peaked rows (scaled weights); u of 0 and of the largest float32 below 1 among them
    for A, scale, seed in ((21, 1.0, 1), (31, 0.2, 2), (2, 1.0, 3), (7, 3.0, 4)):
        n = 200
        u = np.random.RandomState(seed).rand(n).astype(np.float32)
        u[0], u[1], u[2] = 0.0, below_one, 0.5
        net = make_net(vs, feat, A, False, seed)
        _set_head(net, scale / 3.0, np.zeros(A))
        actions, p = draw(net, A, n, u, seed)
        assert actions[0] == 0                                  # (u = 0: t = 0 < c_0)
    # a one-hot row after clamping: the logit of action 2 is 80 above the rest; in float32 the upper clamp 1 - 1e-10 is 1.0.  (A softmax
    # without the maximum subtracted overflows here: exp(80 + ..) is finite, but the second row's 200 is not.)
    for top in (80.0, 200.0):
        net = make_net(vs, feat, 5, False, 5)
        _set_head(net, 0.0, [0, 0, top, 0, 0])
        u = np.asarray([0.0, 0.5, below_one, 1e-9, 0.999], np.float32)
        actions, p = draw(net, 5, 5, u, 5)
        assert (p[:, 2] == 1.0).all() and (p[:, [0, 1, 3, 4]] == np.float32(1e-10)).all()
        assert actions[1] == 2 and actions[0] == 0              # (u = 0 takes action 0: c_0 = 1e-10 > 0)
    # p = [0.5, 0.5] exactly; with u = 0.5, t equals c_0, so `>` gives action 1 (`>=` would give 0)
    net = make_net(vs, feat, 2, False, 6)
    _set_head(net, 0.0, [0.25, 0.25])
    u = np.asarray([0.5, 0.0, below_one, 0.25, 0.75, np.nextafter(np.float32(0.5), np.float32(0))], np.float32)
    actions, p = draw(net, 2, 6, u, 6)
    assert (p == 0.5).all()
    assert actions.tolist() == [1, 0, 1, 0, 1, 0]
    # one action
    net = make_net(vs, feat, 1, False, 7)
    actions, p = draw(net, 1, 4, np.asarray([0.0, 0.5, below_one, 0.1], np.float32), 7)
    assert (actions == 0).all() and (p == 1.0).all()
    # a row with a NaN: no c_a > t holds, the action is A - 1; the other rows are untouched
    net = make_net(vs, feat, 9, False, 8)
    actions, p = draw(net, 9, 40, np.random.RandomState(8).rand(40).astype(np.float32), 8, poison=33)
    assert np.isnan(p[33]).all() and actions[33] == 8 and np.isfinite(np.delete(p, 33, axis=0)).all()


# ---------------------------------------------------------------------------------------------------- 3. the draw follows the distribution
@pytest.mark.parametrize("lg", LEGS)
def test_a2c_draw_follows_the_distribution(lg):
    """one observation repeated R times, u = None (torch.rand after torch.manual_seed): every action's count within the binomial's
    6 sigma + 1 of R p_a"""
    import torch
    lg = leg(lg)
    vs, feat, A = (3, 3, 2), 4, 7
    R = 20000 if lg.name == "emu" else 200000
    for comm in ((False,) if lg.name == "emu" else (False, True)):       # (with CommNet every agent's `others` is the common row itself)
        net = make_net(vs, feat, A, comm, 40, scale=2.0)
        view, featv = make_inputs(vs, feat, 1, 41)
        pol = lg.policy(net.to(lg.dev), vs, feat, A)
        views, feats = view.expand((R,) + vs).contiguous().to(lg.dev), featv.expand(R, feat).contiguous().to(lg.dev)
        torch.manual_seed(1234)
        actions, p = pol.infer(views, feats, want_policy=True)
        lg.sync()
        actions, p = actions.cpu().numpy(), p.cpu().numpy().astype(np.float64)
        assert (p == p[0]).all()
        if lg.name == "gpu":                                     # the same torch seed, the same actions
            torch.manual_seed(1234)
            again = pol.infer(views, feats)
            lg.sync()
            assert np.array_equal(again.cpu().numpy(), actions)
        count = np.bincount(actions, minlength=A)
        assert count.sum() == R and len(count) == A
        pa = p[0] / p[0].sum()
        for a in range(A):
            assert abs(count[a] - R * pa[a]) <= 6 * np.sqrt(R * pa[a] * (1 - pa[a])) + 1, (comm, a, count, R * pa)


# ---------------------------------------------------------------------------------------------------- 4. CommNet spans the call
@pytest.mark.parametrize("lg", LEGS)
def test_a2c_commnet_spans_the_call_and_is_deterministic(lg):
    lg = leg(lg)
    vs, feat, A = (5, 5, 3), 7, 9
    n = 300 if lg.name == "emu" else 1500                      # (past one column-sum block)
    net = make_net(vs, feat, A, True, 50)
    P = net_params(net)
    view, featv = make_inputs(vs, feat, n, 51)
    u = np.random.RandomState(52).rand(n).astype(np.float32)
    net = net.to(lg.dev)
    # the same inputs through chunk = 4, chunk = 131072 and a second run: the same bits
    outs = [run(lg, lg.policy(net, vs, feat, A, chunk=c), view, featv, u) for c in (4, 131072, 131072)]
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b, equal_nan=True)
    actions, p, value = outs[0]
    check_against_float64(P, view, featv, True, p, value, "%s comm n=%d" % (lg.name, n))      # (the means over the call, not over a chunk)
    # permuted agents: permuted outputs, within the working bound (the block sums change, so bits may)
    perm = np.random.RandomState(53).permutation(n)
    _, p2, value2 = run(lg, lg.policy(net, vs, feat, A), view[perm], featv[perm], u[perm])
    assert np.abs(p2 - p[perm]).max() <= P_WORK
    assert np.abs(value2 - value[perm]).max() <= V_WORK * (1.0 + np.abs(value).max())
    # n == 1: others = 0
    _, p1, v1 = run(lg, lg.policy(net, vs, feat, A), view[:1], featv[:1], u[:1])
    check_against_float64(P, view[:1], featv[:1], True, p1, v1, "%s comm n=1" % lg.name)
    # a NaN in one agent's view: every row with CommNet (through the sum), that row alone without
    view[7, 2, 2, 1] = NAN
    _, pn, vn = run(lg, lg.policy(net, vs, feat, A), view, featv, u)
    assert np.isnan(pn).all() and np.isnan(vn).all()
    check_against_float64(P, view, featv, True, pn, vn, "%s comm poisoned" % lg.name)
    plain = make_net(vs, feat, A, False, 54)
    actions, pn, vn = run(lg, lg.policy(plain.to(lg.dev), vs, feat, A, chunk=64), view, featv, u)
    assert np.isnan(pn[7]).all() and np.isnan(vn[7]) and np.isfinite(np.delete(pn, 7, axis=0)).all() and np.isfinite(np.delete(vn, 7)).all()
    check_against_float64(net_params(plain), view, featv, False, pn, vn, "%s plain poisoned, chunk 64" % lg.name)
    assert actions[7] == A - 1
    # an infinity: inf - inf in `others`, as torch has it
    view[7, 2, 2, 1] = INF
    _, pi, vi = run(lg, lg.policy(net, vs, feat, A), view, featv, u)
    check_against_float64(P, view, featv, True, pi, vi, "%s comm inf" % lg.name)


# ---------------------------------------------------------------------------------------------------- 5. buffers
@pytest.mark.parametrize("lg", LEGS)
@pytest.mark.parametrize("comm", COMM)
def test_a2c_writes_nothing_outside_its_buffers(lg, comm):
    """actions, policy, value and the workspace inside sentinel-filled allocations; inputs and u untouched; refused calls write nothing"""
    import torch
    lg = leg(lg)
    vs, feat, A = (6, 5, 4), 6, 11
    n = 261                                  # (past a trunk workgroup and a column-sum block; not a multiple of 32)
    net = make_net(vs, feat, A, comm, 60).to(lg.dev)
    pol = lg.policy(net, vs, feat, A)
    pol.pack()
    view, featv = make_inputs(vs, feat, n, 61)
    view, featv = view.to(lg.dev), featv.to(lg.dev)
    u = torch.rand(n, generator=torch.Generator().manual_seed(62)).to(lg.dev)
    keep = [t.clone() for t in (view, featv, u)]
    PAD = 333
    nb = ctypes.c_size_t(0)
    assert lg.lib.policy_a2c_f32_workspace_bytes(ctypes.byref(pol.shape), n, int(comm), ctypes.byref(nb)) == 0

    def buffers():
        return (torch.full((n + 2 * PAD,), -7, dtype=torch.int32, device=lg.dev), torch.full((n * A + 2 * PAD,), -77.0, device=lg.dev),
                torch.full((n + 2 * PAD,), -777.0, device=lg.dev), torch.full((nb.value + 2 * 4096,), 0x5A, dtype=torch.uint8, device=lg.dev))

    def call(shape, acts, pb, vb, work, u_ptr, acts_ptr, work_off=4096):
        rc = lg.lib.policy_a2c_infer_f32(ctypes.byref(shape), ctypes.byref(pol._w), view.data_ptr(), featv.data_ptr(), n, u_ptr,
                                         work[work_off:].data_ptr(), acts_ptr, pb[PAD:].data_ptr(), vb[PAD:].data_ptr(), None)
        lg.sync()
        return rc
    acts, pb, vb, work = buffers()
    assert work[4096:].data_ptr() % 16 == 0
    assert call(pol.shape, acts, pb, vb, work, u.data_ptr(), acts[PAD:].data_ptr()) == 0
    for buf, fill, m in ((acts, -7, n), (pb, -77.0, n * A), (vb, -777.0, n)):
        assert bool((buf[:PAD] == fill).all()) and bool((buf[PAD + m:] == fill).all())
        assert not bool((buf[PAD:PAD + m] == fill).any())
    assert bool((work[:4096] == 0x5A).all()) and bool((work[4096 + nb.value:] == 0x5A).all())
    for a, b in zip(keep, (view, featv, u)):
        assert torch.equal(a, b)
    # the same step through the wrapper: the same bits
    a2, p2, v2 = pol.infer(view, featv, u=u, want_policy=True, want_value=True)
    lg.sync()
    assert torch.equal(a2, acts[PAD:PAD + n]) and torch.equal(p2.reshape(-1), pb[PAD:PAD + n * A]) and torch.equal(v2, vb[PAD:PAD + n])
    # refused before anything is written: an unsupported shape, a NULL u, NULL actions, a misaligned workspace
    bad = type(pol.shape)(vs[0], vs[1], vs[2], feat, 32)
    assert lg.lib.policy_a2c_f32_supported(ctypes.byref(bad)) == 0
    for shape, u_ptr, null_actions, off in ((bad, u.data_ptr(), False, 4096), (pol.shape, None, False, 4096), (pol.shape, u.data_ptr(), True, 4096),
                                            (pol.shape, u.data_ptr(), False, 4100)):
        acts, pb, vb, work = buffers()
        assert call(shape, acts, pb, vb, work, u_ptr, None if null_actions else acts[PAD:].data_ptr(), off) != 0
        for buf, fill in ((acts, -7), (pb, -77.0), (vb, -777.0), (work, 0x5A)):
            assert bool((buf == fill).all())
    for a, b in zip(keep, (view, featv, u)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- 6. the model on the GPU
class _Env(object):
    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        self.old = os.environ.get(self.key)
        os.environ[self.key] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ[self.key]
        else:
            os.environ[self.key] = self.old


@pytest.mark.gpu
@pytest.mark.parametrize("comm", COMM)
def test_a2c_model_acts_through_the_kernels_in_a_battle(comm):
    """24 steps of a battle on the HIP engine with device observations, both sides acting through AdvantageActorCritic; each step the
    binding's probabilities and values of side 0 agree with the model's own network; then a train() step, after which they still do"""
    import torch
    from magent_amd.builtin.torch_model import AdvantageActorCritic
    from magent_amd.utility import EpisodesBuffer
    env, hs = _battle(11)
    torch.manual_seed(5)
    models = [AdvantageActorCritic(env, h, "a2c%d" % k, use_comm=comm) for k, h in enumerate(hs)]
    A = env.get_action_space(hs[0])[0]
    assert all(m._hip is not None for m in models)
    buf = EpisodesBuffer(capacity=20)

    def agree(view, feat, tag):
        _, p, v = models[0]._hip.infer(view, feat, want_policy=True, want_value=True)
        with torch.no_grad():
            tp, tv = models[0].net(view, feat)
        assert float((p - tp).abs().max()) <= P_WORK, (tag, float((p - tp).abs().max()))
        assert float((v - tv).abs().max()) <= V_WORK * (1.0 + float(tv.abs().max())), (tag, float((v - tv).abs().max()))

    for step in range(24):
        acts = []
        for k, h in enumerate(hs):
            view, feat = env.get_observation(h)
            ids = env.get_agent_id(h)
            assert models[k]._on_kernels(view, feat)
            if k == 0:
                agree(view, feat, step)
            a = models[k].infer_action((view, feat), ids)
            assert isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.int32 and a.shape == (len(ids),)
            assert int(a.min()) >= 0 and int(a.max()) < A
            env.set_action(h, a)
            acts.append((ids, (view, feat), a))
        env.step()
        ids, obs, a = acts[0]
        buf.record_step(ids, obs, a.cpu().numpy(), env.get_reward(hs[0]), env.get_alive(hs[0]))
        env.clear_dead()
    before = [p.detach().clone() for p in models[0].net.parameters()]
    models[0].train(buf)
    assert any(not torch.equal(a, b) for a, b in zip(before, models[0].net.parameters()))
    assert models[0]._hip.dirty
    view, feat = env.get_observation(hs[0])
    agree(view, feat, "after train")
    env.close()


@pytest.mark.gpu
def test_a2c_falls_back_to_torch_past_each_limit_and_on_request():
    from magent_amd.builtin.torch_model import AdvantageActorCritic
    env, hs = _battle(3, n=20, size=20)
    vs, fs = env.get_view_space(hs[0]), env.get_feature_space(hs[0])
    assert AdvantageActorCritic(env, hs[0], "ok")._hip is not None
    assert AdvantageActorCritic(env, hs[0], "ok", custom_view_space=(16, 16, 16), custom_feature_space=(64,))._hip is not None
    for cv, cf in (((16, 16, 17), fs), (vs, (65,))):
        assert AdvantageActorCritic(env, hs[0], "past", custom_view_space=cv, custom_feature_space=cf)._hip is None, (cv, cf)
    with _Env("MAGENT_POLICY_F32", "torch"):
        assert AdvantageActorCritic(env, hs[0], "t")._hip is None
    # numpy observations run the PyTorch path of a kernel model and return numpy
    m = AdvantageActorCritic(env, hs[0], "np", use_comm=True)
    view, feat = env.get_observation(hs[0])
    ids = env.get_agent_id(hs[0])
    out = m.infer_action((view.cpu().numpy(), feat.cpu().numpy()), ids)
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and out.shape == (len(ids),)
    assert not m._on_kernels(view.double(), feat) and not m._on_kernels(view.cpu(), feat.cpu()) and not m._on_kernels(view[:, :5], feat)
    env.close()
