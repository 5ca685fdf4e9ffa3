"""The DRQN acting kernels (magent_amd/csrc/policy_drqn_f32.hip: the DQN's float32 trunk, a GRU(512) cell, the head) and their state table
keyed by agent id (hip_policy.HipDrqnPolicyF32), against a float64 NumPy restatement of one step of drqn.py's _RecurrentQNet.

Two legs: `emu` runs policy_f32.hip + policy_drqn_f32.hip compiled as plain C++ against tests/hipemu (a library of their own, CPU
tensors, no GPU needed); `gpu` (marked) runs the product library on cuda:0.  Every call is checked against float64 fed the kernels' OWN
previous states (looked up with the dict path's semantics), so that errors do not compound in the check.

Planted defects that an emulator test here catches: r and z swapped, b_hn added outside the r product (the supported-region
sweep); the first duplicate stored instead of the last, a stale table after n == 0 (the state table over calls); an fmaxf ReLU (non-finite
inputs and weights)."""
import ctypes
import os

import numpy as np
import pytest

import helpers as H

NAN, INF = float("nan"), float("inf")
S = 512


# the two legs; on the emulator three conv workgroups walk every tile
leg, LEGS = H.policy_legs(lambda: H.policy_emu("drqn"), tune="policy_grid=3", policy_class="HipDrqnPolicyF32")
make_inputs, net_params, make_rnet, DictModel, _battle = H.make_policy_inputs, H.net_params, H.make_rnet, H.DictModel, H.battle


# ---------------------------------------------------------------------------------------------------- float64
def np_drqn_step(P, view, feature, h, dueling, magnitude=False):
    """one step of _RecurrentQNet.forward (batch n, unroll 1) in float64 -> (Q [n][A], h' [n][512]).  relu is np.maximum (a NaN stays NaN).
    magnitude=True: the trunk and the gates' pre-activations on |weights|, |biases|, |inputs|, |h| -> (Xmag, Gmag [4][n][512]) for the bound"""
    mag = np.abs if magnitude else (lambda a: a)
    relu = (lambda a: a) if magnitude else (lambda a: np.maximum(a, 0))
    P = {k: mag(v) for k, v in P.items()}
    x = mag(np.asarray(view, np.float64))

    def conv(x, w, b):                                        # x [n,H,W,C], w [O][C][3][3]
        n, hh, ww, _ = x.shape
        out = np.zeros((n, hh - 2, ww - 2, w.shape[0]))
        for dy in range(3):
            for dx in range(3):
                out += np.tensordot(x[:, dy:dy + hh - 2, dx:dx + ww - 2, :], w[:, :, dy, dx], axes=([3], [1]))
        return relu(out + b)
    x = conv(conv(x, P["conv1.weight"], P["conv1.bias"]), P["conv2.weight"], P["conv2.bias"])
    flat = x.reshape(x.shape[0], -1)
    xh = np.concatenate([relu(flat @ P["dense_view.weight"].T + P["dense_view.bias"]),
                         relu(mag(np.asarray(feature, np.float64)) @ P["dense_emb.weight"].T + P["dense_emb.bias"])], axis=1)
    hp = mag(np.asarray(h, np.float64))
    gi = xh @ P["rnn.weight_ih_l0"].T + P["rnn.bias_ih_l0"]
    gh = hp @ P["rnn.weight_hh_l0"].T + P["rnn.bias_hh_l0"]
    if magnitude:
        return xh, np.stack([gi[:, :S] + gh[:, :S], gi[:, S:2 * S] + gh[:, S:2 * S], gi[:, 2 * S:], gh[:, 2 * S:]])
    with np.errstate(over="ignore", invalid="ignore"):
        r = 1.0 / (1.0 + np.exp(-(gi[:, :S] + gh[:, :S])))
        z = 1.0 / (1.0 + np.exp(-(gi[:, S:2 * S] + gh[:, S:2 * S])))
        nn_ = np.tanh(gi[:, 2 * S:] + r * gh[:, 2 * S:])
        h2 = (1.0 - z) * nn_ + z * hp
    return np_head(P, h2, dueling), h2


def np_head(P, h2, dueling, magnitude=False):
    if magnitude:
        P = {k: np.abs(v) for k, v in P.items()}
        h2 = np.abs(h2)
    value = h2 @ P["value.weight"].T + P["value.bias"]
    if not dueling:
        return value
    adv = h2 @ P["advantage.weight"].T
    return value + adv + adv.mean(axis=1, keepdims=True) if magnitude else value + adv - adv.mean(axis=1, keepdims=True)


def error_bounds(P, view, feature, h, h64, vs, feat, A, dueling):
    """per-entry bounds (on h', on Q) of a float32 evaluation in any summation order (u = 2^-24; Higham's gamma_(K+1) per dot product):
      trunk x      : c_t u Xmag, c_t = the trunk's reduction lengths (helpers.f32_error_bound without the head)
      pre-activation of each gate g: (c_t + 1030) u Gmag (Gmag: the gate's |W_i| Xmag + |b_i| + |W_h| |h| + |b_h|)
      r, z         : e_g / 4 + 4 u (sigmoid is 1/4-Lipschitz; its float evaluation)
      n            : e_nx + e_nh + |W_hn h + b_hn|mag e_r + 4 u (|n| + |r nh|)mag u-terms folded in + 4 u
      h'           : e_n + |n - h| e_z + 4 u   (|n|, |h|, |z| <= 1)
      Q            : (512 + A + 4) u Qmag + |W_head| e_h' (+ the mean of |W_adv| e_h' for the dueling head)"""
    u = 2.0 ** -24
    hh, ww, _ = vs
    c_t = 73 + 289 + ((hh - 4) * (ww - 4) * 32 + 1) + ((feat + 7) // 8 * 8 + 1)
    _, G = np_drqn_step(P, view, feature, h, dueling, magnitude=True)
    e = (c_t + 1030) * u * G
    er, ez = e[0] / 4 + 4 * u, e[1] / 4 + 4 * u
    en = e[2] + e[3] + G[3] * er + 4 * u * (1 + G[3]) + 4 * u
    with np.errstate(invalid="ignore"):
        n64 = np.abs(h64) + np.abs(np.asarray(h, np.float64))
    eh = en + np.minimum(n64 + 2, 2) * ez + 4 * u
    Pa = {k: np.abs(v) for k, v in P.items()}
    eq = (512 + A + 4) * u * np_head(P, h64, dueling, magnitude=True) + eh @ Pa["value.weight"].T
    if dueling:
        ea = eh @ Pa["advantage.weight"].T
        eq = eq + ea + ea.mean(axis=1, keepdims=True)
    return eh, eq


# ---------------------------------------------------------------------------------------------------- one checked call
WORST = {}


def step_and_check(lg, pol, net, dm, view, featv, ids, vs, feat, A, dueling, tag, expect_nonfinite=None):
    """one kernel call of the policy; Q, actions and h' against float64 fed the looked-up kernel states; the table against the dict model"""
    import torch
    n = len(ids)
    h_prev = dm.lookup(ids)
    ids_t = torch.as_tensor(np.asarray(ids, np.int32)).to(lg.dev)
    actions, q = pol.infer(view.to(lg.dev).contiguous(), featv.to(lg.dev).contiguous(), ids_t, want_q=True)
    lg.sync()
    actions, q, h2 = actions.cpu(), q.cpu().double().numpy(), pol._states.cpu().double().numpy()
    P = net_params(net)
    q64, h64 = np_drqn_step(P, view.double().numpy(), featv.double().numpy(), h_prev, dueling)
    # actions: in range, torch.argmax of the kernel's own Q row
    a = actions.long()
    assert bool(((a >= 0) & (a < A)).all()), tag
    assert torch.equal(a, torch.from_numpy(q).argmax(dim=1)), tag
    # non-finite exactly where float64 is, NaN where it is NaN
    for got, want, what in ((q, q64, "Q"), (h2, h64, "h'")):
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), (tag, what, np.argwhere(np.isfinite(got) != np.isfinite(want))[:8])
        assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, what)
    if expect_nonfinite is not None:
        bad = ~np.isfinite(q).all(axis=1)
        assert np.array_equal(np.nonzero(bad)[0], np.asarray(sorted(expect_nonfinite), dtype=np.int64)), (tag, np.nonzero(bad)[0])
    eh, eq = error_bounds(P, view.double().numpy(), featv.double().numpy(), h_prev, h64, vs, feat, A, dueling)
    for got, want, bound, what, tight_scale in ((h2, h64, eh, "h'", 1.0), (q, q64, eq, "Q", None)):
        ok = np.isfinite(want)
        if not ok.any():
            continue
        d = np.abs(got[ok] - want[ok])
        ratio = float((d / bound[ok]).max())
        assert ratio <= 1.0, (tag, what, ratio)
        scale = tight_scale if tight_scale is not None else float(np.abs(want[ok]).max())
        tight = float((d / (1e-5 * scale + 1e-7)).max())
        assert tight <= 1.0, (tag, what, tight, float(d.max()))
        WORST[what] = max(WORST.get(what, (0.0, 0.0)), (ratio, tight))
    # the table: the dict path's keys in its order, each id's row its last occurrence's
    dm.store(ids, h2.astype(np.float32))
    got = pol.states_dict()
    assert list(got.keys()) == list(dm.states.keys()), tag
    for k, v in got.items():
        assert np.array_equal(v.cpu().numpy(), dm.states[k], equal_nan=True), (tag, k)
    print("%s: worst h' %s, Q %s" % (tag, WORST.get("h'"), WORST.get("Q")))
    return actions, q, h2


# ---------------------------------------------------------------------------------------------------- 1. the supported region
# (view_space, feat, n_action, n): the edges of policy_dqn_f32_supported (TA = 4 / 2, H2 W2 odd / even, feat 1 / 56, n_action 1 / 16 / 17 / 31);
# n of 1, 31, 33 (a GRU wave's 32 agents +- 1), 129 (a head group of 128 + 1) on the GPU
CASES = [((5, 5, 1), 1, 1, 1), ((13, 13, 7), 34, 21, 33), ((9, 9, 2), 56, 31, 5), ((14, 14, 6), 17, 16, 3), ((12, 13, 5), 9, 17, 31),
         ((19, 19, 7), 34, 21, 2)]
GPU_N = {1: 1, 33: 300, 5: 129, 3: 257, 31: 31, 2: 40}


@pytest.mark.parametrize("lg", LEGS)
@pytest.mark.parametrize("dueling", [True, False], ids=["dueling", "plain"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-f%d-a%d-n%d" % (c[0] + c[1:4]))
def test_drqn_against_float64_over_the_supported_region(lg, dueling, case):
    """three calls: an empty table (the kernel's variant without the h half), then ids kept, dropped and added"""
    import torch
    lg = leg(lg)
    vs, feat, A, n = case
    n = GPU_N[n] if lg.name == "gpu" else n
    seed = 10 + CASES.index(case) + (100 if dueling else 0)
    net = make_rnet(vs, feat, A, dueling, seed, lg.dev)
    pol = lg.policy(net, vs, feat, A)
    dm = DictModel()
    rs = np.random.RandomState(seed)
    ids = np.arange(n, dtype=np.int32) * 3
    for call in range(3):
        view, featv = make_inputs(vs, feat, len(ids), seed * 7 + call)
        step_and_check(lg, pol, net, dm, view, featv, ids, vs, feat, A, dueling, "%s %s call %d" % (lg.name, case, call))
        keep = ids[rs.rand(len(ids)) < 0.7]
        ids = np.concatenate([keep, np.arange(2) + 1000 * (call + 1)]).astype(np.int32)
    assert torch.is_tensor(pol._states)


# ---------------------------------------------------------------------------------------------------- 2. ids over several calls
ID_CALLS = [
    [0, 1, 2, 3, 4, 5, 6, 7, 8, 9],                     # a first call
    [9, 2, 5, 11, 3, 0, 40],                            # kept (shuffled, non-ascending), dropped (1, 4, 6, 7, 8), new (11, 40)
    [5, 5, 9, 2, 9, 9, 7, 40, 13],                      # duplicates: every row reads the looked-up state; the LAST occurrence is stored
    [9, 5, 2, 7],                                       # then the duplicated ids are read back; 7 was absent last call (dropped, zeros)
    [],                                                 # n == 0: the table is emptied
    [0, 1, 2, 9, 5],                                    # old ids reused after n == 0: they start from zeros
    [3, 2, 1, 0, 8],                                    # ids restarting at 0 as after env.reset (a subset, descending)
]


@pytest.mark.parametrize("lg", LEGS)
def test_drqn_state_table_over_calls(lg):
    import torch
    lg = leg(lg)
    vs, feat, A = (9, 9, 3), 12, 9
    net = make_rnet(vs, feat, A, True, 7, lg.dev)
    pol = lg.policy(net, vs, feat, A)
    dm = DictModel()
    for k, ids in enumerate(ID_CALLS):
        ids = np.asarray(ids, np.int32)
        if len(ids) == 0:            # (drqn.py's n == 0: agent_states = {} -> the device table is emptied)
            pol.load_states({})
            dm.store(ids, np.zeros((0, S), np.float32))
            assert pol.states_dict() == {}
            continue
        view, featv = make_inputs(vs, feat, len(ids), 50 + k)
        prev = dm.lookup(ids)
        _, _, h2 = step_and_check(lg, pol, net, dm, view, featv, ids, vs, feat, A, True, "%s ids call %d" % (lg.name, k))
        if k == 5:
            assert not prev.any()        # every id starts from zeros after the table was emptied
    # a chunked call (the wrapper splits n into chunks that all read the same previous table)
    pol.chunk = 4
    ids = np.asarray([8, 3, 3, 77, 0, 2, 1, 8, 5, 3], np.int32)
    view, featv = make_inputs(vs, feat, len(ids), 99)
    step_and_check(lg, pol, net, dm, view, featv, ids, vs, feat, A, True, "%s chunked" % lg.name)
    assert torch.equal(pol._sorted.cpu(), torch.sort(torch.as_tensor(ids)).values)


# ---------------------------------------------------------------------------------------------------- 3. non-finite inputs and weights
@pytest.mark.parametrize("lg", LEGS)
def test_drqn_non_finite_inputs_and_weights(lg):
    import torch
    lg = leg(lg)
    vs, feat, A = (7, 7, 4), 10, 7
    n = 40 if lg.name == "emu" else 300
    net = make_rnet(vs, feat, A, True, 21, lg.dev)
    pol = lg.policy(net, vs, feat, A)
    dm = DictModel()
    ids = np.arange(n, dtype=np.int32) + 100
    view, featv = make_inputs(vs, feat, n, 3)
    view[0, 3, 3, 1] = NAN            # first agent of a GRU wave
    featv[31, 4] = INF                # last agent of the first wave
    view[33, 0, 0, 0] = -INF
    step_and_check(lg, pol, net, dm, view, featv, ids, vs, feat, A, True, "%s poisoned inputs" % lg.name, expect_nonfinite={0, 31, 33})
    # the poisoned ids carry their NaN states into the next call on clean inputs; a new id beside them does not
    ids2 = np.concatenate([ids[30:35][::-1], [7]]).astype(np.int32)
    view, featv = make_inputs(vs, feat, len(ids2), 4)
    step_and_check(lg, pol, net, dm, view, featv, ids2, vs, feat, A, True, "%s carried NaN" % lg.name,
                   expect_nonfinite={int(np.nonzero(ids2 == 131)[0][0]), int(np.nonzero(ids2 == 133)[0][0])})
    # a NaN in weight_hh_l0 (gate z, unit 77): torch's W_h @ h is NaN there for every agent -- also with an empty table (W_h @ 0)
    with torch.no_grad():
        net.rnn.weight_hh_l0[S + 77, 5] = NAN
    pol.dirty = True
    pol.load_states({})
    dm = DictModel()
    view, featv = make_inputs(vs, feat, 5, 5)
    step_and_check(lg, pol, net, dm, view, featv, ids[:5], vs, feat, A, True, "%s NaN weight, empty table" % lg.name, expect_nonfinite=set(range(5)))
    step_and_check(lg, pol, net, dm, view, featv, ids[:5], vs, feat, A, True, "%s NaN weight, carried" % lg.name, expect_nonfinite=set(range(5)))


# ---------------------------------------------------------------------------------------------------- 4. buffers
@pytest.mark.parametrize("lg", LEGS)
def test_drqn_writes_nothing_outside_its_buffers(lg):
    """actions, Q and the new states inside sentinel-filled allocations; the previous table and the inputs stay untouched"""
    import torch
    lg = leg(lg)
    vs, feat, A = (8, 7, 5), 6, 11
    n = 37
    net = make_rnet(vs, feat, A, True, 31, lg.dev)
    pol = lg.policy(net, vs, feat, A)
    view, featv = make_inputs(vs, feat, n, 8)
    view, featv = view.to(lg.dev), featv.to(lg.dev)
    ids = torch.arange(n, dtype=torch.int32, device=lg.dev) * 2
    pol.infer(view, featv, ids)            # a table of n rows
    lg.sync()
    pol.pack()
    table = [t.clone() for t in (pol._sorted, pol._rows, pol._states)]
    PAD = 333
    acts = torch.full((n + 2 * PAD,), -7, dtype=torch.int32, device=lg.dev)
    q = torch.full((n * A + 2 * PAD,), -77.0, device=lg.dev)
    SP = 332                               # (state rows are float4-aligned: the entry refuses a misaligned table)
    st = torch.full((n * S + 2 * SP,), -777.0, device=lg.dev)
    nb = ctypes.c_size_t(0)
    lg.lib.policy_drqn_f32_workspace_bytes(ctypes.byref(pol.shape), n, ctypes.byref(nb))
    work = torch.full((nb.value + 2 * 4096,), 0x5A, dtype=torch.uint8, device=lg.dev)
    ids2 = torch.flip(ids, [0]).contiguous()
    rc = lg.lib.policy_drqn_infer_f32(ctypes.byref(pol.shape), ctypes.byref(pol._w), view.data_ptr(), featv.data_ptr(), n, ids2.data_ptr(),
                                      pol._sorted.data_ptr(), pol._rows.data_ptr(), pol._states.data_ptr(), n, st[SP:].data_ptr(),
                                      work[4096:].data_ptr(), acts[PAD:].data_ptr(), q[PAD:].data_ptr(), None)
    lg.sync()
    assert rc == 0
    for buf, fill, m, pad in ((acts, -7, n, PAD), (q, -77.0, n * A, PAD), (st, -777.0, n * S, SP)):
        assert bool((buf[:pad] == fill).all()) and bool((buf[pad + m:] == fill).all())
        assert not bool((buf[pad:pad + m] == fill).any())
    assert bool((work[:4096] == 0x5A).all()) and bool((work[4096 + nb.value:] == 0x5A).all())
    for a, b in zip(table, (pol._sorted, pol._rows, pol._states)):
        assert torch.equal(a, b)
    # the same step through the wrapper: the same bits
    a2, q2 = pol.infer(view, featv, ids2, want_q=True)
    lg.sync()
    assert torch.equal(a2, acts[PAD:PAD + n]) and torch.equal(q2.reshape(-1), q[PAD:PAD + n * A]) and torch.equal(pol._states.reshape(-1), st[SP:SP + n * S])
    assert lg.lib.policy_drqn_infer_f32(ctypes.byref(pol.shape), ctypes.byref(pol._w), view.data_ptr(), featv.data_ptr(), n, ids2.data_ptr(),
                                        None, None, None, 0, st[PAD:].data_ptr(), work.data_ptr(), acts[PAD:].data_ptr(), None, None) == 1
    # an unsupported shape or a missing table pointer is refused before anything is written
    bad = type(pol.shape)(vs[0], vs[1], 8, feat, A)
    assert lg.lib.policy_drqn_f32_supported(ctypes.byref(bad)) == 0
    assert lg.lib.policy_drqn_infer_f32(ctypes.byref(bad), ctypes.byref(pol._w), view.data_ptr(), featv.data_ptr(), n, ids2.data_ptr(), None,
                                        None, None, 0, st[PAD:].data_ptr(), work.data_ptr(), acts[PAD:].data_ptr(), None, None) == 1
    assert lg.lib.policy_drqn_infer_f32(ctypes.byref(pol.shape), ctypes.byref(pol._w), view.data_ptr(), featv.data_ptr(), n, ids2.data_ptr(),
                                        None, None, None, 3, st[PAD:].data_ptr(), work.data_ptr(), acts[PAD:].data_ptr(), None, None) == 1


def test_drqn_supported_is_the_dqn_region():
    from magent_amd.builtin.torch_model.hip_policy import _Shape
    lg = leg("emu")
    for h in range(3, 60, 2):
        for w in range(3, 60, 3):
            for c, feat, A in ((7, 34, 21), (1, 56, 31), (8, 34, 21), (7, 57, 21), (7, 34, 32), (7, 34, 0)):
                s = _Shape(h, w, c, feat, A)
                assert lg.lib.policy_drqn_f32_supported(ctypes.byref(s)) == lg.lib.policy_dqn_f32_supported(ctypes.byref(s))


# ---------------------------------------------------------------------------------------------------- 5. the model on the GPU
def _models(env, h, use_dueling=True):
    """the same network twice: the kernel path and, with MAGENT_POLICY_F32=torch, the PyTorch path"""
    import torch
    from magent_amd.builtin.torch_model import DeepRecurrentQNetwork
    torch.manual_seed(5)
    dev = DeepRecurrentQNetwork(env, h, "dev", memory_size=16, use_dueling=use_dueling)
    old = os.environ.get("MAGENT_POLICY_F32")
    os.environ["MAGENT_POLICY_F32"] = "torch"
    try:
        ref = DeepRecurrentQNetwork(env, h, "ref", memory_size=16, use_dueling=use_dueling)
    finally:
        if old is None:
            del os.environ["MAGENT_POLICY_F32"]
        else:
            os.environ["MAGENT_POLICY_F32"] = old
    ref.qnet.load_state_dict(dev.qnet.state_dict())
    assert dev._hip is not None and ref._hip is None
    return dev, ref


@pytest.mark.gpu
@pytest.mark.parametrize("use_dueling", [True, False], ids=["dueling", "plain"])
def test_drqn_device_path_matches_the_torch_path_in_a_battle(use_dueling):
    """24 steps of a battle on the HIP engine with device observations: both sides act through the kernel model; the PyTorch-path model
    of side 0 is fed the same observations and ids.  Q (and the states) agree within float32 round-off, greedy actions are equal except at
    near-ties, e-greedy actions are equal wherever the greedy ones are (same torch seed), agent_states keys are the PyTorch path's"""
    import torch
    env, hs = _battle(11)
    dev, ref = _models(env, hs[0], use_dueling)
    other = _models(env, hs[1], use_dueling)[0]
    near, total = 0, 0
    for step in range(24):
        view, feat = env.get_observation(hs[0])
        ids = env.get_agent_id(hs[0])
        assert dev._on_kernels(view, feat, len(ids))
        prev = ref.agent_states                  # Q of the PyTorch path's network for the states it is about to use
        zero = torch.zeros(S, device=view.device)
        with torch.no_grad():
            q_ref, _ = ref.qnet(view, feat, len(ids), 1, torch.stack([prev.get(int(i), zero) for i in ids]).unsqueeze(0))
        torch.manual_seed(1000 + step)
        a_dev = dev.infer_action((view, feat), ids, policy="e_greedy", eps=0.2)
        torch.manual_seed(1000 + step)
        a_ref = ref.infer_action((view, feat), ids, policy="e_greedy", eps=0.2)
        assert list(dev.agent_states.keys()) == list(ref.agent_states.keys())
        sd, sr = dev.agent_states, ref.agent_states
        for k in list(sd.keys())[:: max(1, len(sd) // 50)]:
            assert torch.allclose(sd[k], sr[k], atol=2e-5, rtol=0), (step, k)
        differ = (a_dev != a_ref).cpu().numpy()
        if differ.any():
            gap = np.sort(q_ref.cpu().numpy(), axis=1)
            gap = gap[:, -1] - gap[:, -2]
            scale = float(q_ref.abs().max())
            assert (gap[differ] <= 1e-4 * scale + 1e-6).all(), (step, gap[differ])
            near += int(differ.sum())
        total += len(ids)
        env.set_action(hs[0], a_dev)
        env.set_action(hs[1], other.infer_action(env.get_observation(hs[1]), env.get_agent_id(hs[1]), policy="e_greedy", eps=0.1))
        env.step()
        env.clear_dead()
    assert near <= total * 1e-3, (near, total)
    env.close()


@pytest.mark.gpu
def test_drqn_falls_back_to_torch_past_each_limit_and_on_request():
    import magent_amd
    from magent_amd.builtin.torch_model import DeepRecurrentQNetwork
    env, hs = _battle(3, n=20, size=20)
    vs, fs, A = env.get_view_space(hs[0]), env.get_feature_space(hs[0]), env.get_action_space(hs[0])[0]
    assert DeepRecurrentQNetwork(env, hs[0], "ok", memory_size=4)._hip is not None
    for cv, cf in (((vs[0], vs[1], 8), fs), (vs, (57,)), ((4, 4, vs[2]), fs)):
        m = DeepRecurrentQNetwork(env, hs[0], "past", memory_size=4, custom_view_space=cv, custom_feature_space=cf)
        assert m._hip is None, (cv, cf)
    old = os.environ.get("MAGENT_POLICY_F32")
    os.environ["MAGENT_POLICY_F32"] = "torch"
    try:
        assert DeepRecurrentQNetwork(env, hs[0], "t", memory_size=4)._hip is None
    finally:
        if old is None:
            del os.environ["MAGENT_POLICY_F32"]
        else:
            os.environ["MAGENT_POLICY_F32"] = old
    # numpy observations run the PyTorch path of a kernel model, with the same state table
    m = DeepRecurrentQNetwork(env, hs[0], "np", memory_size=4)
    view, feat = env.get_observation(hs[0])
    ids = env.get_agent_id(hs[0])
    m.infer_action((view, feat), ids, policy="greedy")
    keys = list(m.agent_states.keys())
    out = m.infer_action((view.cpu().numpy(), feat.cpu().numpy()), ids, policy="greedy")
    assert isinstance(out, np.ndarray) and list(m.agent_states.keys()) == keys
    m.infer_action((view, feat), ids, policy="greedy")         # the dict goes back into the device table
    assert list(m.agent_states.keys()) == keys
    m.agent_states = {}
    assert m.agent_states == {}
    assert A >= 1
    env.close()
