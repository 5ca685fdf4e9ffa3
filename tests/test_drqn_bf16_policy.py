"""The bf16 DRQN acting kernels (magent_amd/csrc/policy_drqn_bf16.hip: the bf16 DQN's trunk stopped after its hidden layer, k_drqn_gru_bf16,
k_drqn_head_bf16), their policy class (hip_policy.HipDrqnPolicy) and the public opt-in (DeepRecurrentQNetwork(infer_dtype="bf16")), against
a ROUNDING REFERENCE: one step of drqn.py's _RecurrentQNet in float64 that rounds to bfloat16 exactly where the kernels do -- the views, the
features, every weight matrix, conv1's bias, the two conv outputs, the two hidden halves, h as the GRU's operand and h' as the head's
operand -- and nowhere else (the other biases, the gates and the blend, which takes the unrounded h).  The kernels are never compared with
themselves or with the float32 kernels.

Two legs (helpers.policy_legs): `emu` runs policy.hip + policy_drqn_bf16.hip compiled as plain C++ against tests/hipemu on CPU tensors; `gpu`
(marked) runs the product library on cuda:0.  Every call is checked against the reference fed the kernels' OWN previous float32 states
(looked up with the dict path's semantics).

The bound.  The bf16 DQN test's form, per entry F_Q = 2e-3 max|Q_ref| + 2e-3 and, for h', F_h = 2e-3 max(1, max|h'_ref|) + 2e-3, was
checked first for being wide enough behind two more rounded layers (measure_spread below, CPU only): the rounding reference evaluated once
in float64 and once in float32 with torch's own summation order differs, over every case of this file, by up to 0.696 F_Q and 0.752 F_h (a
reordered sum flips a bf16 activation on a rounding boundary now and then, and the GRU and the head amplify the flip).  That is more than
a quarter of the form, so the bound is four times the largest spread (flips are heavy-tailed): with the spreads rounded up to 0.70 and 0.76,
|dQ| <= 2.8 F_Q = 5.6e-3 (max|Q_ref| + 1) and |dh'| <= 3.04 F_h = 6.08e-3 (max(1, max|h'_ref|) + 1).
test_reordering_spread_and_clear_agents prints the spread of the machine it runs on.
Actions equal the reference's argmax wherever its best two Q values are more than twice the bound apart, and always the argmax of the
kernels' own Q row; in cases with n >= 50 more than half of the agents are that clear (weights: the default init times 3, as the f32 test)."""
import ctypes
import os

import numpy as np
import pytest

import helpers as H

NAN, INF = float("nan"), float("inf")
S = 512
leg, LEGS = H.policy_legs(lambda: H.policy_emu("drqn_bf16"), policy_class="HipDrqnPolicy")
make_inputs, make_rnet, DictModel, cells_of, _Env, _battle = H.make_policy_inputs, H.make_rnet, H.DictModel, H.cells_of, H.SpacesEnv, H.battle


# ---------------------------------------------------------------------------------------------------- the rounding reference
def ref_step(net, view, feature, h, dtype=None):
    """one step of _RecurrentQNet.forward (batch n, unroll 1) rounding to bf16 at the kernels' points, everything between them in `dtype`
    (float64; float32 = torch's own float32 kernels and summation order, for the spread) -> (Q [n][A], h' [n][512]) as float64 NumPy"""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    bf = lambda t: t.to(torch.bfloat16).to(dtype)
    P = {k: v.detach().cpu().to(dtype) for k, v in net.state_dict().items()}
    x = bf(torch.as_tensor(view).to(dtype)).permute(0, 3, 1, 2)
    f = bf(torch.as_tensor(feature).to(dtype))
    h = torch.as_tensor(h).to(dtype)
    c1 = bf(torch.relu(F.conv2d(x, bf(P["conv1.weight"]), bf(P["conv1.bias"]))))
    c2 = bf(torch.relu(F.conv2d(c1, bf(P["conv2.weight"]), P["conv2.bias"])))
    flat = c2.permute(0, 2, 3, 1).reshape(c2.shape[0], -1)
    xh = torch.cat([bf(torch.relu(F.linear(flat, bf(P["dense_view.weight"]), P["dense_view.bias"]))),
                    bf(torch.relu(F.linear(f, bf(P["dense_emb.weight"]), P["dense_emb.bias"])))], dim=1)
    gi = F.linear(xh, bf(P["rnn.weight_ih_l0"]), P["rnn.bias_ih_l0"])
    gh = F.linear(bf(h), bf(P["rnn.weight_hh_l0"]), P["rnn.bias_hh_l0"])
    r = torch.sigmoid(gi[:, :S] + gh[:, :S])
    z = torch.sigmoid(gi[:, S:2 * S] + gh[:, S:2 * S])
    n_ = torch.tanh(gi[:, 2 * S:] + r * gh[:, 2 * S:])
    h2 = (1 - z) * n_ + z * h                                  # the unrounded h
    hb = bf(h2)
    value = F.linear(hb, bf(P["value.weight"]), P["value.bias"])
    if net.use_dueling:
        adv = F.linear(hb, bf(P["advantage.weight"]))
        value = value + adv - adv.mean(dim=1, keepdim=True)
    return value.double().numpy(), h2.double().numpy()


SPREAD_Q, SPREAD_H = 0.70, 0.76          # the largest float64 / float32 spread of the reference, in units of the DQN test's form (measured)


def bounds(q_ref, h_ref):
    """(the Q bound, the h' bound) of one call: four times the largest reordering spread (the module's docstring)"""
    fin = lambda a: a[np.isfinite(a)]
    qm = float(np.abs(fin(q_ref)).max()) if np.isfinite(q_ref).any() else 0.0
    hm = float(np.abs(fin(h_ref)).max()) if np.isfinite(h_ref).any() else 0.0
    return 4 * SPREAD_Q * (2e-3 * qm + 2e-3), 4 * SPREAD_H * (2e-3 * max(1.0, hm) + 2e-3)


def check_against_ref(tag, net, view, featv, h_prev, actions, q, h2, A, want_clear=False):
    """Q, h' and the actions of one call against the rounding reference fed `h_prev`; returns the worst |dQ| / bound, |dh'| / bound"""
    import torch
    q64, h64 = ref_step(net, view, featv, h_prev)
    bq, bh = bounds(q64, h64)
    a = actions.long()
    assert bool(((a >= 0) & (a < A)).all()), tag
    assert torch.equal(a, torch.from_numpy(q).argmax(dim=1)), tag
    worst = []
    for got, want, bound, what in ((q, q64, bq, "Q"), (h2, h64, bh, "h'")):
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), (tag, what, np.argwhere(np.isfinite(got) != np.isfinite(want))[:8])
        assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, what)
        ok = np.isfinite(want)
        d = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
        print("%s: worst |d%s| %.3g, bound %.3g" % (tag, what, d, bound))
        assert d <= bound, (tag, what, d, bound)
        worst.append(d / bound)
    rows = np.isfinite(q64).all(axis=1)
    if A > 1:
        top = np.sort(q64[rows], axis=1)
        clear = np.zeros(len(q64), bool)
        clear[rows] = top[:, -1] - top[:, -2] > 2 * bq
        assert np.array_equal(a.numpy()[clear], q64.argmax(axis=1)[clear]), tag
        if want_clear and len(q64) >= 50:
            assert clear.sum() * 2 > len(q64), (tag, int(clear.sum()), len(q64))      # (not a vacuous check)
    return worst


def step_and_check(lg, pol, net, dm, view, featv, ids, A, tag, cells=False, want_clear=False):
    """one kernel call of the policy, checked against the reference fed the looked-up kernel states; the table against the dict model"""
    import torch
    h_prev = dm.lookup(ids)
    ids_t = torch.as_tensor(np.asarray(ids, np.int32)).to(lg.dev)
    v_in = cells_of(view) if cells else view
    actions, q = pol.infer(v_in.to(lg.dev).contiguous(), featv.to(lg.dev).contiguous(), ids_t, want_q=True)
    lg.sync()
    actions, q, h2 = actions.cpu(), q.cpu().double().numpy(), pol._states.cpu().double().numpy()
    check_against_ref(tag, net, view, featv, h_prev, actions, q, h2, A, want_clear)
    dm.store(ids, h2.astype(np.float32))
    got = pol.states_dict()
    assert list(got.keys()) == list(dm.states.keys()), tag
    for k, v in got.items():
        assert np.array_equal(v.cpu().numpy(), dm.states[k], equal_nan=True), (tag, k)
    return actions, q, h2


# ---------------------------------------------------------------------------------------------------- 1. region and tiling
# (view_space, feat, n_action): the edges of policy_dqn_supported (the smallest view, view_c 1 / 7, feat 1 / 64, n_action 1 / 31, the
# 16 x 16 = 256-cell limit of a conv tile, a non-square view); n on the emulator 1, 5, 33; on the GPU 1, 129 (a head group of 128 + 1),
# 257 (the GRU workgroup's 256 agents + 1), 301 (no multiple of 4 or 32), 70
CASES = [((5, 5, 1), 1, 1), ((13, 13, 7), 34, 21), ((9, 9, 2), 64, 31), ((16, 16, 4), 36, 13), ((12, 13, 5), 9, 17)]
EMU_N = [1, 33, 5, 5, 33]
GPU_N = [1, 129, 257, 301, 70]


def region_case(k, dueling, lg_name):
    vs, feat, A = CASES[k]
    return vs, feat, A, (GPU_N if lg_name == "gpu" else EMU_N)[k], 10 + k + (100 if dueling else 0)


@pytest.mark.parametrize("lg", LEGS)
@pytest.mark.parametrize("cells", [False, True], ids=["f32views", "bf16cells"])
@pytest.mark.parametrize("dueling", [True, False], ids=["dueling", "plain"])
@pytest.mark.parametrize("k", range(len(CASES)), ids=lambda k: "%dx%dx%d-f%d-a%d" % (CASES[k][0] + CASES[k][1:]))
def test_drqn_bf16_against_the_rounding_reference_over_the_region(lg, cells, dueling, k):
    """two calls: an empty table (the kernel's variant without the h half), then ids kept, dropped and added"""
    lg = leg(lg)
    vs, feat, A, n, seed = region_case(k, dueling, lg.name)
    net = make_rnet(vs, feat, A, dueling, seed, lg.dev)
    pol = lg.policy(net, vs, feat, A)
    dm = DictModel()
    rs = np.random.RandomState(seed)
    ids = np.arange(n, dtype=np.int32) * 3
    for call in range(2):
        view, featv = make_inputs(vs, feat, len(ids), seed * 7 + call)
        step_and_check(lg, pol, net, dm, view, featv, ids, A, "%s %s call %d" % (lg.name, CASES[k], call), cells=cells, want_clear=True)
        keep = ids[rs.rand(len(ids)) < 0.7]
        ids = np.concatenate([keep, np.arange(2) + 1000 * (call + 1)]).astype(np.int32)


@pytest.mark.parametrize("lg", LEGS)
def test_drqn_bf16_three_chunks(lg):
    """chunk= small enough for three chunks: all of them read the same previous table"""
    lg = leg(lg)
    vs, feat, A = (9, 9, 3), 12, 9
    n = 11 if lg.name == "emu" else 300
    net = make_rnet(vs, feat, A, True, 41, lg.dev)
    pol = lg.policy(net, vs, feat, A, chunk=(n + 2) // 3)
    dm = DictModel()
    for call, ids in enumerate((np.arange(n), np.arange(n)[::-1] + 2)):
        view, featv = make_inputs(vs, feat, n, 60 + call)
        step_and_check(lg, pol, net, dm, view, featv, ids.astype(np.int32), A, "%s chunks call %d" % (lg.name, call), cells=bool(call), want_clear=True)


GRID3 = """
import os, sys
os.environ["MAGENT_TUNE"] = "policy_grid=3"
sys.path[:0] = [%r, %r]
import numpy as np
import test_drqn_bf16_policy as T
lg = T.leg(sys.argv[1])
vs, feat, A = (7, 7, 4), 10, 7
n = 30 if lg.name == "emu" else 200
net = T.make_rnet(vs, feat, A, True, 43, lg.dev)
pol = lg.policy(net, vs, feat, A)
dm = T.DictModel()
for call in range(2):
    view, featv = T.make_inputs(vs, feat, n, 70 + call)
    T.step_and_check(lg, pol, net, dm, view, featv, np.arange(n, dtype=np.int32), A, "grid3 call %%d" %% call, cells=bool(call), want_clear=True)
print("grid3 ok")
"""


@pytest.mark.parametrize("lg", LEGS)
def test_drqn_bf16_few_workgroups_walk_many_conv_tiles(lg):
    """MAGENT_TUNE=policy_grid=3 (read once, at the library's first call: a process of its own): three conv workgroups walk every tile"""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-c", GRID3 % (os.path.dirname(os.path.abspath(__file__)), H.ROOT), lg], capture_output=True, text=True)
    assert out.returncode == 0 and "grid3 ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------- 2. the state table over calls
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
def test_drqn_bf16_state_table_over_calls(lg):
    """the call sequence of test_drqn_state_table_over_calls; agent_states' assignment is the policy's load_states (a dict mid-sequence, {})"""
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
        if k == 3:                   # states assigned mid-sequence: the dict goes through load_states and comes back the same
            given = {int(i): np.float32(0.25) * v for i, v in dm.states.items()}
            pol.load_states(given)
            dm.states = given
        view, featv = make_inputs(vs, feat, len(ids), 50 + k)
        prev = dm.lookup(ids)
        step_and_check(lg, pol, net, dm, view, featv, ids, A, "%s ids call %d" % (lg.name, k), cells=bool(k & 1))
        if k == 5:
            assert not prev.any()        # every id starts from zeros after the table was emptied
        if k == 3:
            assert prev.all(axis=1).any() and np.array_equal(prev[0], given[9])       # the assigned states are the ones looked up


# ---------------------------------------------------------------------------------------------------- 3. switching paths with states
@pytest.mark.parametrize("lg", LEGS)
def test_drqn_states_move_between_the_f32_and_the_bf16_path(lg):
    """two steps on HipDrqnPolicyF32, its states handed to a bf16 policy of the same weights, which continues (checked against the
    rounding reference started from those states); then the reverse: the bf16 policy's states continue on the f32 kernels (checked
    against the unrounded float64 network within float32 round-off, 1e-4 of max |Q|)"""
    import torch
    from magent_amd.builtin.torch_model import hip_policy
    lg = leg(lg)
    lib32 = None
    if lg.name == "emu":
        lib32 = ctypes.CDLL(H.policy_emu("drqn"), mode=os.RTLD_LOCAL)
        from magent_amd import c_lib
        c_lib.declare_policy(lib32)
    vs, feat, A = (9, 9, 3), 12, 9
    n = 9 if lg.name == "emu" else 140
    net = make_rnet(vs, feat, A, True, 17, lg.dev)
    p32 = hip_policy.HipDrqnPolicyF32(net, vs, (feat,), A, lg.dev, lib=lib32)
    p16 = lg.policy(net, vs, feat, A)
    ids = np.arange(n, dtype=np.int32) + 5
    ids_t = torch.as_tensor(ids).to(lg.dev)
    for call in range(2):
        view, featv = make_inputs(vs, feat, n, 80 + call)
        p32.infer(view.to(lg.dev), featv.to(lg.dev), ids_t)
    lg.sync()
    handed = p32.states_dict()
    assert type(p32)._set_table is type(p16)._set_table          # one table implementation
    p16.load_states(handed)
    dm = DictModel()
    dm.states = {k: v.cpu().numpy() for k, v in handed.items()}
    assert any(np.abs(v).max() > 0.1 for v in dm.states.values())
    for call in range(2):
        view, featv = make_inputs(vs, feat, n, 90 + call)
        step_and_check(lg, p16, net, dm, view, featv, ids[::-1].copy(), A, "%s f32 -> bf16 call %d" % (lg.name, call), want_clear=True)
    # the reverse
    p32.load_states(p16.states_dict())
    view, featv = make_inputs(vs, feat, n, 95)
    h_prev = dm.lookup(ids)
    a, q = p32.infer(view.to(lg.dev), featv.to(lg.dev), ids_t, want_q=True)
    lg.sync()
    import test_drqn_policy as F32
    q64, h64 = F32.np_drqn_step(H.net_params(net), view.double().numpy(), featv.double().numpy(), h_prev, True)
    assert np.abs(q.cpu().double().numpy() - q64).max() <= 1e-4 * np.abs(q64).max() + 1e-6
    assert np.abs(p32._states.cpu().double().numpy() - h64).max() <= 1e-4


# ---------------------------------------------------------------------------------------------------- 4. non-finite values
def _run(lg, pol, view, featv, ids, states=None):
    import torch
    pol.load_states(states or {})
    a, q = pol.infer(view.to(lg.dev).contiguous(), featv.to(lg.dev).contiguous(), torch.as_tensor(ids).to(lg.dev), want_q=True)
    lg.sync()
    return a.cpu().numpy(), q.cpu().numpy(), pol._states.cpu().numpy()


@pytest.mark.parametrize("lg", LEGS)
def test_drqn_bf16_non_finite_values_stay_with_their_agent(lg):
    """a NaN / Inf in one agent's view, feature or state (they occur in diverged training): every action in range, the poisoned agent's Q
    row and h' non-finite, every other agent's outputs bit-equal to the run without the poison; a non-finite row of weight_hh_l0 with an
    empty table reaches every agent (torch's W_h @ 0)"""
    import torch
    lg = leg(lg)
    vs, feat, A = (7, 7, 4), 10, 7
    n = 40 if lg.name == "emu" else 300
    net = make_rnet(vs, feat, A, True, 21, lg.dev)
    pol = lg.policy(net, vs, feat, A)
    ids = np.arange(n, dtype=np.int32) + 100
    view, featv = make_inputs(vs, feat, n, 3)
    rs = np.random.RandomState(1)
    states = {int(i): (rs.rand(S).astype(np.float32) - 0.5) for i in ids}
    for cells in (False, True):
        vin = (lambda v: cells_of(v)) if cells else (lambda v: v)
        a0, q0, h0 = _run(lg, pol, vin(view), featv, ids, states)
        assert np.isfinite(q0).all() and np.isfinite(h0).all()
        for what, agent, value in (("view", 0, NAN), ("view", 33, -INF), ("feature", 31, INF), ("state", 32, NAN), ("state", n - 1, INF)):
            v2, f2, s2 = view.clone(), featv.clone(), dict(states)
            if what == "view":
                v2[agent, 3, 3, 1] = value
            elif what == "feature":
                f2[agent, 4] = value
            else:
                s2[int(ids[agent])] = states[int(ids[agent])].copy()
                s2[int(ids[agent])][77] = value
            a1, q1, h1 = _run(lg, pol, vin(v2), f2, ids, s2)
            tag = (lg.name, cells, what, agent)
            assert ((a1 >= 0) & (a1 < A)).all(), tag
            assert not np.isfinite(q1[agent]).any() and not np.isfinite(h1[agent]).all(), tag
            others = np.arange(n) != agent
            assert np.array_equal(a1[others], a0[others]) and np.array_equal(q1[others].view(np.int32), q0[others].view(np.int32)), tag
            assert np.array_equal(h1[others].view(np.int32), h0[others].view(np.int32)), tag
    # a non-finite weight in weight_hh_l0 (gate z, unit 77) with an empty table: unit 77 of every agent's h' is NaN, as torch's W_h @ 0.
    # 3.4e38 is finite in float32 and rounds to Inf in bf16: gru_bias0 is computed from the rounded weights
    for value in (NAN, 3.4e38):
        with torch.no_grad():
            net.rnn.weight_hh_l0[S + 77, 5] = value
        a1, q1, h1 = _run(lg, pol, view[:5], featv[:5], ids[:5])
        assert ((a1 >= 0) & (a1 < A)).all() and np.isnan(h1[:, 77]).all() and not np.isfinite(q1).any()
        assert np.isfinite(np.delete(h1, 77, axis=1)).all()
        q64, h64 = ref_step(net, view[:5], featv[:5], np.zeros((5, S), np.float32))
        assert np.array_equal(np.isnan(h64), np.isnan(h1))


# ---------------------------------------------------------------------------------------------------- 5. nothing outside the buffers
@pytest.mark.parametrize("lg", LEGS)
def test_drqn_bf16_writes_nothing_outside_its_buffers(lg):
    """guard rows of a sentinel behind new_states, actions, q and the workspace, NaN observation rows behind n: the guards are unchanged
    and the results unaffected; a refused call (unsupported shape, NULL actions, a buffer misaligned by 4 bytes) writes nothing"""
    import torch
    lg = leg(lg)
    vs, feat, A = (8, 7, 5), 6, 11
    n, extra = 37, 5
    net = make_rnet(vs, feat, A, True, 31, lg.dev)
    pol = lg.policy(net, vs, feat, A)
    view, featv = make_inputs(vs, feat, n, 8, extra=extra, fill=NAN)
    for cells in (False, True):
        vdev = (cells_of(view) if cells else view).to(lg.dev).contiguous()
        fdev = featv.to(lg.dev)
        entry = lg.lib.policy_drqn_infer_bf16 if cells else lg.lib.policy_drqn_infer
        ids = torch.arange(n, dtype=torch.int32, device=lg.dev) * 2
        pol.load_states({})
        pol.infer(vdev[:n].contiguous(), fdev[:n].contiguous(), ids)            # a table of n rows
        lg.sync()
        table = [t.clone() for t in (pol._sorted, pol._rows, pol._states)]
        PAD, SP = 333, 332                     # (state rows are float4-aligned: the entry refuses a misaligned table)
        acts = torch.full((n + 2 * PAD,), -7, dtype=torch.int32, device=lg.dev)
        q = torch.full((n * A + 2 * PAD,), -77.0, device=lg.dev)
        st = torch.full((n * S + 2 * SP,), -777.0, device=lg.dev)
        nb = ctypes.c_size_t(0)
        lg.lib.policy_drqn_workspace_bytes(ctypes.byref(pol.shape), n, ctypes.byref(nb))
        work = torch.full((nb.value + 2 * 4096,), 0x5A, dtype=torch.uint8, device=lg.dev)
        ids2 = torch.flip(ids, [0]).contiguous()
        args = lambda shape, new_states, workspace, actions: (
            ctypes.byref(shape), ctypes.byref(pol._w), vdev.data_ptr(), fdev.data_ptr(), n, ids2.data_ptr(), pol._sorted.data_ptr(),
            pol._rows.data_ptr(), pol._states.data_ptr(), n, new_states, workspace, actions, q[PAD:].data_ptr(), None)
        # refused calls first: nothing is written
        bad = type(pol.shape)(vs[0], vs[1], 8, feat, A)
        assert lg.lib.policy_drqn_supported(ctypes.byref(bad)) == 0
        assert entry(*args(bad, st[SP:].data_ptr(), work[4096:].data_ptr(), acts[PAD:].data_ptr())) != 0
        assert entry(*args(pol.shape, st[SP:].data_ptr(), work[4096:].data_ptr(), None)) != 0
        assert entry(*args(pol.shape, st[SP + 1:].data_ptr(), work[4096:].data_ptr(), acts[PAD:].data_ptr())) != 0
        assert entry(*args(pol.shape, st[SP:].data_ptr(), work[4100:].data_ptr(), acts[PAD:].data_ptr())) != 0
        lg.sync()
        assert bool((acts == -7).all()) and bool((q == -77.0).all()) and bool((st == -777.0).all()) and bool((work == 0x5A).all())
        rc = entry(*args(pol.shape, st[SP:].data_ptr(), work[4096:].data_ptr(), acts[PAD:].data_ptr()))
        lg.sync()
        assert rc == 0
        for buf, fill, m, pad in ((acts, -7, n, PAD), (q, -77.0, n * A, PAD), (st, -777.0, n * S, SP)):
            assert bool((buf[:pad] == fill).all()) and bool((buf[pad + m:] == fill).all())
            assert not bool((buf[pad:pad + m] == fill).any())
        assert bool((work[:4096] == 0x5A).all()) and bool((work[4096 + nb.value:] == 0x5A).all())
        for a, b in zip(table, (pol._sorted, pol._rows, pol._states)):
            assert torch.equal(a, b)
        # the same step through the wrapper, without the NaN rows behind n: the same bits
        a2, q2 = pol.infer(vdev[:n].contiguous(), fdev[:n].contiguous(), ids2, want_q=True)
        lg.sync()
        assert torch.equal(a2, acts[PAD:PAD + n]) and torch.equal(q2.reshape(-1), q[PAD:PAD + n * A])
        assert torch.equal(pol._states.reshape(-1), st[SP:SP + n * S]) and bool(torch.isfinite(q2).all())


def test_drqn_bf16_supported_is_the_dqn_region():
    from magent_amd.builtin.torch_model.hip_policy import _Shape
    lg = leg("emu")
    for h in range(3, 24, 2):
        for w in range(3, 24, 3):
            for c, feat, A in ((7, 34, 21), (1, 64, 31), (8, 34, 21), (7, 65, 21), (7, 34, 32), (7, 34, 0)):
                s = _Shape(h, w, c, feat, A)
                assert lg.lib.policy_drqn_supported(ctypes.byref(s)) == lg.lib.policy_dqn_supported(ctypes.byref(s))


# ---------------------------------------------------------------------------------------------------- 6. the documented packing
def test_drqn_bf16_weight_packing_is_the_documented_permutation():
    """CPU-only: include/magent_policy.h's PolicyDrqnWeights, checked by undoing it -- gru: k-step s, tile 3 T + G, lane l holds the weight
    of gate G's unit 32 T + (l & 31) at k = 16 s + 8 (l >> 5) + e; k < 512: x's hidden slot k (weight_ih_l0's column of that slot's unit),
    k >= 512: unit k - 512 of weight_hh_l0.  head: natural order of the 512 state units"""
    import torch
    from magent_amd.builtin.torch_model.hip_policy import HipDrqnPolicy, slot_channels
    vs, feat, A = (13, 13, 7), 34, 21
    net = make_rnet(vs, feat, A, True, 3, scale=1.0)
    with torch.no_grad():
        net.rnn.weight_hh_l0[2 * S + 9, 100] = 3.4e38         # (finite in float32, Inf in bf16)
    pol = HipDrqnPolicy(net, vs, (feat,), A, "cpu")
    pol.pack()
    t = pol._packed
    assert t["gru"].shape == (64, 48, 64, 8) and t["gru"].dtype == torch.bfloat16 and t["head"].shape == (32, 1, 64, 8)
    assert t["dense_view"].shape == (162, 8, 64, 8) and t["gru_bias"].shape == (4, S) and t["head_bias"].shape == (32,)
    ch = slot_channels("cpu")
    bf = lambda x: x.detach().to(torch.bfloat16).float()
    g = t["gru"].float()
    get = lambda gate, unit, k: g[k // 16, 3 * (unit // 32) + gate, 32 * ((k % 16) // 8) + unit % 32, k % 8]
    unit_of = lambda slot: (slot // 32) * 32 + int(ch[slot % 32])
    wih, whh = bf(net.rnn.weight_ih_l0), bf(net.rnn.weight_hh_l0)
    for gate, unit, k in ((0, 0, 0), (1, 77, 5 * 32 + 30), (2, 511, 256 + 2 * 32 + 1), (0, 300, 511), (2, 33, 17)):
        assert get(gate, unit, k) == wih[gate * S + unit, unit_of(k)], (gate, unit, k)
    for gate, unit, k in ((0, 0, 0), (1, 77, 190), (2, 511, 511), (2, 9, 100)):
        assert get(gate, unit, S + k) == whh[gate * S + unit, k], (gate, unit, k)
    hd = t["head"].float()
    geth = lambda o, k: hd[k // 16, 0, 32 * ((k % 16) // 8) + o, k % 8]
    assert geth(4, 190) == bf(net.advantage.weight)[4, 190] and geth(A, 300) == bf(net.value.weight)[0, 300] and geth(A + 1, 77) == 0
    assert t["head_bias"][A] == net.value.bias[0] and t["head_bias"][0] == 0
    bih, bhh = net.rnn.bias_ih_l0.detach(), net.rnn.bias_hh_l0.detach()
    assert torch.equal(t["gru_bias"][0], bih[:S] + bhh[:S]) and torch.equal(t["gru_bias"][2], bih[2 * S:]) and torch.equal(t["gru_bias"][3], bhh[2 * S:])
    b0 = t["gru_bias0"]
    assert torch.isnan(b0[3, 9]) and int(torch.isnan(b0).sum()) == 1 and torch.equal(torch.nan_to_num(b0), torch.nan_to_num(t["gru_bias"]) * (~torch.isnan(b0)))
    # the trunk is the bf16 DQN's own packing: the hidden slots x is stored in are the ones its head reads
    assert torch.equal(t["dense_view_bias"][3 * 32 + 21], net.dense_view.bias[3 * 32 + int(ch[21])])


# ---------------------------------------------------------------------------------------------------- the bound's precondition
def spread_cases():
    """every (net, view, feature, h) the reference is evaluated on above, on the emulator's sizes and the GPU's"""
    rs = np.random.RandomState(0)
    for name in ("emu", "gpu"):
        for k in range(len(CASES)):
            for dueling in (True, False):
                vs, feat, A, n, seed = region_case(k, dueling, name)
                net = make_rnet(vs, feat, A, dueling, seed)
                for call in range(2):
                    view, featv = make_inputs(vs, feat, n, seed * 7 + call)
                    h = np.zeros((n, S), np.float32) if call == 0 else (rs.rand(n, S).astype(np.float32) * 2 - 1)
                    yield "%s %s %s %d" % (name, CASES[k], dueling, call), net, view, featv, h
    for vs, feat, A, n, seed, iseed in (((9, 9, 3), 12, 9, 300, 41, 60), ((7, 7, 4), 10, 7, 200, 43, 70), ((9, 9, 3), 12, 9, 10, 7, 50),
                                        ((9, 9, 3), 12, 9, 140, 17, 90), ((7, 7, 4), 10, 7, 300, 21, 3), ((8, 7, 5), 6, 11, 37, 31, 8)):
        net = make_rnet(vs, feat, A, True, seed)
        view, featv = make_inputs(vs, feat, n, iseed)
        yield "%s seed %d" % (vs, seed), net, view, featv, rs.rand(n, S).astype(np.float32) * 2 - 1


def measure_spread():
    """(largest |Q_f64 - Q_f32| / F_Q, the same for h' and F_h: in units of the DQN test's form) of the rounding reference over spread_cases, and whether the reference alone has
    more than half of the agents clear in the cases with n >= 50"""
    import torch
    worst_q, worst_h, least_clear = 0.0, 0.0, 1.0
    for tag, net, view, featv, h in spread_cases():
        q64, h64 = ref_step(net, view, featv, h)
        q32, h32 = ref_step(net, view, featv, h, torch.float32)
        bq, bh = bounds(q64, h64)
        sq, sh = float(np.abs(q64 - q32).max()) / bq * 4 * SPREAD_Q, float(np.abs(h64 - h32).max()) / bh * 4 * SPREAD_H
        worst_q, worst_h = max(worst_q, sq), max(worst_h, sh)
        if len(q64) >= 50 and q64.shape[1] > 1:
            top = np.sort(q64, axis=1)
            least_clear = min(least_clear, float((top[:, -1] - top[:, -2] > 2 * bq).mean()))
        print("%-40s spread Q %.3f h' %.3f of the form" % (tag, sq, sh))
    return worst_q, worst_h, least_clear


def test_reordering_spread_and_clear_agents():
    """CPU-only.  The reference alone has more than half of the agents clear wherever n >= 50 (measured: at least 0.8 of them), so the
    action check is not vacuous.  The reordering spread is printed; it was 0.696 F_Q and 0.752 F_h where the bound was set (a quarter of the
    bound is 0.70 / 0.76).  Another CPU sums in another order, so only half of the bound is asserted here."""
    worst_q, worst_h, least_clear = measure_spread()
    print("largest spread: Q %.3f F_Q, h' %.3f F_h; least share of clear agents %.3f" % (worst_q, worst_h, least_clear))
    assert worst_q <= 2 * SPREAD_Q and worst_h <= 2 * SPREAD_H and least_clear > 0.5


# ---------------------------------------------------------------------------------------------------- 7. the public class, CPU only
def test_public_class_takes_infer_dtype_on_the_cpu(monkeypatch):
    import torch
    from magent_amd.builtin.torch_model import DeepRecurrentQNetwork
    env = _Env()
    torch.manual_seed(2)
    m = DeepRecurrentQNetwork(env, 0, "x", infer_dtype="bf16", device="cpu", memory_size=4)
    assert m.infer_dtype == "bf16" and m._hip is None and not m.bf16_kernels
    with pytest.raises(ValueError):
        DeepRecurrentQNetwork(env, 0, "x", infer_dtype="fp8", device="cpu", memory_size=4)
    monkeypatch.setenv("MAGENT_POLICY_DTYPE", "bf16")
    assert DeepRecurrentQNetwork(env, 0, "x", device="cpu", memory_size=4).infer_dtype == "bf16"
    assert DeepRecurrentQNetwork(env, 0, "x", device="cpu", memory_size=4, infer_dtype="f32").infer_dtype == "f32"
    monkeypatch.setenv("MAGENT_POLICY_DTYPE", "int4")
    with pytest.raises(ValueError):
        DeepRecurrentQNetwork(env, 0, "x", device="cpu", memory_size=4)
    monkeypatch.delenv("MAGENT_POLICY_DTYPE")
    assert DeepRecurrentQNetwork(env, 0, "x", device="cpu", memory_size=4).infer_dtype == "f32"
    # acts through PyTorch; a bfloat16 cell tensor gives the actions of the float32 channels it carries, and the same states
    n = 12
    view, featv = make_inputs(env.vs, env.feat, n, 5)
    ids = np.arange(n, dtype=np.int32)
    cells = cells_of(view)
    carried = cells[..., :env.vs[2]].float()
    a_ref = m.infer_action((carried, featv), ids, policy="greedy")
    s_ref = {k: v.clone() for k, v in m.agent_states.items()}
    m.agent_states = {}
    a = m.infer_action((cells, featv), ids, policy="greedy")
    assert isinstance(a, torch.Tensor) and torch.equal(a, a_ref) and a.shape == (n,)
    assert list(m.agent_states.keys()) == list(s_ref.keys()) and all(torch.equal(m.agent_states[k], s_ref[k]) for k in s_ref)
    q, _ = m.qnet(carried, featv, n, 1, torch.zeros(1, n, S))
    assert torch.equal(a.long(), q.argmax(dim=1))


# ---------------------------------------------------------------------------------------------------- 8. / 9. the public class on the GPU
def _torch_model(env, h, name, **kw):
    from magent_amd.builtin.torch_model import DeepRecurrentQNetwork
    old = os.environ.get("MAGENT_POLICY_F32")
    os.environ["MAGENT_POLICY_F32"] = "torch"
    try:
        return DeepRecurrentQNetwork(env, h, name, memory_size=4, **kw)
    finally:
        if old is None:
            del os.environ["MAGENT_POLICY_F32"]
        else:
            os.environ["MAGENT_POLICY_F32"] = old


@pytest.mark.gpu
@pytest.mark.parametrize("device_obs", ["bf16", True], ids=["bf16cells", "f32views"])
def test_bf16_model_in_a_battle(device_obs):
    """6 steps of a 40 x 40 battle, ~300 agents a side: a bf16 model and a PyTorch model with the same weights see the same observations.
    The bf16 model's Q are within the bound of the rounding reference at every step (fed the model's own states, carried by id across
    deaths).  REPORTED, not asserted (a property of bf16, not of the code): the largest |dQ| / max|Q| and the share of equal greedy
    actions against the float32 PyTorch network after the 6 steps."""
    import torch
    from magent_amd.builtin.torch_model import DeepRecurrentQNetwork
    env, hs = _battle(11, device_obs)
    torch.manual_seed(5)
    dev = DeepRecurrentQNetwork(env, hs[0], "dev", memory_size=4, infer_dtype="bf16")
    ref = _torch_model(env, hs[0], "ref")
    ref.qnet.load_state_dict(dev.qnet.state_dict())
    assert dev.bf16_kernels and ref._hip is None
    A = dev.num_actions
    cpu_net = make_rnet(dev.view_space, dev.feature_space[0], A, True, 0, scale=1.0)
    cpu_net.load_state_dict(dev.qnet.state_dict())
    dm = DictModel()
    deaths = 0
    for step in range(6):
        view, feat = env.get_observation(hs[0])
        ids = env.get_agent_id(hs[0])
        n = len(ids)
        assert dev._on_kernels(view, feat, n) and (view.dtype == torch.bfloat16) == (device_obs == "bf16")
        view32 = view[..., :dev.view_space[2]].float() if view.dtype == torch.bfloat16 else view
        h_prev = dm.lookup(ids)
        deaths += int(len(dm.states) > 0 and len(dm.states) != n)
        a_dev = dev.infer_action((view, feat), ids, policy="greedy")
        a_ref = ref.infer_action((view32, feat), ids, policy="greedy")
        # the kernels' Q of this very call: the same step again from the same table (the states are float32 rows, restored after it)
        table = dev.agent_states
        h2 = np.stack([table[int(i)].cpu().numpy() for i in ids])
        dev._hip.load_states({k: torch.from_numpy(v) for k, v in dm.states.items()})       # the previous table, dead ids included
        a_again, q = dev._hip.infer(view, feat, torch.as_tensor(np.asarray(ids, np.int32)).to(view.device), want_q=True)
        dev._agent_states = None
        torch.cuda.synchronize()
        assert torch.equal(a_again, a_dev) and list(dev.agent_states.keys()) == [int(i) for i in ids]
        assert np.array_equal(dev._hip._states.cpu().numpy(), h2)
        check_against_ref("battle step %d" % step, cpu_net, view32.cpu(), feat.cpu(), h_prev, a_dev.cpu(), q.cpu().double().numpy(),
                          h2.astype(np.float64), A)
        dm.store(ids, h2)
        env.set_action(hs[0], a_dev)
        env.set_action(hs[1], torch.randint(A, (len(env.get_agent_id(hs[1])),), dtype=torch.int32, device=view.device))
        env.step()
        env.clear_dead()
    # against the float32 PyTorch network, fed its own states: reported only
    zero = torch.zeros(S, device=view.device)
    prev = ref.agent_states
    view, feat = env.get_observation(hs[0])
    ids = env.get_agent_id(hs[0])
    view32 = view[..., :dev.view_space[2]].float() if view.dtype == torch.bfloat16 else view
    with torch.no_grad():
        q_ref, _ = ref.qnet(view32, feat, len(ids), 1, torch.stack([prev.get(int(i), zero) for i in ids]).unsqueeze(0))
    _, q_dev = dev._hip.infer(view, feat, torch.as_tensor(np.asarray(ids, np.int32)).to(view.device), want_q=True)
    print("bf16 DRQN against the float32 PyTorch network after 6 steps (%s): largest |dQ| / max|Q| %.4f, equal greedy actions %.4f (n %d, ids lost %d)"
          % (device_obs, float((q_dev - q_ref).abs().max() / q_ref.abs().max()), float((q_dev.argmax(1) == q_ref.argmax(1)).float().mean()), len(ids), deaths))
    env.close()


@pytest.mark.gpu
def test_bf16_model_falls_back_past_each_limit_and_on_request():
    """view_c = 8, feat = 65 and n_action = 32 construct, act through the existing paths and say that the bf16 kernels are not in use;
    MAGENT_POLICY_F32=torch keeps PyTorch (where the bf16 kernels do not take the shape)"""
    import torch
    from magent_amd.builtin.torch_model import DeepRecurrentQNetwork
    from magent_amd.builtin.torch_model import hip_policy
    dev = torch.device("cuda", 0)
    ok = DeepRecurrentQNetwork(_Env(), 0, "ok", memory_size=4, infer_dtype="bf16")
    assert ok.bf16_kernels and isinstance(ok._hip, hip_policy.HipDrqnPolicy)
    assert not DeepRecurrentQNetwork(_Env(), 0, "f32", memory_size=4).bf16_kernels
    for env in (_Env(vs=(9, 9, 8)), _Env(feat=65), _Env(A=32)):
        torch.manual_seed(3)
        m = DeepRecurrentQNetwork(env, 0, "past", memory_size=4, infer_dtype="bf16")
        assert not m.bf16_kernels and not isinstance(m._hip, hip_policy.HipDrqnPolicy)
        n = 20
        view, featv = make_inputs(env.vs, env.feat, n, 9)
        view, featv = view.to(dev), featv.to(dev)
        ids = np.arange(n, dtype=np.int32)
        a = m.infer_action((view, featv), ids, policy="greedy")
        with torch.no_grad():
            q, _ = m.qnet(view, featv, n, 1, torch.zeros(1, n, S, device=dev))
        top = q.sort(dim=1).values
        clear = (top[:, -1] - top[:, -2]) > 1e-4 * float(q.abs().max())
        assert torch.equal(a.long()[clear], q.argmax(dim=1)[clear]) and bool(clear.any())
        if env.vs[2] <= 7:       # bf16 cells on a model without the bf16 kernels: the channels go back to float32
            m.agent_states = {}
            a16 = m.infer_action((cells_of(view.cpu()).to(dev), featv), ids, policy="greedy")
            with torch.no_grad():
                q16, _ = m.qnet(view.to(torch.bfloat16).float(), featv, n, 1, torch.zeros(1, n, S, device=dev))
            top = q16.sort(dim=1).values
            clear = (top[:, -1] - top[:, -2]) > 1e-4 * float(q16.abs().max())
            assert torch.equal(a16.long()[clear], q16.argmax(dim=1)[clear])
    t = _torch_model(_Env(feat=65), 0, "t", infer_dtype="bf16")
    assert t._hip is None and not t.bf16_kernels


if __name__ == "__main__":
    print(measure_spread())
