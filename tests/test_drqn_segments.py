"""The segmented DRQN acting step (include/magent_policy.h: policy_drqn_lookup_seg_f32 / policy_drqn_lookup_seg, then
policy_drqn_infer_f32_rows / policy_drqn_infer_rows / policy_drqn_infer_bf16_rows; the bindings' `segments=`, forget_segments and the
(segment, id) table of hip_policy._DrqnPolicy): ONE call over a packed buffer of several worlds' rows, every world with its own id
namespace.

The main criterion needs no tolerance: over a sequence of calls the actions, Q and h' of a segment's rows are, bit for bit, those of the
PLAIN entry called on that segment's rows alone by a plain policy object of that world, which carries that world's own id table.  The
plain entries are checked against float64 / the rounding reference by test_drqn_policy.py and test_drqn_bf16_policy.py; one segmented call
per leg and kind goes through the same restatements and bounds here (imported, not copied).

Two legs (helpers.policy_legs, the modules' own): `emu` runs the kernels compiled as plain C++ against tests/hipemu on CPU tensors, `gpu`
(marked) the product library.  Three kinds: the float32 kernels, the bf16 kernels on float32 views and on the engine's bf16 cells.

Shapes: network (5, 5, 3) / 7 features / 9 actions, dueling.  test_a2c_segments.lay_out's layout "a": counts [1, 0, 33, 257, 2] at rows 4,
8, 8, 52, 312 of 322 -- an agent alone, an empty world, a segment across a 32-row MFMA tile and a 4-agent conv tile, one across the GRU's
256-agent workgroup and the head's 128-agent group at rows that are no multiple of either, stale rows behind segments and a tail.  Gap
rows hold random values (NaN in every third of them) and ids 0..4, which collide with living agents' ids.  The segmented policy of the
sequence runs with chunk = 96: its GRU steps are cut inside segments, the look-up is one launch all the same.

The sequence (CALLS): ids arange(count) in every world (they collide across worlds); shrunken counts with non-contiguous surviving ids,
begins unchanged; duplicates, a shuffled world and a new id inside one world; one world forgotten with forget_segments, its ids
restarting at 0.

No kernel makes a row's bits depend on its position (MFMA columns are independent; a lane without a state feeds zeros through the same
MFMAs): the criterion holds for all three kinds.

Planted defects that the emulator leg of test_segments_equal_the_plain_call_per_world catches (each tried, each fails by a bit
difference): the look-up ignoring the segment (the key built with segment 0 for every row: call 1, world 0); the first duplicate found
instead of the last (state_row_of_key returning the first equal entry: call 3, world 2, which reads the duplicated ids back); a gap row's
state entering the table under its id (the gap rows' key built as drqn_key(0, id): world 0's agent 0 reads a gap row in call 1); from_row
indexed by chunk-relative row (from_row passed without [beg:] in _DrqnPolicy._step: call 1, world 3, behind the first chunk)."""
import ctypes

import numpy as np
import pytest

import helpers as H
import test_drqn_bf16_policy as B16
import test_drqn_policy as F32
from test_a2c_segments import lay_out

NAN = float("nan")
S = 512
LEGS = F32.LEGS
KINDS = ["f32", "bf16", "cells"]          # the float32 kernels; the bf16 kernels on float32 views; on bf16 cells
VS, FEAT, A = (5, 5, 3), 7, 9
MAX_SEGMENTS = 256                        # include/magent_policy.h: POLICY_A2C_MAX_SEGMENTS
NO_KEY = 0x7FFFFFFFFFFFFFFF
SEG, N = lay_out([1, 0, 33, 257, 2], stale={2: 2})
assert SEG.tolist() == [[4, 1], [8, 0], [8, 33], [52, 257], [312, 2]] and N == 322
BEGIN = SEG[:, 0].tolist()


def the_leg(kind, name):
    return (F32.leg if kind == "f32" else B16.leg)(name)


def calls():
    """the sequence: per call (the worlds forgotten in front of it, the ids of every world)"""
    rs = np.random.RandomState(5)
    w2 = sorted(rs.choice(33, 20, replace=False).tolist())
    w3 = sorted(rs.choice(257, 201, replace=False).tolist())
    w3b = [w3[k] for k in rs.permutation(201)[:150]]
    return [
        ([], [[0], [], list(range(33)), list(range(257)), [0, 1]]),
        ([], [[0], [], w2, w3, [1]]),                                                    # survivors; begins unchanged
        ([], [[0], [], w2[:10] + [w2[3], 1000, w2[3], w2[0]] + w2[12:], w3b, [1, 0]]),   # duplicates, a new id; a shuffled world; 0 is back: zeros
        ([3], [[0], [], [w2[3], w2[0], 1000, 5], list(range(180)), [0, 1]]),             # the duplicated ids read back; world 3 was reset
    ]


CALLS = calls()


def packed_inputs(call, ids_by_world, seed=300):
    """(view, feature, ids int32 [N], table) of one call: the worlds' rows at BEGIN, random gap rows with NaN in every third, gap ids 0..4"""
    view, featv = H.make_policy_inputs(VS, FEAT, N, seed + call)
    ids = (np.arange(N) % 5).astype(np.int32)
    free = np.ones(N, dtype=bool)
    for b, w in zip(BEGIN, ids_by_world):
        ids[b:b + len(w)] = w
        free[b:b + len(w)] = False
    gaps = np.nonzero(free)[0]
    view[gaps[::3], 1, 2, 0] = NAN
    seg = np.asarray([[b, len(w)] for b, w in zip(BEGIN, ids_by_world)], dtype=np.int32)
    return view, featv, ids, seg


def run(lg, pol, kind, view, featv, ids, segments=None):
    """one call -> [actions, Q, h'] as NumPy; segments=None is the plain call (no keyword: the parent commit's call; no row: the table is
    emptied as drqn.py does for n == 0)"""
    import torch
    if len(ids) == 0:
        pol.load_states({})
        return [np.zeros(0, np.int32), np.zeros((0, A), np.float32), np.zeros((0, S), np.float32)]
    vin = H.cells_of(view) if kind == "cells" else view
    kw = {} if segments is None else {"segments": segments}
    actions, q = pol.infer(vin.to(lg.dev).contiguous(), featv.to(lg.dev).contiguous(), torch.as_tensor(np.asarray(ids, np.int32)).to(lg.dev),
                           want_q=True, **kw)
    lg.sync()
    return [actions.cpu().numpy(), q.cpu().numpy(), pol._states.cpu().numpy()]


def same_bits(got, want, tag):
    for g, w, what in zip(got, want, ("actions", "Q", "h'")):
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=True), (tag, what, np.argwhere(~((g == w) | ((g != g) & (w != w))))[:4].tolist())


def make_net(lg, seed=41):
    return H.make_rnet(VS, FEAT, A, True, seed, lg.dev)


PLAYED = {}


def played(kind, lg):
    """the sequence played once per kind and leg, shared by the tests and left unchanged: per call (view, feature, ids, table, the
    segmented call's outputs, the outputs of every world's own plain policy on its rows alone), and the net"""
    key = (kind, lg.name)
    if key not in PLAYED:
        net = make_net(lg)
        pol = lg.policy(net, VS, FEAT, A, chunk=96)
        worlds = [lg.policy(net, VS, FEAT, A) for _ in BEGIN]
        rounds = []
        for call, (forget, ids_by_world) in enumerate(CALLS):
            view, featv, ids, seg = packed_inputs(call, ids_by_world)
            if forget:
                pol.forget_segments(forget)
                for s in forget:
                    worlds[s].load_states({})
            out = run(lg, pol, kind, view, featv, ids, seg)
            plain = [run(lg, worlds[s], kind, view[b:b + len(w)], featv[b:b + len(w)], w) for s, (b, w) in enumerate(zip(BEGIN, ids_by_world))]
            rounds.append((view, featv, ids, seg, out, plain))
        PLAYED[key] = (net, rounds, pol)
    return PLAYED[key]


# ---------------------------------------------------------------------------------------------------- 1. the plain call per world
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", LEGS)
def test_segments_equal_the_plain_call_per_world(lg, kind):
    """over the four calls of CALLS, actions, Q and h' of every segment's rows equal the plain infer of that world's own policy object on
    view[b:b+c], feat[b:b+c] and the world's ids; the forgotten world starts from zeros.  The planted defects this catches are listed in
    the module's docstring."""
    lg = the_leg(kind, lg)
    net, rounds, pol = played(kind, lg)
    for call, (view, featv, ids, seg, out, plain) in enumerate(rounds):
        assert out[0].dtype == np.int32 and out[1].shape == (N, A) and out[2].shape == (N, S)
        assert ((out[0] >= 0) & (out[0] < A)).all()
        for s, (b, c) in enumerate(seg.tolist()):
            same_bits([o[b:b + c] for o in out], plain[s], "%s %s call %d world %d" % (lg.name, kind, call, s))
    # the states mattered: world 3's rows of call 1 differ from a start from zeros, and call 3's (forgotten) are a start from zeros
    view, featv, ids, seg, out, plain = rounds[3]
    b, c = seg[3].tolist()
    fresh = lg.policy(net, VS, FEAT, A)
    same_bits([o[b:b + c] for o in out], run(lg, fresh, kind, view[b:b + c], featv[b:b + c], ids[b:b + c]), "forgotten world")
    view, featv, ids, seg, out, plain = rounds[1]
    b, c = seg[3].tolist()
    fresh = lg.policy(net, VS, FEAT, A)
    assert not np.array_equal(out[2][b:b + c], run(lg, fresh, kind, view[b:b + c], featv[b:b + c], ids[b:b + c])[2])


def test_states_dict_has_the_tuple_keys_of_the_living():
    """after the last call of the sequence (emulator, float32): {(world, id): state} in call order, a duplicated id once, no gap row"""
    lg = the_leg("f32", "emu")
    net, rounds, pol = played("f32", lg)
    want = []
    for s, w in enumerate(CALLS[-1][1]):
        want += [(s, i) for i in w]
    got = pol.states_dict()
    assert list(got.keys()) == list(dict.fromkeys(want))
    h2 = rounds[-1][4][2]
    assert np.array_equal(got[(3, 7)].numpy(), h2[BEGIN[3] + 7]) and np.array_equal(got[(4, 1)].numpy(), h2[BEGIN[4] + 1])


# ---------------------------------------------------------------------------------------------------- 2. float64, once per leg and kind
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", LEGS)
def test_a_segmented_call_against_float64(lg, kind):
    """call 2 of the sequence (duplicates, a new id, collisions across worlds, gap rows) through test_drqn_policy.py's float64 restatement
    and bounds (the derived bound and the working bound of its step_and_check) or test_drqn_bf16_policy.py's rounding reference and bound,
    fed the kernels' own states of call 1 looked up per (world, id); gap rows start from zeros, NaN rows are NaN"""
    import torch
    lg = the_leg(kind, lg)
    net, rounds, _ = played(kind, lg)
    view, featv, ids, seg, (actions, q, h2), _ = rounds[2]
    pview, _, pids, pseg, pout, _ = rounds[1]
    table = {}
    for s, (b, c) in enumerate(pseg.tolist()):
        for r in range(b, b + c):
            table[(s, int(pids[r]))] = pout[2][r]
    h_prev = np.zeros((N, S), np.float32)
    found = 0
    for s, (b, c) in enumerate(seg.tolist()):
        for r in range(b, b + c):
            if (s, int(ids[r])) in table:
                h_prev[r] = table[(s, int(ids[r]))]
                found += 1
    assert found >= 150
    tag = "%s %s segmented" % (lg.name, kind)
    if kind != "f32":
        B16.check_against_ref(tag, net, view, featv, h_prev, torch.from_numpy(actions), q.astype(np.float64), h2.astype(np.float64), A)
        return
    P = H.net_params(net)
    v64, f64 = view.double().numpy(), featv.double().numpy()
    q64, h64 = F32.np_drqn_step(P, v64, f64, h_prev, True)
    assert np.array_equal(actions, torch.from_numpy(q).argmax(dim=1).numpy())
    eh, eq = F32.error_bounds(P, v64, f64, h_prev, h64, VS, FEAT, A, True)
    for got, want, bound, what, tight_scale in ((h2, h64, eh, "h'", 1.0), (q, q64, eq, "Q", None)):
        assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.array_equal(np.isnan(got), np.isnan(want)), (tag, what)
        ok = np.isfinite(want)
        assert ok.any() and not ok.all()
        d = np.abs(got[ok] - want[ok])
        scale = tight_scale if tight_scale is not None else float(np.abs(want[ok]).max())
        ratio, tight = float((d / bound[ok]).max()), float((d / (1e-5 * scale + 1e-7)).max())
        print("%s: worst %s %.3g of the bound, %.3g of the working bound" % (tag, what, ratio, tight))
        assert ratio <= 1.0 and tight <= 1.0, (tag, what, ratio, tight)


# ---------------------------------------------------------------------------------------------------- 3. chunking
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", LEGS)
def test_chunks_do_not_change_a_bit(lg, kind):
    """calls 0 .. 2 with pol.chunk = 64 and unchunked: the bits of the sequence's policy (chunk = 96)"""
    lg = the_leg(kind, lg)
    net, rounds, _ = played(kind, lg)
    for chunk in (64, 131072):
        pol = lg.policy(net, VS, FEAT, A)
        pol.chunk = chunk
        for call in range(3):
            view, featv, ids, seg, out, _ = rounds[call]
            same_bits(run(lg, pol, kind, view, featv, ids, seg), out, "%s %s chunk %d call %d" % (lg.name, kind, chunk, call))


# ---------------------------------------------------------------------------------------------------- 4. more segments than one look-up takes
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", [pytest.param("gpu", marks=pytest.mark.gpu)])
def test_more_segments_than_one_lookup_takes(lg, kind):
    """300 segments of 1 .. 3 rows, two calls (ids arange(count), then reversed with every fifth world's first agent replaced by a new
    one): every segment equals its own world's plain policy -- also behind the cut at segment 256, whose look-up adds 256 to the key's
    segment.  (The emulator leg would run 600 plain calls of a full MFMA tile each: minutes.)"""
    lg = the_leg(kind, lg)
    rs = np.random.RandomState(9)
    counts = rs.randint(1, 4, size=300).tolist()
    seg, n = lay_out(counts, first=0, stale={7: 1, 255: 2, 256: 1})
    assert len(seg) > MAX_SEGMENTS
    net = make_net(lg, 43)
    pol = lg.policy(net, VS, FEAT, A)
    worlds = [lg.policy(net, VS, FEAT, A) for _ in counts]
    for call in range(2):
        view, featv = H.make_policy_inputs(VS, FEAT, n, 500 + call)
        ids = (np.arange(n) % 3).astype(np.int32)
        for s, (b, c) in enumerate(seg.tolist()):
            w = list(range(c)) if call == 0 else list(range(c))[::-1]
            if call == 1 and s % 5 == 0:
                w[0] = 77
            ids[b:b + c] = w
        out = run(lg, pol, kind, view, featv, ids, seg)
        for s, (b, c) in enumerate(seg.tolist()):
            same_bits([o[b:b + c] for o in out], run(lg, worlds[s], kind, view[b:b + c], featv[b:b + c], ids[b:b + c]), "call %d world %d" % (call, s))
    keys = pol._keys.cpu().numpy()
    b, c = seg[299].tolist()
    assert (keys[b:b + c] >> 32 == 299).all() and (keys[seg[256][0]] >> 32) == 256 and (keys == NO_KEY).sum() == n - sum(counts)


# ---------------------------------------------------------------------------------------------------- 5. hand-overs
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", LEGS)
def test_tables_change_hands(lg, kind):
    """plain -> segmented: segment 0 inherits the plain table, segment 1 with the same ids starts from zeros; segmented -> plain: segment
    0's entries survive, the others' ids start from zeros; states_dict / load_states round trip with tuple keys"""
    lg = the_leg(kind, lg)
    net = make_net(lg, 47)
    n = 24
    ids = np.asarray([3, 1, 4, 1, 5, 9, 2, 6, -5, 35], np.int32)           # (a duplicate and a negative id)
    seg = np.asarray([[0, 10], [12, 10]], dtype=np.int32)
    both = np.zeros(n, np.int32)
    both[0:10], both[12:22] = ids, ids
    inputs = [H.make_policy_inputs(VS, FEAT, n, 600 + k) for k in range(4)]
    pol, twin, fresh = [lg.policy(net, VS, FEAT, A) for _ in range(3)]
    # plain, plain twin alike
    view, featv = inputs[0]
    same_bits(run(lg, pol, kind, view[:10], featv[:10], ids), run(lg, twin, kind, view[:10], featv[:10], ids), "first")
    assert list(pol.states_dict().keys()) == [3, 1, 4, 5, 9, 2, 6, -5, 35]
    # -> segmented
    view, featv = inputs[1]
    out = run(lg, pol, kind, view, featv, both, seg)
    same_bits([o[0:10] for o in out], run(lg, twin, kind, view[0:10], featv[0:10], ids), "segment 0 inherits")
    same_bits([o[12:22] for o in out], run(lg, fresh, kind, view[12:22], featv[12:22], ids), "segment 1 is new")
    d = pol.states_dict()
    assert list(d.keys()) == [(0, int(i)) for i in [3, 1, 4, 5, 9, 2, 6, -5, 35]] + [(1, int(i)) for i in [3, 1, 4, 5, 9, 2, 6, -5, 35]]
    # the dict view and back: another policy continues with the same bits
    other = lg.policy(net, VS, FEAT, A)
    other.load_states(d)
    view, featv = inputs[2]
    out = run(lg, pol, kind, view, featv, both, seg)
    same_bits(run(lg, other, kind, view, featv, both, seg)[:2], out[:2], "round trip")
    same_bits([o[12:22] for o in out], run(lg, fresh, kind, view[12:22], featv[12:22], ids), "segment 1 carries on")
    run(lg, twin, kind, view[0:10], featv[0:10], ids)
    # int keys read as segment 0 beside tuple keys
    mixed = lg.policy(net, VS, FEAT, A)
    mixed.load_states({3: d[(0, 3)], (1, 3): d[(1, 3)]})
    assert list(mixed.states_dict().keys()) == [(0, 3), (1, 3)]
    # -> plain: ids of segment 0 carry on, 77 is new, and segment 1's states are gone
    view, featv = inputs[3]
    ids2 = np.asarray([35, -5, 77, 1], np.int32)
    same_bits(run(lg, pol, kind, view[:4], featv[:4], ids2), run(lg, twin, kind, view[:4], featv[:4], ids2), "back to plain")
    assert list(pol.states_dict().keys()) == [35, -5, 77, 1] and pol._sorted.dtype == __import__("torch").int32


@pytest.mark.parametrize("lg", LEGS)
def test_a_float32_table_goes_to_the_bf16_policy(lg):
    """two segmented calls on HipDrqnPolicyF32, its (segment, id) table handed to a bf16 policy of the same weights: the bf16 policy's
    segmented call equals, per world, a plain bf16 policy loaded with that world's states under their ids"""
    f32, b16 = F32.leg(lg), B16.leg(lg)
    net = make_net(f32, 49)
    seg = np.asarray([[0, 5], [8, 6]], dtype=np.int32)
    ids = np.asarray([0, 1, 2, 3, 4, 9, 9, 9, 0, 1, 2, 3, 4, 5, 7, 7], np.int32)
    p32, p16 = f32.policy(net, VS, FEAT, A), b16.policy(net, VS, FEAT, A)
    for call in range(2):
        view, featv = H.make_policy_inputs(VS, FEAT, 16, 700 + call)
        run(f32, p32, "f32", view, featv, ids, seg)
    handed = p32.states_dict()
    assert set(handed.keys()) == {(0, i) for i in range(5)} | {(1, i) for i in range(6)}
    p16.load_states(handed)
    view, featv = H.make_policy_inputs(VS, FEAT, 16, 702)
    out = run(b16, p16, "bf16", view, featv, ids, seg)
    for s, (b, c) in enumerate(seg.tolist()):
        own = b16.policy(net, VS, FEAT, A)
        own.load_states({i: v for (w, i), v in handed.items() if w == s})
        same_bits([o[b:b + c] for o in out], run(b16, own, "bf16", view[b:b + c], featv[b:b + c], ids[b:b + c]), "world %d" % s)
    assert np.abs(out[2][:5]).max() > 0.05


# ---------------------------------------------------------------------------------------------------- 6. the C entries
ENTRIES = {"f32": ("policy_drqn_lookup_seg_f32", "policy_drqn_infer_f32_rows", "policy_drqn_f32_workspace_bytes"),
           "bf16": ("policy_drqn_lookup_seg", "policy_drqn_infer_rows", "policy_drqn_workspace_bytes"),
           "cells": ("policy_drqn_lookup_seg", "policy_drqn_infer_bf16_rows", "policy_drqn_workspace_bytes")}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", LEGS)
def test_refused_calls_write_nothing_and_valid_ones_stay_inside(lg, kind):
    """the look-up and the *_rows entry on sentinel-filled from_row, keys, new_states, actions and q with guards around their n rows:
    an overlapping or descending table, a segment past n, n_seg 257, a negative seg_first and a misaligned new_states return non-zero
    and leave every word; a valid call writes its n rows and nothing else, and equals the binding's call"""
    import torch
    lg = the_leg(kind, lg)
    lookup, rows_entry, bytes_entry = (getattr(lg.lib, e) for e in ENTRIES[kind])
    net = make_net(lg, 51)
    pol = lg.policy(net, VS, FEAT, A)
    n, PAD = 37, 64
    view, featv = H.make_policy_inputs(VS, FEAT, n, 800)
    ids_np = (np.arange(n) % 11).astype(np.int32)
    seg = np.asarray([[0, 9], [12, 20]], dtype=np.int32)
    first = run(lg, pol, kind, view, featv, ids_np, seg)                   # a table of n rows (two of them share a key)
    table = [t.clone() for t in (pol._sorted, pol._rows, pol._states)]
    vin = (H.cells_of(view) if kind == "cells" else view).to(lg.dev).contiguous()
    fin, ids = featv.to(lg.dev).contiguous(), torch.as_tensor(ids_np).to(lg.dev)
    from_row = torch.full((n + 2 * PAD,), -7, dtype=torch.int32, device=lg.dev)
    keys = torch.full((n + 2 * PAD,), -77, dtype=torch.int64, device=lg.dev)
    acts = torch.full((n + 2 * PAD,), -7, dtype=torch.int32, device=lg.dev)
    q = torch.full((n * A + 2 * PAD,), -77.0, device=lg.dev)
    st = torch.full((n * S + 2 * PAD,), -777.0, device=lg.dev)
    nb = ctypes.c_size_t(0)
    bytes_entry(ctypes.byref(pol.shape), n, ctypes.byref(nb))
    work = torch.full((nb.value + 2 * 4096,), 0x5A, dtype=torch.uint8, device=lg.dev)
    arr = lambda v: (ctypes.c_int32 * max(len(v), 1))(*v)

    def look(begin, count, n_seg, seg_first=0, rows=n):
        return lookup(ids.data_ptr(), rows, arr(begin), arr(count), n_seg, seg_first, pol._sorted.data_ptr(), pol._rows.data_ptr(), n,
                      from_row[PAD:].data_ptr(), keys[PAD:].data_ptr(), None)

    def untouched():
        lg.sync()
        return all(bool((buf == fill).all()) for buf, fill in ((from_row, -7), (keys, -77), (acts, -7), (q, -77.0), (st, -777.0)))

    assert look([0, 8], [9, 20], 2) != 0                                   # overlapping
    assert look([12, 0], [20, 9], 2) != 0                                  # descending
    assert look([0, 12], [9, 26], 2) != 0                                  # past n
    assert look([0], [-1], 1) != 0
    assert look(list(range(257)), [0] * 257, 257, rows=300) != 0           # n_seg 257
    assert look([0], [9], 1, seg_first=-1) != 0
    assert look([0], [9], 1, seg_first=0x7FFFFFFF - 256) != 0
    assert untouched()
    step = lambda new_states, states=pol._states.data_ptr(), fr=from_row[PAD:].data_ptr(): rows_entry(
        ctypes.byref(pol.shape), ctypes.byref(pol._w), vin.data_ptr(), fin.data_ptr(), n, fr, states, new_states, work[4096:].data_ptr(),
        acts[PAD:].data_ptr(), q[PAD:].data_ptr(), None)
    assert step(st[PAD + 1:].data_ptr()) != 0                              # misaligned new_states
    assert step(st[PAD:].data_ptr(), states=pol._states.data_ptr() + 4) != 0
    assert step(st[PAD:].data_ptr(), fr=None) != 0
    assert step(None) != 0
    bad = type(pol.shape)(4, 4, VS[2], FEAT, A)                            # (a view too small for the two convolutions)
    assert rows_entry(ctypes.byref(bad), ctypes.byref(pol._w), vin.data_ptr(), fin.data_ptr(), n, from_row[PAD:].data_ptr(), None,
                      st[PAD:].data_ptr(), work[4096:].data_ptr(), acts[PAD:].data_ptr(), None, None) != 0
    assert untouched() and bool((work == 0x5A).all())
    # a valid pair of calls: the second call of the binding on the same inputs
    assert look(seg[:, 0].tolist(), seg[:, 1].tolist(), 2) == 0 and step(st[PAD:].data_ptr()) == 0
    lg.sync()
    for buf, fill, m in ((from_row, -7, n), (keys, -77, n), (acts, -7, n), (q, -77.0, n * A), (st, -777.0, n * S)):
        assert bool((buf[:PAD] == fill).all()) and bool((buf[PAD + m:] == fill).all()), fill
    assert bool((work[:4096] == 0x5A).all()) and bool((work[4096 + nb.value:] == 0x5A).all())
    for a, b in zip(table, (pol._sorted, pol._rows, pol._states)):
        assert torch.equal(a, b)
    fr, ky = from_row[PAD:PAD + n].cpu().numpy(), keys[PAD:PAD + n].cpu().numpy()
    inside = np.zeros(n, dtype=bool)
    for s, (b, c) in enumerate(seg.tolist()):
        inside[b:b + c] = True
        assert np.array_equal(ky[b:b + c], (s << 32) | ids_np[b:b + c].astype(np.int64))
        # the LAST row of the previous call with that (segment, id)
        want = [max(r for r in range(b, b + c) if ids_np[r] == ids_np[k]) for k in range(b, b + c)]
        assert fr[b:b + c].tolist() == want
    assert (fr[~inside] == -1).all() and (ky[~inside] == NO_KEY).all()
    second = run(lg, pol, kind, view, featv, ids_np, seg)
    same_bits([acts[PAD:PAD + n].cpu().numpy(), q[PAD:PAD + n * A].cpu().numpy().reshape(n, A), st[PAD:PAD + n * S].cpu().numpy().reshape(n, S)],
              second, "the binding's call")
    assert not np.array_equal(first[2][:9], second[2][:9])
    # the empty table: states NULL, from_row given and not read
    acts.fill_(-7)
    assert step(st[PAD:].data_ptr(), states=None) == 0
    lg.sync()
    assert np.array_equal(acts[PAD:PAD + n].cpu().numpy(), first[0])


# ---------------------------------------------------------------------------------------------------- 7. validation
@pytest.mark.parametrize("table,word", [([[0, 4], [3, 2]], "segment 1"), ([[0, 4], [8, 2], [6, 1]], "segment 2"), ([[0, 4], [8, 9]], "segment 1"),
                                        ([[-1, 2]], "segment 0"), ([[0, 2], [4, -3]], "segment 1")])
def test_malformed_tables_are_named(table, word):
    """every malformed table raises ValueError naming the offending segment, before anything is launched; the table stays as it was"""
    import torch
    lg = the_leg("f32", "emu")
    pol = lg.policy(make_net(lg, 53), VS, FEAT, A)
    view, featv = H.make_policy_inputs(VS, FEAT, 16, 900)
    before = pol.states_dict()
    with pytest.raises(ValueError, match=word):
        pol.infer(view, featv, torch.zeros(16, dtype=torch.int32), segments=np.asarray(table, dtype=np.int32))
    with pytest.raises(ValueError):
        pol.infer(view, featv, torch.zeros(16, dtype=torch.int32), segments=np.zeros((2, 3), dtype=np.int32))
    assert pol.states_dict() == before
