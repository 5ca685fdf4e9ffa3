"""The segmented A2C acting step (include/magent_policy.h: policy_a2c_infer_f32_seg, policy_a2c_infer_seg, policy_a2c_infer_bf16_seg; the
bindings' and AdvantageActorCritic.infer_action's `segments=`; EnvBatch.packed_segments): ONE call over a packed buffer of several
environments' rows, every CommNet mean inside the agent's own segment.

The main criterion needs no tolerance: the outputs of a segment's rows are, bit for bit, those of the PLAIN entry called on that segment's
rows of view, feature and u alone -- the column sums of a segment are taken over blocks of 256 agents counted from the segment's own first
row.  The plain entries are checked against float64 / the rounding reference by test_a2c_policy.py and test_a2c_bf16_policy.py; one
segmented call per leg goes through the same restatements and bounds here (imported, not copied), segment by segment.

Two legs (helpers.policy_legs, the modules' own): `emu` runs the kernels compiled as plain C++ against tests/hipemu on CPU tensors, `gpu`
(marked) the product library.  Three kinds: the float32 kernels, the bf16 kernels on float32 views and on the engine's bf16 cells.

Shapes (test 1): network (5, 5, 3) / 7 features / 9 actions with CommNet.  LAYOUTS["a"]: counts [1, 0, 33, 257, 2] at rows 4, 8, 8, 52,
312 of 322 -- an agent alone, an empty world, a segment across a 32-agent tile, one across the 256-agent workgroup at row 256 whose sum
blocks start at row 52 (no multiple of 256: [52, 308), [308, 309)), 11 stale rows behind the third segment, 6 rows behind the last;
LAYOUTS["b"]: [31, 300, 0, 1].  Every begin is a multiple of 4 and the first is not 0.  The gap rows hold random values, like stale rows.

Planted defects that the emulator leg of test_segments_equal_the_plain_call_per_segment catches, each by a bit difference in layout "a":
the sums taken over the whole call; the divisor taken from the call's n; the sum blocks counted from row 0 of the call instead of the
segment's first row (segment 3 would be cut at row 256, not 308); a gap row added into its neighbour's sum."""
import ctypes

import numpy as np
import pytest

import helpers as H
import test_a2c_bf16_policy as B16
import test_a2c_policy as F32

NAN = float("nan")
LEGS = F32.LEGS
KINDS = ["f32", "bf16", "cells"]          # the float32 kernels; the bf16 kernels on float32 views; on bf16 cells
VS, FEAT, A = (5, 5, 3), 7, 9
MAX_SEGMENTS = 256                        # include/magent_policy.h: POLICY_A2C_MAX_SEGMENTS


def the_leg(kind, name):
    return (F32.leg if kind == "f32" else B16.leg)(name)


def lay_out(counts, first=4, stale=None, tail=6):
    """segments of `counts` rows, each begin a multiple of 4, `stale[s]` further rows behind segment s, `tail` rows behind the last ->
    (int32 table [n_seg][2], n)"""
    stale = stale or {}
    seg, at = [], first
    for s, c in enumerate(counts):
        seg.append((at, c))
        at += (c + 3) // 4 * 4 + 4 * stale.get(s, 0)
    return np.asarray(seg, dtype=np.int32).reshape(-1, 2), at + tail


LAYOUTS = {
    "a": lay_out([1, 0, 33, 257, 2], stale={2: 2}),
    "b": lay_out([31, 300, 0, 1], stale={0: 2}, tail=5),
    "big": lay_out([1500, 5, 0, 40, 1, 2, 7, 3, 64, 9, 2, 31], stale={0: 1, 3: 3}),        # (GPU only: past five sum blocks, 12 segments)
}
assert LAYOUTS["a"][0].tolist() == [[4, 1], [8, 0], [8, 33], [52, 257], [312, 2]] and LAYOUTS["a"][1] == 322


def make(kind, lg, n, seed=70, comm=True):
    """(net on the CPU, policy on the leg's device, view, feature, u) of n rows"""
    net = F32.make_net(VS, FEAT, A, comm, seed)
    view, featv = H.make_policy_inputs(VS, FEAT, n, seed + 1)
    u = np.random.RandomState(seed + 2).rand(n).astype(np.float32)
    return net, lg.policy(B16.cpu_net(net).to(lg.dev), VS, FEAT, A), view, featv, u


def run(lg, pol, kind, view, featv, u, segments=None):
    """one call -> [actions, p, value] as NumPy; segments=None is the plain call (no keyword: the parent commit's call)"""
    import torch
    vin = H.cells_of(view) if kind == "cells" else view
    kw = {} if segments is None else {"segments": segments}
    out = pol.infer(vin.to(lg.dev).contiguous(), featv.to(lg.dev).contiguous(), u=torch.as_tensor(u).to(lg.dev), want_policy=True,
                    want_value=True, **kw)
    lg.sync()
    return [t.cpu().numpy() for t in out]


PACKED = {}


def packed(kind, lg, layout):
    """(net, policy, view, feature, u, table, the segmented call's [actions, p, value]) of LAYOUTS[layout]: computed once per kind and leg,
    shared by the tests and left unchanged"""
    key = (kind, lg.name, layout)
    if key not in PACKED:
        seg, n = LAYOUTS[layout]
        net, pol, view, featv, u = make(kind, lg, n)
        PACKED[key] = (net, pol, view, featv, u, seg, run(lg, pol, kind, view, featv, u, seg))
    return PACKED[key]


def same_bits(got, want, tag):
    for g, w, what in zip(got, want, ("actions", "p", "value")):
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=True), (tag, what, np.argwhere(~((g == w) | ((g != g) & (w != w))))[:4].tolist())


def in_no_segment(seg, n):
    free = np.ones(n, dtype=bool)
    for b, c in seg.tolist():
        free[b:b + c] = False
    return np.nonzero(free)[0]


def check_per_segment(lg, pol, kind, view, featv, u, seg, out, tag, loners=3):
    """`out` of the segmented call against the plain call on every segment's rows, and on `loners` of the rows in no segment, one row each"""
    n = view.shape[0]
    for s, (b, c) in enumerate(seg.tolist()):
        if c > 0:
            same_bits([o[b:b + c] for o in out], run(lg, pol, kind, view[b:b + c], featv[b:b + c], u[b:b + c]), "%s segment %d" % (tag, s))
    free = in_no_segment(seg, n)
    assert ((out[0][free] >= 0) & (out[0][free] < A)).all()
    for r in free[np.linspace(0, len(free) - 1, min(loners, len(free))).astype(int)] if len(free) else []:
        same_bits([o[r:r + 1] for o in out], run(lg, pol, kind, view[r:r + 1], featv[r:r + 1], u[r:r + 1]), "%s row %d alone" % (tag, r))


# ---------------------------------------------------------------------------------------------------- 1. the plain call per segment
SHAPES = [("emu", "a"), ("emu", "b")] + [pytest.param("gpu", k, marks=pytest.mark.gpu) for k in ("a", "b", "big")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg,layout", SHAPES)
def test_segments_equal_the_plain_call_per_segment(lg, layout, kind):
    """actions, probabilities and values of every segment's rows equal the plain infer on view[b:b+c], feat[b:b+c], u[b:b+c]; rows in no
    segment equal a plain call of that one row.  The planted defects this catches are listed in the module's docstring."""
    lg = the_leg(kind, lg)
    net, pol, view, featv, u, seg, out = packed(kind, lg, layout)
    n = LAYOUTS[layout][1]
    assert out[0].dtype == np.int32 and out[1].shape == (n, A) and out[2].shape == (n,)
    check_per_segment(lg, pol, kind, view, featv, u, seg, out, "%s %s %s" % (lg.name, kind, layout), loners=4)
    if lg.name == "gpu":      # the means stayed inside the segments: the whole buffer as one plain call gives other bits in every segment of two or more
        whole = run(lg, pol, kind, view, featv, u)
        for b, c in seg.tolist():
            assert c < 2 or not np.array_equal(out[1][b:b + c], whole[1][b:b + c])


# ---------------------------------------------------------------------------------------------------- 2. float64, once per leg
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", LEGS)
def test_a_segmented_call_against_float64_per_segment(lg, kind):
    """one segmented call through the restatements and bounds of test_a2c_policy.py (float64, derived and working bound) and
    test_a2c_bf16_policy.py (the rounding reference, four times its reordering spread), applied per segment and to two rows alone"""
    lg = the_leg(kind, lg)
    net, pol, view, featv, u, seg, (actions, p, value) = packed(kind, lg, "a")
    n = LAYOUTS["a"][1]
    assert np.array_equal(actions, F32.np_draw(p, u))
    free = in_no_segment(seg, n)
    spans = [(b, c) for b, c in seg.tolist() if c > 0] + [(int(free[0]), 1), (int(free[-1]), 1)]
    for b, c in spans:
        tag = "%s %s rows %d..%d" % (lg.name, kind, b, b + c - 1)
        if kind == "f32":
            F32.check_against_float64(H.net_params(net), view[b:b + c], featv[b:b + c], True, p[b:b + c], value[b:b + c], tag)
        else:
            B16.check_against_ref(tag, net, view[b:b + c], featv[b:b + c], True, p[b:b + c], value[b:b + c])


# ---------------------------------------------------------------------------------------------------- 3. isolation
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", LEGS)
def test_a_nan_stays_in_its_segment(lg, kind):
    """a NaN planted in a gap row and one in segment 2: every other segment and every other gap row keeps its bits; the poisoned segment is
    all NaN with action A - 1, and so is the poisoned gap row"""
    lg = the_leg(kind, lg)
    net, pol, view, featv, u, seg, clean = packed(kind, lg, "a")
    n, view = LAYOUTS["a"][1], view.clone()
    assert np.isfinite(clean[1]).all() and np.isfinite(clean[2]).all()
    b2, c2 = seg[2].tolist()
    gap = b2 + c2 + 5                                       # (a stale row behind segment 2, in front of segment 3)
    assert gap in in_no_segment(seg, n)
    view[gap, 1, 2, 0] = NAN
    view[b2 + 7, 2, 2, 1] = NAN
    actions, p, value = run(lg, pol, kind, view, featv, u, seg)
    hit = np.zeros(n, dtype=bool)
    hit[b2:b2 + c2] = True
    hit[gap] = True
    assert np.isnan(p[hit]).all() and np.isnan(value[hit]).all() and (actions[hit] == A - 1).all()
    same_bits([actions[~hit], p[~hit], value[~hit]], [o[~hit] for o in clean], "%s %s" % (lg.name, kind))


# ---------------------------------------------------------------------------------------------------- 4. degenerate tables
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", LEGS)
def test_degenerate_tables(lg, kind):
    """[(0, n)] is the plain call; no segment at all is n calls of one row; without CommNet any valid table is the plain call"""
    lg = the_leg(kind, lg)
    n = 70 if lg.name == "emu" else 300
    net, pol, view, featv, u = make(kind, lg, n, seed=80)
    plain = run(lg, pol, kind, view, featv, u)
    same_bits(run(lg, pol, kind, view, featv, u, np.asarray([[0, n]], dtype=np.int32)), plain, "one segment")
    for empty in (np.zeros((0, 2), dtype=np.int32), []):
        out = run(lg, pol, kind, view, featv, u, empty)
        for r in (0, 1, 31, 32, n - 1):
            same_bits([o[r:r + 1] for o in out], run(lg, pol, kind, view[r:r + 1], featv[r:r + 1], u[r:r + 1]), "no segment, row %d" % r)
    net, pol, view, featv, u = make(kind, lg, n, seed=81, comm=False)
    plain = run(lg, pol, kind, view, featv, u)
    for table in ([[0, n]], [[4, 9], [16, 0], [16, n - 20]], []):
        same_bits(run(lg, pol, kind, view, featv, u, np.asarray(table, dtype=np.int32).reshape(-1, 2)), plain, "plain net, %s" % table)
    with pytest.raises(ValueError):          # (validated all the same)
        run(lg, pol, kind, view, featv, u, np.asarray([[8, 8], [4, 2]], dtype=np.int32))


# ---------------------------------------------------------------------------------------------------- 5, 6. the C entries' buffers
class CCall(object):
    """the segmented C entry of `kind` on sentinel-filled, guarded buffers: actions, policy, value and a workspace of exactly
    workspace_bytes_seg(n, comm, n_seg) bytes between two 4096-byte guards"""
    PAD, FILLS = 333, (-7, -77.0, -777.0, 0x5A)

    def __init__(self, kind, lg, n, comm=True):
        import torch
        self.kind, self.lg, self.n = kind, lg, n
        self.net, self.pol, view, featv, u = make(kind, lg, n, seed=90, comm=comm)
        self.pol.pack()
        self.host = (view, featv, u)
        self.view = (H.cells_of(view) if kind == "cells" else view).to(lg.dev).contiguous()
        self.feat, self.u = featv.to(lg.dev).contiguous(), torch.as_tensor(u).to(lg.dev)
        self.keep = [t.clone() for t in (self.view, self.feat, self.u)]
        self.entry = getattr(lg.lib, {"f32": "policy_a2c_infer_f32_seg", "bf16": "policy_a2c_infer_seg", "cells": "policy_a2c_infer_bf16_seg"}[kind])
        self.bytes_fn = getattr(lg.lib, "policy_a2c_f32_workspace_bytes_seg" if kind == "f32" else "policy_a2c_workspace_bytes_seg")
        self.comm = comm

    def buffers(self, n_seg):
        import torch
        nb = ctypes.c_size_t(0)
        assert self.bytes_fn(ctypes.byref(self.pol.shape), self.n, int(self.comm), n_seg, ctypes.byref(nb)) == 0
        n, dev, P = self.n, self.lg.dev, self.PAD
        self.nb = nb.value
        bufs = (torch.full((n + 2 * P,), -7, dtype=torch.int32, device=dev), torch.full((n * A + 2 * P,), -77.0, device=dev),
                torch.full((n + 2 * P,), -777.0, device=dev), torch.full((self.nb + 2 * 4096,), 0x5A, dtype=torch.uint8, device=dev))
        assert bufs[3][4096:].data_ptr() % 16 == 0
        return bufs

    def call(self, bufs, begin, count, n_seg=None):
        acts, pb, vb, work = bufs
        P = self.PAD
        n_seg = len(begin) if n_seg is None else n_seg
        cb, cc = (ctypes.c_int32 * max(len(begin), 1))(*begin), (ctypes.c_int32 * max(len(count), 1))(*count)
        rc = self.entry(ctypes.byref(self.pol.shape), ctypes.byref(self.pol._w), self.view.data_ptr(), self.feat.data_ptr(), self.n,
                        self.u.data_ptr(), work[4096:].data_ptr(), acts[P:].data_ptr(), pb[P:].data_ptr(), vb[P:].data_ptr(), None, cb, cc, n_seg)
        self.lg.sync()
        return rc

    def inputs_untouched(self):
        import torch
        as_int = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)
        return all(torch.equal(as_int(a), as_int(b)) for a, b in zip(self.keep, (self.view, self.feat, self.u)))


REFUSED = {"overlapping": [(0, 10), (8, 5)], "descending": [(20, 5), (0, 5)], "negative begin": [(-4, 2), (8, 3)], "negative count": [(0, -1), (8, 3)],
           "past n": [(0, 4), (38, 3)]}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", LEGS)
def test_refused_tables_write_nothing(lg, kind):
    """overlapping, descending, negative begin, negative count, begin + count > n, and one segment past the cap: the C entry returns 1 with
    every buffer still the sentinel, with and without CommNet; the binding raises ValueError for the first five"""
    lg = the_leg(kind, lg)
    n = 40
    for comm in (True, False):
        c = CCall(kind, lg, n, comm)
        cases = list(REFUSED.items()) + [("one past the cap", [(0, 0)] * (MAX_SEGMENTS + 1))]
        for name, table in cases:
            bufs = c.buffers(len(table))
            assert c.call(bufs, [b for b, _ in table], [k for _, k in table]) == 1, (name, comm)
            for buf, fill in zip(bufs, c.FILLS):
                assert bool((buf == fill).all()), (name, comm)
        bufs = c.buffers(0)
        assert c.call(bufs, [], [], n_seg=-1) == 1 and all(bool((buf == fill).all()) for buf, fill in zip(bufs, c.FILLS))
        assert c.inputs_untouched()
        view, featv, u = c.host
        for name, table in REFUSED.items():
            with pytest.raises(ValueError):
                run(lg, c.pol, kind, view, featv, u, np.asarray(table, dtype=np.int32))
        # the cap itself is taken
        bufs = c.buffers(MAX_SEGMENTS)
        assert c.call(bufs, [0] * MAX_SEGMENTS, [0] * MAX_SEGMENTS) == 0


LONG_SEGMENTS = {"emu": 270, "gpu": 700}          # (past the cap: two C calls, three on the GPU)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", LEGS)
def test_the_binding_splits_a_table_longer_than_the_cap(lg, kind):
    """segments of 0, 1 and 2 rows, every third with a gap row behind it: the binding cuts the table at segment boundaries into calls of at
    most 256 segments, and every segment still has the bits of the plain call on its rows (every segment on the GPU; on the emulator,
    where a call of one row costs what a call of 32 does, those around the cut and every twentieth elsewhere)"""
    lg = the_leg(kind, lg)
    counts = [(0, 1, 2, 2, 1)[s % 5] for s in range(LONG_SEGMENTS[lg.name])]
    seg, at = [], 1
    for s, c in enumerate(counts):
        seg.append((at, c))
        at += c + (s % 3 == 0)
    seg, n = np.asarray(seg, dtype=np.int32), at + 2
    net, pol, view, featv, u = make(kind, lg, n, seed=95)
    out = run(lg, pol, kind, view, featv, u, seg)
    picked = [s for s in range(len(seg)) if lg.name == "gpu" or s % 20 == 0 or abs(s - MAX_SEGMENTS) <= 2]
    check_per_segment(lg, pol, kind, view, featv, u, seg[picked], out, "%s %s long table" % (lg.name, kind), loners=0)
    free = in_no_segment(seg, n)
    assert ((out[0][free] >= 0) & (out[0][free] < A)).all()
    for r in (int(free[0]), int(free[len(free) // 2]), int(free[-1])):
        same_bits([o[r:r + 1] for o in out], run(lg, pol, kind, view[r:r + 1], featv[r:r + 1], u[r:r + 1]), "row %d alone" % r)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", LEGS)
def test_a_segmented_call_writes_nothing_outside_its_buffers(lg, kind):
    """actions, policy, value and a workspace of exactly workspace_bytes_seg bytes between sentinels: the guards are unchanged, every
    output element is written (pad and stale rows too), the inputs are untouched, and the binding returns the same bits"""
    import torch
    lg = the_leg(kind, lg)
    seg, n = lay_out([3, 0, 37, 261 if lg.name == "gpu" else 70, 1], stale={2: 1}, tail=3)
    c = CCall(kind, lg, n)
    bufs = c.buffers(len(seg))
    acts, pb, vb, work = bufs
    assert c.call(bufs, seg[:, 0].tolist(), seg[:, 1].tolist()) == 0
    P = c.PAD
    for buf, fill, m in ((acts, -7, n), (pb, -77.0, n * A), (vb, -777.0, n)):
        assert bool((buf[:P] == fill).all()) and bool((buf[P + m:] == fill).all())
        assert not bool((buf[P:P + m] == fill).any())
    assert bool((work[:4096] == 0x5A).all()) and bool((work[4096 + c.nb:] == 0x5A).all())
    assert c.inputs_untouched()
    view, featv, u = c.host
    a2, p2, v2 = run(lg, c.pol, kind, view, featv, u, seg)
    same_bits([a2, p2.reshape(-1), v2], [acts[P:P + n].cpu().numpy(), pb[P:P + n * A].cpu().numpy(), vb[P:P + n].cpu().numpy()], "binding")
    # the workspace grows by the sum rows, at most n / 256 + n_seg partial rows and the maps -- and by nothing without CommNet
    plain, none = ctypes.c_size_t(0), ctypes.c_size_t(0)
    plain_fn = getattr(lg.lib, "policy_a2c_f32_workspace_bytes" if kind == "f32" else "policy_a2c_workspace_bytes")
    assert plain_fn(ctypes.byref(c.pol.shape), n, 1, ctypes.byref(plain)) == 0
    rows = (len(seg) + n // 256 + len(seg)) * 512 * 4
    assert plain.value <= c.nb <= plain.value + rows + 4 * n + 24 * len(seg) + 8 * (n // 256) + 6 * 256
    assert c.bytes_fn(ctypes.byref(c.pol.shape), n, 0, len(seg), ctypes.byref(none)) == 0 and plain_fn(ctypes.byref(c.pol.shape), n, 0, ctypes.byref(plain)) == 0
    assert none.value == plain.value


# ---------------------------------------------------------------------------------------------------- 7. the PyTorch path means the same
def test_the_torch_path_gives_segments_the_same_meaning():
    """AdvantageActorCritic.infer_action(..., segments=) on CPU tensors and on NumPy arrays (the PyTorch path) with a policy head scaled until
    every row is one-hot: the actions of every segment are those of a call on that environment's rows alone, a row in no segment acts as a
    call of one row, and the whole buffer as one call acts differently somewhere (the head does depend on the means)"""
    import torch
    from magent_amd.builtin.torch_model import AdvantageActorCritic
    seg, n = lay_out([1, 0, 33, 40, 2], stale={2: 2})
    torch.manual_seed(7)
    model = AdvantageActorCritic(H.SpacesEnv(VS, FEAT, A), None, "seg", use_comm=True, device="cpu")
    assert model._hip is None
    with torch.no_grad():
        for p in model.net.parameters():
            p.mul_(3.0)
    F32._set_head(model.net, 1000.0, np.zeros(A))
    view, featv = H.make_policy_inputs(VS, FEAT, n, 71)
    with torch.no_grad():
        assert float(model.net(view, featv)[0].max(dim=1).values.min()) > 1 - 1e-6          # one-hot rows
    for as_numpy in (False, True):
        obs = lambda sl: (view[sl].numpy(), featv[sl].numpy()) if as_numpy else (view[sl], featv[sl])
        got = np.asarray(model.infer_action(obs(slice(0, n)), None, segments=seg))
        assert got.shape == (n,) and got.dtype == np.int32
        for b, c in seg.tolist():
            if c > 0:
                assert np.array_equal(got[b:b + c], np.asarray(model.infer_action(obs(slice(b, b + c)), None))), (b, c)
        for r in in_no_segment(seg, n):
            assert got[r] == np.asarray(model.infer_action(obs(slice(r, r + 1)), None))[0], r
        assert not np.array_equal(got, np.asarray(model.infer_action(obs(slice(0, n)), None)))
    with pytest.raises(ValueError):
        model.infer_action((view, featv), None, segments=np.asarray([[8, 8], [4, 2]]))


def test_packed_segments_is_the_documented_arithmetic():
    """EnvBatch.packed_segments on hand-picked counts: begin from the offsets the buffers were laid out with, count from the agents living
    now.  No library, no device."""
    import magent_amd

    class FakeEnv(object):
        game, group_handles = None, [0, 1]
    batch = magent_amd.EnvBatch.__new__(magent_amd.EnvBatch)
    batch.envs, batch.n_group = [FakeEnv() for _ in range(3)], 2
    off, tot = batch.packed_offsets(np.array([[5, 3], [1, 0], [4, 9]]))
    tables = batch.packed_segments(off, np.array([[4, 3], [0, 0], [4, 7]]))
    assert len(tables) == 2 and all(t.dtype == np.int32 and t.shape == (3, 2) for t in tables)
    assert tables[0].tolist() == [[0, 4], [8, 0], [12, 4]] and tables[1].tolist() == [[0, 3], [4, 0], [4, 7]]
    from magent_amd.builtin.torch_model.hip_policy import check_segments
    for g in range(2):
        check_segments(tables[g], int(tot[g]))


# ---------------------------------------------------------------------------------------------------- 8. the model over an EnvBatch
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_a2c_call_per_side_over_a_packed_batch(dtype):
    """three battle worlds (map 30, 2 x 40 agents, different seeds) in ONE EnvBatch, packed buffers (float32 views for "f32", cells for
    "bf16"), six cycles with AdvantageActorCritic(use_comm=True).infer_action(..., segments=batch.packed_segments(off)[g]) acting for both
    sides.  Each cycle the policy object's segmented call with a fixed u equals, bit for bit, its plain calls on every environment's rows
    of the same buffers; the pad and stale rows' actions are in range; and the worlds kept their batched form: no environment launched a
    render of its own (the batch's launches did the work), and nobody entered the large-world pipeline (pipeline_stats()[6] stays 0)."""
    import torch
    import magent_amd
    from magent_amd.builtin.torch_model import AdvantageActorCritic
    envs = []
    for k in range(3):
        env = magent_amd.GridWorld("battle", map_size=30)
        env.set_seed(300 + k)
        env.reset()
        for h in env.get_handles():
            env.add_agents(h, "random", n=40 - k)                  # (40, 39, 38: pad rows between the segments)
        env.profile_enable(1)
        envs.append(env)
    handles = envs[0].get_handles()
    dev = torch.device("cuda", envs[0].device_id)
    batch = magent_amd.EnvBatch(envs, n_threads=1)
    off, rows = batch.packed_offsets()
    hgt, wid, ch = envs[0].get_view_space(handles[0])
    F = envs[0].get_feature_space(handles[0])[0]
    n_act = envs[0].get_action_space(handles[0])[0]
    cells = dtype == "bf16"
    views = [torch.zeros((int(r), hgt, wid, 8), dtype=torch.bfloat16, device=dev) if cells else torch.zeros((int(r), hgt, wid, ch), device=dev) for r in rows]
    feats = [torch.zeros((int(r), F), device=dev) for r in rows]
    acts = [torch.zeros(int(r), dtype=torch.int32, device=dev) for r in rows]
    rews = [torch.zeros(int(r), device=dev) for r in rows]
    view_p, feat_p, act_p, rew_p = (batch.packed_pointers(t, off) for t in (views, feats, acts, rews))
    flags = batch.cell_flags([views] * 3)
    torch.manual_seed(11)
    models = [AdvantageActorCritic(envs[0], h, "side%d" % g, use_comm=True, infer_dtype=dtype) for g, h in enumerate(handles)]
    assert all(m._hip is not None and m.bf16_kernels == cells for m in models)
    us = [torch.rand(int(r), generator=torch.Generator().manual_seed(5 + g)).to(dev) for g, r in enumerate(rows)]
    torch.cuda.synchronize()
    for env in envs:
        env.profile_read("render")
    for cycle in range(6):
        batch.cycle(view_p, feat_p, act_p, rew_p, view_cells=flags)
        assert [env.profile_read("render")[0] for env in envs] == [0, 0, 0], (cycle, [env.engine_stats() for env in envs])
        tables = batch.packed_segments(off)
        for g, m in enumerate(models):
            assert m._on_kernels(views[g], feats[g])
            seg = tables[g]
            assert np.array_equal(seg[:, 0], off[:, g]) and np.array_equal(seg[:, 1], batch.nums_array()[:, g])
            out = m._hip.infer(views[g], feats[g], u=us[g], want_policy=True, want_value=True, segments=seg)
            for b, c in seg.tolist():
                if c > 0:
                    own = m._hip.infer(views[g][b:b + c], feats[g][b:b + c], u=us[g][b:b + c], want_policy=True, want_value=True)
                    assert all(torch.equal(o[b:b + c].view(torch.int32), w.view(torch.int32)) for o, w in zip(out, own)), (cycle, g, b, c)
            a = m.infer_action((views[g], feats[g]), None, segments=seg)
            assert a.dtype == torch.int32 and a.shape == (int(rows[g]),) and int(a.min()) >= 0 and int(a.max()) < n_act
            assert int(out[0].min()) >= 0 and int(out[0].max()) < n_act
            acts[g].copy_(a)
    assert all(env.pipeline_stats()[6] == 0 for env in envs), [env.pipeline_stats() for env in envs]
    for env in envs:
        env.close()
