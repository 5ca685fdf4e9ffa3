"""magent_amd.DeviceEpisodesBuffer (magent_amd/csrc/replay.hip) on synthetic packed buffers, against a numpy restatement of its contract
(class Restated below: a dict of key -> slot, and lists).  Rows are copied, never computed: every comparison is on bits.

The buffers: 5 segments laid out by EnvBatch.packed_offsets' rule (every segment starts on a multiple of 4 rows), 6-8 calls.  One segment
is empty from the start, one shrinks to empty, <= 3 pad rows lie between segments; the stale rows behind a shrunken segment and the pad
rows hold ids that ARE tracked in their world; the same ids live in every segment; agents disappear at different calls (after their
first call, at the last one); one id is duplicated inside a segment (the last row is the agent's); two agents first appear in call 3.
Every row of every call -- pad and stale rows too -- holds values of its own, so a wrong source row cannot match by accident.

Views are float32 [rows, 5, 5, 3] (300-byte rows: the 4-byte path of the copy) or bf16 cells [rows, 5, 5, 8] with view_channels=3 (the
16-byte path); features [rows, 9].  Two legs: `emu` runs replay.hip lane by lane on the CPU (helpers.build_policy_emu, from this file), `gpu`
(marked) the product library.

tests/native/replay_asan.cc drives two calls, a close and a pack through the C-ABI in a stand-alone program built from the emulated
replay.hip with -fsanitize=address,undefined (CPU only; no Python under a sanitizer)."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import helpers as H
from magent_amd import c_lib, utility
from magent_amd.replay import DeviceEpisodesBuffer

LEGS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
VIEWS = ["f32", "cells"]
H5, C, FEAT = 5, 3, 9
_made = {}


def leg_of(name):
    """(lib or None, device) of a leg"""
    if name not in _made:
        if name == "emu":
            path = H.build_policy_emu("replay", ["replay.hip"], ["policy_f32_dev.h", "policy_host.h"], __file__)
            _made[name] = (c_lib.declare_replay(ctypes.CDLL(path, mode=os.RTLD_LOCAL)), torch.device("cpu"))
        else:
            assert torch.cuda.is_available()
            _made[name] = (None, torch.device("cuda", 0))
    return _made[name]


def key_of(seg, aid):
    return (seg << 32) | (int(aid) & 0xFFFFFFFF)


class Restated(object):
    """the recorder's contract in numpy.  record_step / close take host arrays; `order` a sequence of row indices or None"""

    def __init__(self, capacity, max_transitions):
        self.capacity, self.max_transitions = capacity, max_transitions
        self.slot, self.episodes = {}, []              # key -> slot (the admission rank); per slot the list of (view, feature, action, reward)
        self.recorded, self.died = set(), set()        # the slots the previous call recorded; the slots that died
        self.transitions, self.overflow = 0, False

    def _rows(self, ids, segments):
        """(key of every in-segment row, the LAST row of every key)"""
        segments = [(0, len(ids))] if segments is None else segments
        key_of_row, last = {}, {}
        for s, (b, c) in enumerate(np.asarray(segments).tolist()):
            for r in range(b, b + c):
                key_of_row[r] = key_of(s, ids[r])
                last[key_of_row[r]] = r
        return key_of_row, last

    def _step(self, last, rows):
        if self.overflow:
            return
        present = {self.slot[k]: r for k, r in last.items() if k in self.slot}
        if rows is not None and self.transitions + len(present) > self.max_transitions:
            self.overflow = True
            return
        self.died |= self.recorded - set(present)
        if rows is None:
            self.recorded &= set(present)
            return
        for s, r in present.items():
            self.episodes[s].append(tuple(a[r].copy() for a in rows))
        self.recorded = set(present)
        self.transitions += len(present)

    def record_step(self, ids, views, feats, acts, rewards, segments=None, order=None):
        key_of_row, last = self._rows(ids, segments)
        for r in (range(len(ids)) if order is None else order):
            if len(self.slot) >= self.capacity:
                break
            k = key_of_row.get(int(r))
            if k is not None and k not in self.slot:
                self.slot[k] = len(self.slot)
                self.episodes.append([])
        self._step(last, (views, feats, acts, rewards))

    def close(self, ids, segments=None):
        self._step(self._rows(ids, segments)[1], None)

    def packed(self):
        if self.transitions == 0:
            return None
        cols, terminal, mask = [[], [], [], []], [], []
        for s, ep in enumerate(self.episodes):
            for t, tr in enumerate(ep):
                for c, v in zip(cols, tr):
                    c.append(v)
                last = t == len(ep) - 1
                terminal.append(last and s in self.died)
                mask.append(0.0 if last and s not in self.died else 1.0)
        return tuple(np.stack(c) for c in cols) + (np.array(terminal, dtype=bool), np.array(mask, dtype=np.float32))


# ---------------------------------------------------------------------------------------------------- the synthetic round
def row_data(codes, kind):
    """the four arrays of rows with the given codes (one code per row and call): every row differs from every other in every array"""
    codes = np.asarray(codes, dtype=np.int64)
    ch = C if kind == "f32" else 8
    y, x, c = np.meshgrid(np.arange(H5), np.arange(H5), np.arange(ch), indexing="ij")
    v = (codes[:, None, None, None] + 3 * y + 5 * x + 7 * c) % 200
    v[..., 0], v[..., 1] = (codes % 128)[:, None, None], (codes // 128)[:, None, None]
    views = torch.from_numpy(v.astype(np.float32))           # (integers below 256: exact in bf16)
    if kind == "cells":
        views = views.to(torch.bfloat16)
    feats = (codes[:, None] * 16 + np.arange(FEAT)[None, :] + 0.5).astype(np.float32)
    return views, torch.from_numpy(feats), torch.from_numpy((codes * 3 + 1).astype(np.int32)), torch.from_numpy((codes + 0.25).astype(np.float32))


def host_view(views, kind):
    """a view tensor as packed() returns its rows, in numpy"""
    return (views if kind == "f32" else views[..., :C].float()).numpy()


def offsets_of(counts):
    padded = (np.asarray(counts) + 3) // 4 * 4
    return (np.cumsum(padded) - padded).tolist(), int(padded.sum())


def synthetic_round(kind, n_calls=7, seed=5, quiet_first=False):
    """the calls of the module's round and the (ids, segments) after the last one; quiet_first: nobody vanishes between calls 1 and 2"""
    rs = np.random.RandomState(seed)
    worlds = [list(range(9)), [], list(range(11)), list(range(7)), list(range(13))]       # 40 rows offered by the first call
    worlds[2][6] = 2                                                                       # (id 2 twice in world 2: rows 2 and 6 of its segment)
    off, rows = offsets_of([len(w) for w in worlds])
    assert rows == 48 and off == [0, 12, 12, 24, 32]
    ids = np.full(rows, 1, dtype=np.int32)                                                 # (pad rows: id 1, which every world has)
    calls = []
    for t in range(n_calls + 1):
        if t == 2:
            worlds[0].append(100); worlds[4].append(101)                                   # (first seen by call 3; world 4 has its 14th row free)
        for w, o in zip(worlds, off):
            ids[o:o + len(w)] = w                                                          # (rows behind: stale, as the engine leaves them)
        segs = np.array([[o, len(w)] for w, o in zip(worlds, off)], dtype=np.int32)
        if t == n_calls:
            return calls, (ids.copy(), segs)
        calls.append((ids.copy(), segs) + row_data(1000 * (t + 1) + np.arange(rows), kind))
        for s, w in enumerate(worlds):                                                     # who is gone before the next call
            gone = 1 if s != 3 else (2 if t < 3 else len(w))                               # (world 3 is empty from call 4 on)
            if (t == 4 and s == 0) or (t == 0 and quiet_first):
                gone = 0
            for _ in range(min(gone, len(w))):
                w.pop(rs.randint(len(w)))


def guard(t, dev):
    """tensor t in a guarded buffer on dev"""
    name = {torch.float32: "float32", torch.int32: "int32", torch.bfloat16: "bfloat16"}[t.dtype]
    g = H.guarded(tuple(t.shape), name, dev)
    g.interior.copy_(t)
    g.before = H._guard_words(g).copy()
    return g


def make(leg, kind, capacity, max_transitions):
    lib, dev = leg_of(leg)
    return DeviceEpisodesBuffer(capacity, max_transitions, (H5, H5, C if kind == "f32" else 8), (FEAT,), view_dtype=torch.float32 if kind == "f32" else torch.bfloat16,
                                view_channels=None if kind == "f32" else C, device=dev, lib=lib)


def play(rec, want, calls, after, kind, order=None, close=True, plain=False):
    """the calls into the recorder (from guarded buffers, which stay untouched) and into the restatement"""
    dev = rec.device
    for ids, segs, views, feats, acts, rews in calls:
        gs = [guard(t, dev) for t in (torch.from_numpy(ids), views, feats, acts, rews)] + ([guard(order, dev)] if order is not None else [])
        rec.record_step(gs[0].interior, (gs[1].interior, gs[2].interior), gs[3].interior, gs[4].interior, segments=None if plain else segs,
                        order=gs[5].interior if order is not None else None)
        want.record_step(ids, host_view(views, kind), feats.numpy(), acts.numpy(), rews.numpy(), None if plain else segs, None if order is None else order.tolist())
        for g in gs:
            assert np.array_equal(H._guard_words(g), g.before), "a caller-owned input was written"
    if close:
        g = guard(torch.from_numpy(after[0]), dev)
        rec.close(g.interior, None if plain else after[1])
        want.close(after[0], None if plain else after[1])
        assert np.array_equal(H._guard_words(g), g.before)


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint8) if a.dtype == bool else a.view(np.uint32)


def assert_packed(got, want, tag):
    assert (got is None) == (want is None), tag
    if want is None:
        return
    assert got[2].dtype == torch.int32 and got[3].dtype == torch.float32 and got[4].dtype == torch.bool and got[5].dtype == torch.float32
    assert got[0].dtype == torch.float32
    for name, g, w in zip(("views", "features", "actions", "rewards", "terminal", "mask"), got, want):
        assert tuple(g.shape) == w.shape, "%s: %s %s, restated %s" % (tag, name, tuple(g.shape), w.shape)
        assert np.array_equal(bits(g), bits(w)), "%s: %s differ from the restatement's" % (tag, name)


@pytest.mark.parametrize("order_kind", ["perm", "rows"])
@pytest.mark.parametrize("kind", VIEWS)
@pytest.mark.parametrize("capacity", [13, 64])
@pytest.mark.parametrize("leg", LEGS)
def test_round_equals_the_restatement(leg, capacity, kind, order_kind):
    """capacity 13: the cut falls inside the first call's 40 offers -- exactly the first 13 in `order`.  Capacity 64: above the population;
    the two agents that first appear in call 3 are admitted then"""
    calls, after = synthetic_round(kind)
    order = torch.from_numpy(np.random.RandomState(77).permutation(48).astype(np.int32)) if order_kind == "perm" else None
    rec, want = make(leg, kind, capacity, 400), Restated(capacity, 400)
    play(rec, want, calls, after, kind, order)
    assert_packed(rec.packed(), want.packed(), "%s capacity %d" % (leg, capacity))
    s = rec.stats()
    assert s == {"tracked": len(want.slot), "transitions": want.transitions, "overflow": False}
    if capacity == 13:
        seq = range(48) if order is None else order.tolist()
        offered = [r for r in seq if any(b <= r < b + c for b, c in calls[0][1].tolist())]
        first, seen = [], set()
        for r in offered:                                       # (the duplicated id offers its key twice: once counts)
            k = next(key_of(s_, calls[0][0][r]) for s_, (b, c) in enumerate(calls[0][1].tolist()) if b <= r < b + c)
            if k not in seen:
                seen.add(k); first.append(k)
        assert list(want.slot) == first[:13] and s["tracked"] == 13
    else:
        assert key_of(0, 100) in want.slot and key_of(4, 101) in want.slot and len(want.slot) == 41
        assert want.slot[key_of(0, 100)] >= 39                  # (admitted after everybody of the first call)
    # the properties the round was built for, read from the restatement
    p = want.packed()
    assert p[4].any() and (p[5] == 0).any() or capacity == 13
    assert (2 << 32 | 2) in want.slot or capacity == 13
    buf = rec.buffer
    assert set(buf) == {(k >> 32, k & 0xFFFFFFFF) for k in want.slot}
    for k, s_ in want.slot.items():
        ep, w = buf[(k >> 32, k & 0xFFFFFFFF)], want.episodes[s_]
        assert len(ep.rewards) == len(w) and ep.terminal == (s_ in want.died and len(w) > 0)
        assert [int(a) for a in ep.actions] == [int(tr[2]) for tr in w]
        assert all(np.array_equal(bits(v), bits(tr[0])) for v, tr in zip(ep.views, w))


@pytest.mark.parametrize("leg", LEGS)
def test_duplicated_id_takes_its_last_row_and_stale_rows_are_nobodys(leg):
    calls, after = synthetic_round("f32")
    rec, want = make(leg, "f32", 64, 400), Restated(64, 400)
    play(rec, want, calls[:2], after, "f32", close=False)
    ep = rec.buffer[(2, 2)]
    ids, segs, views = calls[0][0], calls[0][1], calls[0][2]
    b = int(segs[2][0])
    assert ids[b + 2] == 2 and ids[b + 6] == 2
    assert np.array_equal(bits(ep.views[0]), bits(views[b + 6])) and not np.array_equal(bits(ep.views[0]), bits(views[b + 2]))
    # call 1's stale rows hold ids tracked in their world: none of them is anybody's second transition
    ids1, segs1, views1 = calls[1][0], calls[1][1], calls[1][2]
    stale = [r for s, (b1, c1) in enumerate(segs1.tolist()) for r in range(b1 + c1, b1 + int(segs[s][1]))]
    assert stale and all(key_of(s, ids1[r]) in want.slot for s, (b1, c1) in enumerate(segs1.tolist()) for r in range(b1 + c1, b1 + int(segs[s][1])))
    p = rec.packed()[0]
    for r in stale:
        assert not (bits(p).reshape(len(p), -1) == bits(views1[r]).reshape(1, -1)).all(axis=1).any()


@pytest.mark.parametrize("kind", VIEWS)
@pytest.mark.parametrize("leg", LEGS)
def test_without_close_the_last_calls_agents_end_unfinished(leg, kind):
    calls, after = synthetic_round(kind, n_calls=6)
    outs = []
    for close in (True, False):
        rec, want = make(leg, kind, 64, 400), Restated(64, 400)
        play(rec, want, calls, after, kind, close=close)
        assert_packed(rec.packed(), want.packed(), "%s close=%s" % (leg, close))
        outs.append((rec.packed(), want))
    (with_close, w1), (without, w0) = outs
    last = w1.recorded | (w1.died - w0.died)                    # the slots the last call recorded
    gone = w1.died - w0.died
    assert gone, "agents vanish after the last call"
    ends = np.cumsum([len(e) for e in w1.episodes]) - 1
    for s in last:
        assert bool(with_close[4][ends[s]]) == (s in gone) and float(without[5][ends[s]]) == 0.0 and not bool(without[4][ends[s]])


@pytest.mark.parametrize("leg", LEGS)
def test_wide_scan(leg):
    """capacity 1500, 1400 one-transition agents in one call: the scans cross a workgroup's width"""
    n = 1400
    ids = np.random.RandomState(3).permutation(5000)[:n].astype(np.int32)
    data = row_data(np.arange(n), "cells")
    order = torch.from_numpy(np.random.RandomState(4).permutation(n).astype(np.int32))
    rec, want = make(leg, "cells", 1500, 1500), Restated(1500, 1500)
    play(rec, want, [(ids, None) + data], (ids[:700].copy(), None), "cells", order=order, plain=True)
    assert_packed(rec.packed(), want.packed(), leg)
    assert rec.stats()["tracked"] == n and int(rec.packed()[4].sum()) == 700
    assert set(rec.buffer) == set(ids.tolist())                 # (without segments the buffer is keyed by id)


@pytest.mark.parametrize("leg", LEGS)
def test_long_table(leg):
    """300 segments of 1-3 rows in one call: the table is cut into two launches"""
    rs = np.random.RandomState(9)
    counts = rs.randint(1, 4, size=300)
    off, rows = offsets_of(counts)
    segs = np.stack([off, counts], axis=1).astype(np.int32)
    ids = np.full(rows, 0, dtype=np.int32)
    for b, c in segs.tolist():
        ids[b:b + c] = rs.permutation(4)[:c]
    data = row_data(np.arange(rows), "f32")
    segs2 = segs.copy()
    segs2[::2, 1] -= 1                                           # (every other world loses its last agent)
    data2 = row_data(3000 + np.arange(rows), "f32")
    rec, want = make(leg, "f32", 700, 1300), Restated(700, 1300)
    play(rec, want, [(ids, segs) + data, (ids, segs2) + data2], (ids, segs2), "f32", order=torch.from_numpy(rs.permutation(rows).astype(np.int32)))
    assert_packed(rec.packed(), want.packed(), leg)
    assert rec.stats()["tracked"] == int(counts.sum()) and (299, int(ids[off[299]])) in rec.buffer


@pytest.mark.parametrize("quiet_first", [True, False])
@pytest.mark.parametrize("kind", VIEWS)
@pytest.mark.parametrize("leg", LEGS)
def test_overflow(leg, kind, quiet_first):
    """max_transitions takes calls 1-2 and not the third: calls 1-2 whole, nothing afterwards, packed() warns.  Every episode that call 2
    recorded ends unfinished (mask 0): with quiet_first that is every episode.  Without it some agents vanished between calls 1 and 2,
    which call 2 -- recorded whole -- detected: their one transition is terminal, as the contract has it."""
    calls, after = synthetic_round(kind, quiet_first=quiet_first)
    probe = Restated(64, 10 ** 6)
    for k, c in enumerate(calls[:3]):
        two = probe.transitions                                  # (after the loop: what calls 1-2 record)
        probe.record_step(c[0], host_view(c[2], kind), c[3].numpy(), c[4].numpy(), c[5].numpy(), c[1])
    room = probe.transitions - 1                                 # (one row short of the third call)
    assert two < room
    rec, want = make(leg, kind, 64, room), Restated(64, room)
    play(rec, want, calls, after, kind)
    assert want.overflow and want.transitions == two
    with pytest.warns(RuntimeWarning):
        got = rec.packed()
    assert_packed(got, want.packed(), leg)
    s = rec.stats()
    assert s["overflow"] and s["transitions"] == two
    lens = np.array([len(e) for e in want.episodes if e])
    ends = np.cumsum(lens) - 1
    early = np.array([s_ in want.died for s_, e in enumerate(want.episodes) if e])      # (vanished between calls 1 and 2)
    assert early.any() != quiet_first and (lens[early] == 1).all() and (lens[~early] == 2).all()
    mask, terminal = got[5].cpu().numpy(), got[4].cpu().numpy()
    assert (mask[ends[~early]] == 0).all() and not terminal[ends[~early]].any() and terminal[ends[early]].all() and terminal.sum() == early.sum()
    assert float(mask.sum()) == two - (~early).sum()


@pytest.mark.parametrize("leg", LEGS)
def test_nothing_recorded_and_reset(leg):
    calls, after = synthetic_round("f32")
    rec = make(leg, "f32", 13, 400)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert rec.packed() is None and rec.buffer == {} and list(rec.episodes()) == []
        empty = np.zeros((5, 2), dtype=np.int32)
        rec.record_step(*[t.to(rec.device) for t in (torch.from_numpy(calls[0][0]),)], tuple(t.to(rec.device) for t in calls[0][2:4]),
                        calls[0][4].to(rec.device), calls[0][5].to(rec.device), segments=empty)
        assert rec.packed() is None and rec.stats() == {"tracked": 0, "transitions": 0, "overflow": False}
    want = Restated(13, 400)
    play(rec, want, calls[:3], after, "f32", close=False)
    assert_packed(rec.packed(), want.packed(), "first round")
    rec.reset()
    assert rec.packed() is None
    want = Restated(13, 400)
    order = torch.from_numpy(np.random.RandomState(1).permutation(48).astype(np.int32))
    play(rec, want, calls, after, "f32", order=order)
    fresh = make(leg, "f32", 13, 400)
    play(fresh, Restated(13, 400), calls, after, "f32", order=order)
    assert_packed(rec.packed(), want.packed(), "after reset")
    for a, b in zip(rec.packed(), fresh.packed()):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("leg", LEGS)
def test_refused_tables_record_nothing(leg):
    calls, after = synthetic_round("f32")
    rec, want = make(leg, "f32", 64, 400), Restated(64, 400)
    play(rec, want, calls[:1], after, "f32", close=False)
    ids, segs, views, feats, acts, rews = calls[1]
    dev = rec.device
    args = lambda table: ((torch.from_numpy(ids).to(dev), (views.to(dev), feats.to(dev)), acts.to(dev), rews.to(dev)), {"segments": table})
    overlap, beyond, negative = segs.copy(), segs.copy(), segs.copy()
    overlap[2, 0] = 5
    beyond[4, 1] = 17
    negative[3, 1] = -1
    for table, word in ((overlap, "segment 2"), (beyond, "segment 4"), (negative, "segment 3")):
        a, kw = args(table)
        with pytest.raises(ValueError, match=word):
            rec.record_step(*a, **kw)
        with pytest.raises(ValueError, match=word):
            rec.close(a[0], table)
    assert_packed(rec.packed(), want.packed(), "after the refusals")
    play(rec, want, calls[1:], after, "f32")
    assert_packed(rec.packed(), want.packed(), "the round goes on")


@pytest.mark.parametrize("leg", LEGS)
def test_one_world_against_episodes_buffer(leg):
    """one world, segments=None, capacity >= population, close given: per id exactly the episode utility.EpisodesBuffer builds from the same
    steps (fed with alives = "present in the next ids"; compared per id: its admission order is its own)"""
    rs = np.random.RandomState(21)
    alive = list(range(30))
    rec, host = make(leg, "f32", 40, 300), utility.EpisodesBuffer(40)
    dev = rec.device
    steps = []
    for t in range(6):
        ids = np.array(alive, dtype=np.int32)
        for _ in range(3 if t != 2 else 0):
            alive.pop(rs.randint(len(alive)))
        steps.append((ids, np.isin(ids, alive)))
    for t, (ids, alives) in enumerate(steps):
        views, feats, acts, rews = row_data(500 * t + np.arange(len(ids)), "f32")
        rec.record_step(torch.from_numpy(ids).to(dev), (views.to(dev), feats.to(dev)), acts.to(dev), rews.to(dev))
        host.record_step(ids, (views.numpy(), feats.numpy()), acts.numpy(), rews.numpy(), alives)
    rec.close(torch.from_numpy(np.array(alive, dtype=np.int32)).to(dev))
    got, want = rec.buffer, host.buffer
    assert set(got) == set(want) == set(range(30))
    for i, w in want.items():
        g = got[i]
        assert g.terminal == w.terminal and [int(a) for a in g.actions] == w.actions
        assert np.array_equal(bits(np.asarray(g.rewards, dtype=np.float32)), bits(np.asarray(w.rewards, dtype=np.float32)))
        assert np.array_equal(bits(torch.stack(g.views)), bits(np.stack(w.views))) and np.array_equal(bits(torch.stack(g.features)), bits(np.stack(w.features)))
    assert any(e.terminal for e in got.values()) and not all(e.terminal for e in got.values())


def test_a_library_without_the_entries_says_rebuild():
    class Old(object):
        has_replay_api = False
    with pytest.raises(RuntimeError, match="rebuild"):
        DeviceEpisodesBuffer(4, 4, (5, 5, 3), (9,), lib=Old())


def test_the_host_code_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/replay_asan.cc with the emulated replay.hip and the emulator's runtime, built here with -fsanitize=address,undefined:
    every buffer is a heap block of exactly the stated size.  Exit code 0 and no report.  Skipped only where a one-line program does not
    link with the flags."""
    leg_of("emu")
    sys.path.insert(0, os.path.join(H.ROOT, "tests", "hipemu"))
    import build as emu_build
    out = os.path.join(H.ROOT, "tests", "hipemu", "_build", "replay")
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-strict-aliasing", "-ffp-contract=off", "-w"]
    (tmp_path / "probe.cc").write_text("int main() { return 0; }\n")
    probe = subprocess.run([emu_build.CXX] + flags + [str(tmp_path / "probe.cc"), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("%s does not link with -fsanitize=address,undefined: %s" % (emu_build.CXX, probe.stderr[-300:]))
    exe = str(tmp_path / "replay_asan")
    subprocess.run([emu_build.CXX] + flags + ["-I", emu_build.HERE, "-I", out, "-I", emu_build.CSRC, "-I", os.path.join(H.ROOT, "include"),
                                              os.path.join(out, "replay_emu.cc"), os.path.join(emu_build.HERE, "emu_runtime.cc"),
                                              os.path.join(H.ROOT, "tests", "native", "replay_asan.cc"), "-o", exe, "-lpthread"], check=True)
    env = H.merge_env(os.environ, {"ASAN_OPTIONS": "halt_on_error=1:exitcode=66", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "replay_asan ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-4000:])
