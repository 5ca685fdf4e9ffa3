"""The rule-based actors' device kernels (magent_amd/csrc/actors.hip), drawn actions included, against an exact restatement.

tests/test_rule_actors.py only requires a drawn action to lie in the set the reference could have drawn from.  DESIGN.md 3.16
specifies the draw completely, so the drawn action is a function of (seed, counter, agent, observation): `np_draw` restates the
draw in NumPy uint64 arithmetic from the four lines of that section, `np_actor` the three policies with the exact value wherever
a draw decides, and the kernels must EQUAL it for every agent -- on the CPU emulator (`emu`) and, marked `gpu`, on the product
library in-process with torch tensors.

* the draw's own properties (known answers in plain Python integers, chi-square, stream independence) are checked on `np_draw`
  alone: the kernels are proven equal to it, so they need no GPU;
* constructed observations force each path: the k-th pick across 64-cell rounds, my position (the LAST cell with channel 3 > 1),
  slot 1, the diagonal tie-break, the first ATTACKABLE hit, the cell in front, NaN / inf features and cells, views below 3 x 3;
* call edges: n around the four-agents-per-workgroup tail, `drew == NULL`, buffers inside sentinel-filled allocations, another
  stream, the largest accepted view (16384 cells: 64 KiB of dynamic LDS), a seeded random sweep of shapes.

Seeds lie above 2^63 and counters above 2^32 throughout, so a truncated seed or counter cannot pass.
"""
import ctypes
import functools
import os
import statistics

import numpy as np
import pytest

import helpers as H
import test_rule_actors as T

LEGS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
SEED = 0xD1B54A32D192ED03            # > 2^63
COUNTER = 2 ** 40 + 3                # > 2^32
M64 = 2 ** 64 - 1
GOLDEN = 0x9E3779B97F4A7C15


# ---------------------------------------------------------------------------------------------- the restatement
def _np_mix(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def np_draw(seed, counter, row, slot, m):
    """value in [0, m) of draw `slot` of agent `row` (an int or an array of them) in call `counter` of stream `seed`:
         key = mix(seed ^ mix(counter + G));  h = mix(key + G * (4 row + slot + 1));  (h >> 32) % m
    in uint64 arrays (NumPy wraps them silently) -> int, or int64 array"""
    u = lambda x: np.atleast_1d(np.asarray(x, dtype=np.uint64))
    g = np.uint64(GOLDEN)
    key = _np_mix(u(seed & M64) ^ _np_mix(u(counter & M64) + g))
    h = _np_mix(key + g * (u(row) * np.uint64(4) + u(slot) + np.uint64(1)))
    out = ((h >> np.uint64(32)) % np.uint64(m)).astype(np.int64)
    return int(out[0]) if np.ndim(row) == 0 else out


def _py_mix(z):
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def py_draw(seed, counter, row, slot, m):
    """the same four lines in plain Python integers"""
    key = _py_mix(seed ^ _py_mix((counter + GOLDEN) & M64))
    h = _py_mix((key + GOLDEN * (4 * row + slot + 1)) & M64)
    return (h >> 32) % m


def _forward_free(x):
    """temp_c_booster.cc:74, `(int)(x + 0.5) != 1` in double; a NaN or an infinite cell converts to no 1 on x86 and on the GPU"""
    t = float(x) + 0.5
    return not (np.isfinite(t) and int(t) == 1)


def np_actor(kind, view, feat, p, seed, counter):
    """-> (actions int32[n], drew uint8[n]): the reference's decision rules (as T.possible_sets restates them), with the exact
    value of DESIGN.md 3.16 wherever a draw decides"""
    view = np.ascontiguousarray(view, dtype=np.float32)
    n, h, w, c = view.shape
    base, v2a = p["base"], np.asarray(p["v2a"], dtype=np.int64).reshape(-1)
    flat = np.ascontiguousarray(feat, dtype=np.float32).reshape(-1)
    act, drew = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    for i in range(n):
        o = view[i].reshape(h * w, c)
        draw = lambda slot, m: np_draw(seed, counter, i, slot, m)
        if kind == "runaway":
            rows = [r for r in range(h - 3, h) if r >= 0]
            cols = [q for q in range(w // 2 - 1, w // 2 + 2) if 0 <= q < w]
            sees = any(view[i, r, q, p["channel"]] > np.float32(0.5) for r in rows for q in cols)
            act[i] = p["move_back"] if sees else p["move_back"] + 1
        elif kind == "rush":
            a = -1
            if flat[i] < np.float32(p["threshold"]):
                hit = (o[:, p["channel"]] > np.float32(0.5)) | (o[:, 1] > np.float32(0.5))
                att = np.nonzero(hit & (v2a != -1))[0]
                if len(att):
                    a = base + v2a[att[0]]
                elif hit.any() and _forward_free(view[i, h - 1, w // 2, 0]):
                    a = 0
            if a < 0:
                a, drew[i] = draw(0, base), 1
            act[i] = a
        else:
            food = o[:, 4] == np.float32(1.0)
            att = np.nonzero(food & (v2a != -1))[0]
            disp = np.nonzero(food & (v2a == -1))[0]
            drew[i] = 1
            if len(att):
                a = v2a[att[draw(0, len(att))]] + base
            elif len(disp):
                dr, dc = disp[0] // w - h // 2, disp[0] % w - w // 2
                if dr == dc and abs(dc) == 1:
                    if draw(0, 2) == 1:
                        dr = 0
                    else:
                        dc = 0
                else:
                    drew[i] = 0
                a = T._get_action(dr, dc, False)
            else:
                mm = np.nonzero(o[:, 6] > np.float32(0.0))[0]
                if not len(mm):
                    a = draw(0, base)
                else:
                    me = np.nonzero(o[:, 3] > np.float32(1.0))[0]
                    mr, mc = (me[-1] // w, me[-1] % w) if len(me) else (-1, -1)
                    cell = mm[draw(0, len(mm))]
                    a = T._get_action(cell // w - mr, cell % w - mc, True)
                    if a == 6:
                        a = draw(1, base)
            act[i] = a
    return act, drew


# ---------------------------------------------------------------------------------------------- the two legs
GUARD = 64
ACT_FILL, DREW_FILL = -7, 9


class Leg(object):
    """`emu`: the kernels compiled against tests/hipemu, on host memory; `gpu`: the product library on cuda:0, torch tensors.
    run(...) -> (actions, drew or None).  `lead` is None: plain buffers (on the emulator T.device_call).  Otherwise `actions` and
    `drew` start `lead` elements into allocations filled with sentinels and GUARD more follow them: no byte outside may change."""

    def __init__(self, name):
        self.name = name
        if name == "emu":
            self.path = T.build_actor_emu()
            self.fn = ctypes.CDLL(self.path, mode=os.RTLD_LOCAL).actor_infer_action_device
            self.fn.restype, self.fn.argtypes = ctypes.c_int, [ctypes.c_void_p] * 7
        else:
            import torch
            from magent_amd import c_lib
            self.torch, self.dev = torch, torch.device("cuda", 0)
            self.fn = c_lib.load(H.HIP_LIB).actor_infer_action_device

    def run(self, kind, view, feat, p, seed=SEED, counter=COUNTER, lead=None, with_drew=True, stream=False):
        view = np.ascontiguousarray(view, dtype=np.float32)
        feat = np.ascontiguousarray(feat, dtype=np.float32)
        n, h, w, c = view.shape
        if self.name == "emu" and lead is None and with_drew:
            act, drew = T.device_call(self.path, kind, view, feat, p, seed=seed, counter=counter)
            assert (act != ACT_FILL).all() and (drew != DREW_FILL).all(), "an agent's action or mark was not written"
            return act, drew
        lead = 0 if lead is None else lead
        v2a = np.ascontiguousarray(p["v2a"], dtype=np.int32).reshape(-1)
        args = T.ActorArgs(T.KIND[kind], n, h, w, c, p["base"], p["channel"], p["move_back"], p["threshold"], seed & M64, counter)
        size = lead + n + GUARD
        if self.name == "emu":
            act, drew = np.full(size, ACT_FILL, dtype=np.int32), np.full(size, DREW_FILL, dtype=np.uint8)
            assert self.fn(ctypes.byref(args), view.ctypes.data, feat.ctypes.data, v2a.ctypes.data, act.ctypes.data + 4 * lead,
                           drew.ctypes.data + lead if with_drew else None, None) == 0
        else:
            torch = self.torch
            side = torch.cuda.Stream(self.dev) if stream else torch.cuda.current_stream(self.dev)
            dv, df, da = (torch.from_numpy(x.copy()).to(self.dev) for x in (view, feat, v2a))      # (the shared inputs are read-only)
            act_d = torch.full((size,), ACT_FILL, dtype=torch.int32, device=self.dev)
            drew_d = torch.full((size,), DREW_FILL, dtype=torch.uint8, device=self.dev)
            side.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(side):
                assert self.fn(ctypes.byref(args), dv.data_ptr(), df.data_ptr(), da.data_ptr(), act_d.data_ptr() + 4 * lead,
                               drew_d.data_ptr() + lead if with_drew else None, side.cuda_stream) == 0
                act, drew = act_d.cpu().numpy(), drew_d.cpu().numpy()
            torch.cuda.current_stream(self.dev).wait_stream(side)
        inside = np.zeros(size, dtype=bool)
        inside[lead:lead + n] = True
        assert (act[~inside] == ACT_FILL).all(), "actions written outside [0, %d): at %s" % (n, np.nonzero(act[~inside] != ACT_FILL)[0][:5])
        assert (drew[~inside] == DREW_FILL).all(), "drew written outside [0, %d)" % n
        assert (act[inside] != ACT_FILL).all(), "an agent's action was not written"
        if not with_drew:
            assert (drew == DREW_FILL).all(), "drew written although NULL was passed"
            return act[inside], None
        return act[inside], drew[inside]


_LEGS = {}


def leg(name):
    if name not in _LEGS:
        _LEGS[name] = Leg(name)
    return _LEGS[name]


def params(h, w, attack=None, base=13, channel=3, threshold=100.0):
    """actor parameters; `attack` {cell: view2attack value}, every other cell -1"""
    v2a = -np.ones(h * w, dtype=np.int32)
    for cell, value in (attack or {}).items():
        v2a[cell] = value
    return {"base": base, "v2a": v2a.reshape(h, w), "threshold": threshold, "move_back": 4, "channel": channel}


def front_is_finite(view):
    n, h, w, c = view.shape
    return bool(np.isfinite(view[:, h - 1, w // 2, 0]).all())


def assert_device_equals_restatement(lg, kind, view, feat, p, want=None, seed=SEED, counter=COUNTER, ref=False, what="", **how):
    """the device's (actions, drew) == np_actor's for every agent; where nothing was drawn also the host path's action and -- on
    the CPU leg, for inputs the reference defines (`ref`) -- the compiled reference's"""
    want_act, want_drew = want if want is not None else np_actor(kind, view, feat, p, seed, counter)
    act, drew = leg(lg).run(kind, view, feat, p, seed=seed, counter=counter, **how)
    bad = np.nonzero(act != want_act)[0]
    assert not len(bad), "%s %s: %d of %d actions differ from the restatement, first %s: device %s, restated %s (drew %s)" % (
        kind, what, len(bad), len(act), bad[:6], act[bad[:6]], want_act[bad[:6]], want_drew[bad[:6]])
    if drew is not None:
        assert drew.dtype == np.uint8 and (drew == want_drew).all(), "%s %s: drew differs at %s" % (
            kind, what, np.nonzero(drew != want_drew)[0][:6])
    exact = want_drew == 0
    T.LIBC.srandom(1)
    host = T.call(getattr(T.product(), T.PRODUCT_SYMBOLS[kind]), kind, view, feat, p)
    assert (act[exact] == host[exact]).all(), "%s %s: undrawn actions differ from the host path at %s" % (
        kind, what, np.nonzero(exact & (act != host))[0][:6])
    if ref and lg == "emu" and H.have_ref() and exact.any():
        keep = ~T.gather_divides_by_zero(view, p) if kind == "gather" else np.ones(len(view), dtype=bool)
        H.single_threaded_reference()
        T.LIBC.srandom(1)
        theirs = T.call(T.reference(kind), kind, view[keep], feat, p)      # (gather reads no feature: the rows need not match)
        both = exact[keep]
        assert (theirs[both] == act[keep][both]).all(), "%s %s: undrawn actions differ from the compiled reference" % (kind, what)
    return act, drew


# ---------------------------------------------------------------------------------------------- 1. the restatement itself
def test_splitmix_finaliser_reproduces_the_published_stream():
    """mix is the output function of splitmix64 (Steele, Lea, Flood 2014; Vigna's splitmix64.c): its first outputs for state 0"""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC]
    assert [_py_mix(GOLDEN * (k + 1) & M64) for k in range(4)] == want
    assert _np_mix(np.array([GOLDEN * (k + 1) & M64 for k in range(4)], dtype=np.uint64)).tolist() == want


KNOWN = [   # (seed, counter, row, slot, m)
    (0, 0, 0, 0, 13), (1, 0, 0, 0, 13), (7, 1, 5, 0, 2), (0x6D6167656E74, 12, 399999, 0, 21), (M64, 2 ** 40 + 3, 2 ** 24, 1, 13),
    (SEED, COUNTER, 2 ** 31 - 1, 1, 5), (1 << 63, 1 << 63, 0, 1, 2 ** 31 - 1), (M64, M64, 2 ** 32 - 1, 1, 1),
]


def test_np_draw_equals_the_hand_evaluation():
    assert [py_draw(*k) for k in KNOWN] == [8, 8, 1, 13, 1, 0, 410772749, 0]      # (evaluated once, kept as a pin of py_draw)
    for seed, counter, row, slot, m in KNOWN:
        want = py_draw(seed, counter, row, slot, m)
        assert 0 <= want < m
        assert np_draw(seed, counter, row, slot, m) == want, (seed, counter, row, slot, m)
        rows = np.array([row, 0, row], dtype=np.uint64)
        assert np_draw(seed, counter, rows, slot, m).tolist() == [want, py_draw(seed, counter, 0, slot, m), want]
    # the issue's example, spelled out step by step: every intermediate in Python integers
    seed, counter, row, slot = M64, 2 ** 40 + 3, 2 ** 24, 1
    inner = _py_mix((counter + GOLDEN) % 2 ** 64)
    key = _py_mix(seed ^ inner)
    h = _py_mix((key + GOLDEN * (4 * row + slot + 1)) % 2 ** 64)
    assert np_draw(seed, counter, row, slot, 13) == (h // 2 ** 32) % 13


# ---------------------------------------------------------------------------------------------- 2. the draw's own properties
ROWS = 200000


def chi2_bound(df, p=1e-6):
    """the chi-square quantile at upper tail probability p: scipy.stats.chi2.isf(p, df) where scipy is present, otherwise the
    Wilson-Hilferty approximation  df (1 - 2 / (9 df) + z sqrt(2 / (9 df)))^3  with z the normal quantile at 1 - p"""
    try:
        from scipy import stats
        return float(stats.chi2.isf(p, df))
    except ImportError:
        z = statistics.NormalDist().inv_cdf(1.0 - p)
        return df * (1.0 - 2.0 / (9.0 * df) + z * (2.0 / (9.0 * df)) ** 0.5) ** 3


def chi2(values, cells):
    counts = np.bincount(values, minlength=cells)
    assert len(counts) == cells
    e = len(values) / cells
    return float(((counts - e) ** 2 / e).sum())


@pytest.mark.parametrize("m", [2, 5, 13, 21])
@pytest.mark.parametrize("slot", [0, 1])
def test_draws_are_uniform(slot, m):
    """2 x 10^5 rows of one call: a fixed function of the seed, so the test is deterministic"""
    x = chi2(np_draw(SEED, COUNTER, np.arange(ROWS), slot, m), m)
    print("slot %d m %d: chi-square %.2f, bound %.2f" % (slot, m, x, chi2_bound(m - 1)))
    assert x < chi2_bound(m - 1), (x, chi2_bound(m - 1))


def test_draws_of_the_two_slots_and_of_neighbouring_rows_are_independent():
    m = 5
    rows = np.arange(ROWS)
    a, b = np_draw(SEED, COUNTER, rows, 0, m), np_draw(SEED, COUNTER, rows, 1, m)
    x = chi2(a * m + b, m * m)
    print("slots 0 and 1: chi-square %.2f, bound %.2f" % (x, chi2_bound(m * m - 1)))
    assert x < chi2_bound(m * m - 1), x
    for slot, v in ((0, a), (1, b)):      # disjoint pairs (row, row + 1)
        x = chi2(v[0::2] * m + v[1::2], m * m)
        print("rows r and r + 1, slot %d: chi-square %.2f, bound %.2f" % (slot, x, chi2_bound(m * m - 1)))
        assert x < chi2_bound(m * m - 1), (slot, x)


def test_streams_of_other_counters_and_seeds_differ():
    m = 13
    rows = np.arange(ROWS)
    for slot in (0, 1):
        mine = np_draw(SEED, COUNTER, rows, slot, m)
        for what, other in (("counter + 1", np_draw(SEED, COUNTER + 1, rows, slot, m)),
                            ("counter + 2^32", np_draw(SEED, COUNTER + 2 ** 32, rows, slot, m)),
                            ("seed ^ 2^63", np_draw(SEED ^ (1 << 63), COUNTER, rows, slot, m)),
                            ("seed + 2^32", np_draw(SEED + 2 ** 32, COUNTER, rows, slot, m))):
            assert (mine != other).mean() >= 1.0 - 1.0 / m - 0.01, (slot, what, (mine != other).mean())
    assert (np_draw(SEED, COUNTER, rows, 0, m) != np_draw(SEED, COUNTER, rows, 1, m)).mean() >= 1.0 - 1.0 / m - 0.01


# ---------------------------------------------------------------------------------------------- 3. constructed observations
def blank(n, h, w, c=7):
    return np.zeros((n, h, w, c), dtype=np.float32), np.zeros((n, 3), dtype=np.float32)


def cells_of(view):
    n, h, w, c = view.shape
    return view.reshape(n, h * w, c)       # (a view of the same memory)


KTH_CELLS = [40, 64, 77, 100, 127, 128, 130, 141, 150, 155, 160, 168]      # 1 + 4 + 7 over the three rounds of 13 x 13
KTH_V2A = [7, 2, 11, 0, 5, 9, 3, 10, 1, 6, 4, 8]


def case_gather_kth_rounds():
    view, feat = blank(96, 13, 13)
    o = cells_of(view)
    o[:, KTH_CELLS, 4] = 1.0
    o[:, [10, 90, 165], 4] = 1.0           # food that cannot be attacked: not in the set
    o[:, 41, 4] = 0.5                      # attackable, but no food
    o[:, 129, 4] = 2.0
    o[:, 131, 4] = np.nan
    attack = dict(zip(KTH_CELLS, KTH_V2A))
    attack[41] = 12
    p = params(13, 13, attack)

    def expect(act, drew):
        k = np_draw(SEED, COUNTER, np.arange(96), 0, 12)
        assert sorted(set(k.tolist())) == list(range(12)), "the case must reach every k"
        assert drew.all() and act.tolist() == [13 + KTH_V2A[j] for j in k]
    return "gather", view, feat, p, expect, False


def _case_gather_kth_shape(h, w):
    def build():
        view, feat = blank(40, h, w)
        food = sorted(set(x for x in (0, 63, 64, h * w - 1) if x < h * w))
        cells_of(view)[:, food, 4] = 1.0
        p = params(h, w, {x: 3 + 2 * j for j, x in enumerate(food)})

        def expect(act, drew):
            k = np_draw(SEED, COUNTER, np.arange(40), 0, len(food))
            assert sorted(set(k.tolist())) == list(range(len(food)))
            assert drew.all() and act.tolist() == [13 + 3 + 2 * j for j in k]
        return "gather", view, feat, p, expect, False
    return build


MAP_CELLS = [(0, 0), (1, 6), (2, 10), (6, 2), (6, 9), (8, 3), (10, 6), (11, 9), (12, 0)]      # three in each round of 13 x 13
MAP_ACTIONS = [1, 0, 3, 4, 8, 9, 12, 11, 9]        # get_action(cell - (6, 6), stride): neighbours in rank differ


def case_minimap_rounds():
    view, feat = blank(64, 13, 13)
    for j, (r, q) in enumerate(MAP_CELLS):
        view[:, r, q, 6] = (0.5, 2.0, 0.7)[j % 3]
    view[:, 0, 5, 6], view[:, 5, 5, 6], view[:, 12, 12, 6] = -1.0, np.nan, -np.inf       # no minimap cells
    view[:, 6, 6, 3] = 2.0
    view[:, 9, 9, 3] = 1.0                  # (not > 1)

    def expect(act, drew):
        assert [r * 13 + q for r, q in MAP_CELLS] == sorted(r * 13 + q for r, q in MAP_CELLS)
        assert [sum(64 * b <= r * 13 + q < 64 * b + 64 for r, q in MAP_CELLS) for b in range(3)] == [3, 3, 3]
        assert [T._get_action(r - 6, q - 6, True) for r, q in MAP_CELLS] == MAP_ACTIONS
        k = np_draw(SEED, COUNTER, np.arange(64), 0, 9)
        assert sorted(set(k.tolist())) == list(range(9))
        assert drew.all() and act.tolist() == [MAP_ACTIONS[j] for j in k]
    return "gather", view, feat, params(13, 13, {3: 1, 80: 2}), expect, False


MYPOS_MAP = [5, 60, 70, 100, 140, 167]
MYPOS_HITS = [([20, 50, 135, 150], 150), ([20, 50], 50), ([], None), ([20, 90], 90), ([63, 64], 64), ([168, 0], 168)]


def case_mypos_last_wins():
    """channel 3 > 1 in rounds 0 and 2 (two cells each), in round 0 only, nowhere, in rounds 0 and 1, on both sides of a round's
    edge, in the first and the last cell: 16 agents each"""
    view, feat = blank(16 * len(MYPOS_HITS), 13, 13)
    o = cells_of(view)
    o[:, MYPOS_MAP, 6] = 0.7
    o[:, 160, 3], o[:, 165, 3], o[:, 166, 3] = 1.0, np.nan, -np.inf        # (not > 1)
    for g, (hits, _) in enumerate(MYPOS_HITS):
        o[16 * g:16 * g + 16, hits, 3] = 2.0

    def expect(act, drew):
        assert drew.all()
        for g, (_, me) in enumerate(MYPOS_HITS):
            mr, mc = (me // 13, me % 13) if me is not None else (-1, -1)
            for i in range(16 * g, 16 * g + 16):
                cell = MYPOS_MAP[np_draw(SEED, COUNTER, i, 0, len(MYPOS_MAP))]
                assert act[i] == T._get_action(cell // 13 - mr, cell % 13 - mc, True), (g, i)
    return "gather", view, feat, params(13, 13), expect, False


def case_slot1():
    view, feat = blank(64, 13, 13)
    view[:, 7, 5, 6] = 0.7
    view[:, 7, 5, 3] = 2.0

    def expect(act, drew):
        rows = np.arange(64)
        assert drew.all() and act.tolist() == np_draw(SEED, COUNTER, rows, 1, 13).tolist()
        assert (np_draw(SEED, COUNTER, rows, 1, 13) != np_draw(SEED, COUNTER, rows, 0, 13)).mean() > 0.8
    return "gather", view, feat, params(13, 13), expect, False


DIAGONALS = [(1, 1), (-1, -1), (1, -1), (-1, 1)]


def _case_diagonal(h, w):
    def build():
        view, feat = blank(16 * 4, h, w)
        view[:, h - 1, 1, 4] = 1.0         # a later food cell: not the first
        for g, (dr, dc) in enumerate(DIAGONALS):
            view[16 * g:16 * g + 16, h // 2 + dr, w // 2 + dc, 4] = 1.0

        def expect(act, drew):
            for g, (dr, dc) in enumerate(DIAGONALS):
                for i in range(16 * g, 16 * g + 16):
                    if dr == dc:
                        one = np_draw(SEED, COUNTER, i, 0, 2) == 1
                        want = T._get_action(0, dc, False) if one else T._get_action(dr, 0, False)
                    else:
                        want = T._get_action(dr, dc, False)
                    assert (act[i], drew[i]) == (want, dr == dc), (g, i)
            assert len(set(act[:16].tolist())) == 2 and len(set(act[16:32].tolist())) == 2      # both outcomes occur
        return "gather", view, feat, params(h, w, {0: 5}), expect, True
    return build


def case_rush_first_attackable():
    view, feat = blank(8, 13, 13)
    o = cells_of(view)
    o[:, 3, 3], o[:, 70, 1], o[:, 150, 3] = 1.0, 0.7, 1.0
    o[:, 5, 3] = 0.5                       # (not > 0.5)

    def expect(act, drew):
        assert not drew.any() and (act == 13 + 4).all()
    return "rush", view, feat, params(13, 13, {5: 2, 70: 4, 150: 9}), expect, True


FRONTS = [0.0, 1.0, 0.5, np.nan, 0.49, 1.49, 1.5, np.inf, -np.inf]
FRONT_FREE = [True, False, False, True, True, False, True, True, True]


def case_rush_forward():
    """an unattackable hit and each value in the cell in front; then the same without any hit: always a draw"""
    k = len(FRONTS)
    view, feat = blank(2 * k, 13, 13)
    view[:k, 0, 3, 3] = 1.0
    view[:, 12, 6, 0] = FRONTS + FRONTS

    def expect(act, drew):
        assert drew.tolist() == [0 if f else 1 for f in FRONT_FREE] + [1] * k
        assert (act[drew == 0] == 0).all()
        assert act[drew == 1].tolist() == np_draw(SEED, COUNTER, np.nonzero(drew)[0], 0, 13).tolist()
    return "rush", view, feat, params(13, 13, {100: 1}), expect, True


def case_rush_feature():
    """the threshold test `!(f < threshold)` on the i-th float of the FLATTENED feature array"""
    values = [np.nan, np.inf, -np.inf, 100.0, np.nextafter(np.float32(100.0), np.float32(0.0)), np.nextafter(np.float32(100.0), np.float32(200.0))]
    view, _ = blank(len(values), 13, 13)
    cells_of(view)[:, 70, 3] = 1.0
    feat = np.full((len(values), 3), 1000.0, dtype=np.float32)
    feat.reshape(-1)[:len(values)] = values

    def expect(act, drew):
        assert drew.tolist() == [1, 1, 0, 1, 0, 1]
        assert act[drew == 0].tolist() == [17, 17]
        assert act[drew == 1].tolist() == np_draw(SEED, COUNTER, np.nonzero(drew)[0], 0, 13).tolist()
    return "rush", view, feat, params(13, 13, {70: 4}), expect, True


def _case_runaway_small(h, w):
    def build():
        rs = np.random.RandomState(h * 31 + w)
        view, feat = blank(24, h, w)
        view[:, :, :, 3] = rs.choice(np.array([0.0, 0.0, 0.0, 0.5, 0.7, 1.0, np.nan], dtype=np.float32), size=(24, h, w))
        view[:, :, :, 2] = 1.0             # (another channel)
        return "runaway", view, feat, params(h, w), None, h >= 3 and w >= 3
    return build


CASES = {
    "gather_kth_rounds": case_gather_kth_rounds,
    "gather_kth_8x8": _case_gather_kth_shape(8, 8), "gather_kth_5x13": _case_gather_kth_shape(5, 13),
    "gather_kth_16x8": _case_gather_kth_shape(16, 8),
    "minimap_rounds": case_minimap_rounds, "mypos_last_wins": case_mypos_last_wins, "slot1": case_slot1,
    "diagonal_13x13": _case_diagonal(13, 13), "diagonal_7x9": _case_diagonal(7, 9),
    "rush_first_attackable": case_rush_first_attackable, "rush_forward": case_rush_forward, "rush_feature": case_rush_feature,
    "runaway_1x1": _case_runaway_small(1, 1), "runaway_2x5": _case_runaway_small(2, 5), "runaway_5x2": _case_runaway_small(5, 2),
    "runaway_3x3": _case_runaway_small(3, 3),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (kind, view, feature, params, expect, ref, restated (actions, drew)); built and restated once, shared by every test"""
    kind, view, feat, p, expect, ref = CASES[name]()
    want = np_actor(kind, view, feat, p, SEED, COUNTER)
    for a in (view, feat, p["v2a"]) + want:
        a.setflags(write=False)
    return kind, view, feat, p, expect, ref, want


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_hand_stated_answers(name):
    """np_actor against the answer written out by hand for the case, and against the existing restatement of the sets"""
    kind, view, feat, p, expect, ref, (act, drew) = case(name)
    if expect is not None:
        expect(act, drew)
    if front_is_finite(view):
        want_drew, sets = T.possible_sets(kind, view, feat, p)
        assert (drew.astype(bool) == want_drew).all()
        assert all(int(act[i]) in sets[i] for i in np.nonzero(drew)[0])


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("lg", LEGS)
def test_constructed_observations(lg, name):
    kind, view, feat, p, expect, ref, want = case(name)
    assert_device_equals_restatement(lg, kind, view, feat, p, want=want, ref=ref, what=name)


POISON = [np.nan, np.inf, -np.inf]


@functools.lru_cache(maxsize=None)
def poisoned(kind):
    rs = np.random.RandomState(40 + T.KIND[kind])
    view, feat, p = T.synthetic(kind, 40, 13, 13, 7, rs, density=0.05)
    if kind == "gather":                   # some agents without food in view, so that channels 3 and 6 decide
        view[::2, :, :, 4] = 0
    dirty = view.copy()
    agents = [0, 3, 4, 17, 38, 39]
    for i in agents:
        for ch in (1, 3, 4, 6, p["channel"]):
            for value in POISON:
                dirty[i, rs.randint(13), rs.randint(13), ch] = value
    dirty[3, :, :, 6], dirty[4, :, :, 3], dirty[17, :, :, 4], dirty[38, :, :, 1] = np.nan, np.nan, np.nan, np.nan
    clean_agents = np.setdiff1d(np.arange(40), agents)
    return view, dirty, feat, p, clean_agents, np_actor(kind, view, feat, p, SEED, COUNTER), np_actor(kind, dirty, feat, p, SEED, COUNTER)


@pytest.mark.parametrize("kind", ["runaway", "rush", "gather"])
@pytest.mark.parametrize("lg", LEGS)
def test_nan_and_inf_cells_only_move_their_own_agents(lg, kind):
    view, dirty, feat, p, clean_agents, want_clean, want_dirty = poisoned(kind)
    a0, d0 = assert_device_equals_restatement(lg, kind, view, feat, p, want=want_clean, ref=True, what="clean")
    a1, d1 = assert_device_equals_restatement(lg, kind, dirty, feat, p, want=want_dirty, what="poisoned")
    assert (a0[clean_agents] == a1[clean_agents]).all() and (d0[clean_agents] == d1[clean_agents]).all()
    want_drew, sets = T.possible_sets(kind, dirty, feat, p)
    assert (d1.astype(bool) == want_drew).all() and all(int(a1[i]) in sets[i] for i in np.nonzero(d1)[0])


# ---------------------------------------------------------------------------------------------- 4. call edges
@functools.lru_cache(maxsize=None)
def edge_inputs(kind, n):
    rs = np.random.RandomState(1000 * T.KIND[kind] + n)
    view, feat, p = T.synthetic(kind, n, 13, 13, 7, rs, density=0.03)
    return view, feat, p, np_actor(kind, view, feat, p, SEED, COUNTER)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 257])
@pytest.mark.parametrize("kind", ["runaway", "rush", "gather"])
@pytest.mark.parametrize("lg", LEGS)
def test_agent_counts_around_the_workgroup_tail(lg, kind, n):
    """`actions` and `drew` inside sentinel-filled allocations (Leg.run checks every byte outside [0, n)), at their start and one
    and four elements in; without `drew` the same actions"""
    view, feat, p, want = edge_inputs(kind, n)
    for lead in ((0, 1, 4) if n == 1 else (0, 4)):
        assert_device_equals_restatement(lg, kind, view, feat, p, want=want, what="n %d lead %d" % (n, lead), lead=lead)
    assert_device_equals_restatement(lg, kind, view, feat, p, want=want, what="n %d, drew NULL" % n, lead=1, with_drew=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["runaway", "rush", "gather"])
def test_another_stream_gives_the_same(kind):
    view, feat, p, want = edge_inputs(kind, 257)
    a0, d0 = assert_device_equals_restatement("gpu", kind, view, feat, p, want=want, lead=4)
    a1, d1 = assert_device_equals_restatement("gpu", kind, view, feat, p, want=want, lead=4, stream=True)
    assert (a0 == a1).all() and (d0 == d1).all()


@functools.lru_cache(maxsize=None)
def largest(kind, h, w):
    """n = 5 on a view of 16384 (16383) cells: what decides lies in the first and in the last round, view2attack at both ends"""
    last = h * w - 1
    view, feat = blank(5, h, w)
    o = cells_of(view)
    p = params(h, w, {0: 3, last: 8})
    if kind == "runaway":
        view[0, h - 1, w // 2 + 1, 3] = 1.0
        view[1, h - 3, w // 2 - 1, 3] = 0.7
        view[2, h - 4, w // 2, 3] = 1.0    # (a row too far)
        view[3, 0, 0, 3] = 1.0
    elif kind == "rush":
        o[0, last, 3] = 1.0                                  # the only hit is the last cell: attackable
        o[1, 0, 1], o[1, last, 3] = 1.0, 1.0                 # the first cell wins
        o[2, 1, 3] = 1.0                                     # cannot be attacked, the cell in front is free: 0
        feat.reshape(-1)[3] = 100.0                          # at the threshold: a draw
        o[4, 1, 3], o[4, last - 1, 3], view[4, h - 1, w // 2, 0] = 1.0, 1.0, 1.0     # hits that cannot be attacked, a wall: a draw
    else:
        o[0, [0, 70, last], 4] = 1.0                         # a pick among {first, last}; cell 70 cannot be attacked
        o[1, [0, 5000, last], 6], o[1, [2, last - 2], 3] = 0.7, 2.0      # a minimap pick seen from the last round's position
        o[2, last - 1, 4] = 1.0                              # the first food that cannot be attacked, in the last round
        o[4, last, 6], o[4, [0, last], 3] = 0.7, 2.0         # the one minimap cell is my position: slot 1
        # (agent 3 sees nothing: a draw over every action)
    return view, feat, p, np_actor(kind, view, feat, p, SEED, COUNTER)


@pytest.mark.parametrize("shape", [(128, 128), (127, 129)])
@pytest.mark.parametrize("kind", ["runaway", "rush", "gather"])
@pytest.mark.parametrize("lg", LEGS)
def test_largest_accepted_view(lg, kind, shape):
    h, w = shape
    view, feat, p, want = largest(kind, h, w)
    act, drew = want
    last = h * w - 1
    if kind == "runaway":
        assert act.tolist() == [4, 4, 5, 5, 5]
    elif kind == "rush":
        assert act[:3].tolist() == [13 + 8, 13 + 3, 0] and drew.tolist() == [0, 0, 0, 1, 1]
    else:
        k = np_draw(SEED, COUNTER, 0, 0, 2)
        assert act[0] == 13 + (3, 8)[k] and drew.tolist() == [1, 1, 0, 1, 1]
        cell = (0, 5000, last)[np_draw(SEED, COUNTER, 1, 0, 3)]
        assert act[1] == T._get_action(cell // w - (last - 2) // w, cell % w - (last - 2) % w, True)
        assert act[2] == T._get_action((last - 1) // w - h // 2, (last - 1) % w - w // 2, False) == 11
        assert act[3] == np_draw(SEED, COUNTER, 3, 0, 13) and act[4] == np_draw(SEED, COUNTER, 4, 1, 13)
    assert_device_equals_restatement(lg, kind, view, feat, p, want=want, what="%d x %d" % shape, lead=4)


@functools.lru_cache(maxsize=None)
def sweep():
    """30 seeded (H, W, C, n, density, seed, counter); C >= 7 holds gather's channels 3, 4, 6 and rush's 1 and 3"""
    rs = np.random.RandomState(20260)
    out = []
    for _ in range(30):
        h, w, c, n = rs.randint(1, 21), rs.randint(1, 21), rs.randint(7, 10), rs.randint(1, 41)
        density = float(rs.choice([0.01, 0.03, 0.08, 0.3]))
        seed = int(rs.randint(0, 2 ** 32, dtype=np.uint64)) << 32 | int(rs.randint(0, 2 ** 32, dtype=np.uint64))
        counter = int(rs.randint(0, 2 ** 32, dtype=np.uint64)) << 16 | int(rs.randint(0, 2 ** 16))
        kinds = []
        for kind in ("runaway", "rush", "gather"):
            view, feat, p = T.synthetic(kind, n, h, w, c, rs, density=density)
            kinds.append((kind, view, feat, p, np_actor(kind, view, feat, p, seed, counter)))
        out.append(((h, w, c, n, density, seed, counter), kinds))
    return out


@pytest.mark.parametrize("lg,count", [("emu", 30), pytest.param("gpu", 8, marks=pytest.mark.gpu)])
def test_random_sweep_of_shapes(lg, count):
    for (h, w, c, n, density, seed, counter), kinds in sweep()[:count]:
        for kind, view, feat, p, want in kinds:
            assert_device_equals_restatement(lg, kind, view, feat, p, want=want, seed=seed, counter=counter,
                                             ref=kind != "runaway" or (h >= 3 and w >= 3),
                                             what="%d x %d x %d, n %d, density %g, seed %#x, counter %#x" % (h, w, c, n, density, seed, counter))
            want_drew, sets = T.possible_sets(kind, view, feat, p)
            assert (want[1].astype(bool) == want_drew).all() and all(int(want[0][i]) in sets[i] for i in np.nonzero(want[1])[0])
