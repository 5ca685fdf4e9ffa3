"""DeviceEpisodesBuffer.last_rows / returns (magent_amd/csrc/replay.hip: k_replay_returns, C entry replay_returns) against the host loop
they replace: helpers.np_discounted_returns per slot over the episodes of test_replay_kernels' numpy restatement, cast once to float32.
Every comparison is on bits.

The arithmetic is the contract: keep = keep * gamma + r in IEEE double, product and sum rounded separately.  A fused multiply-add rounds
once and gives other bits -- but only on inputs built for it: on random rewards the two doubles differ in their last place, and the cast
to float32 hides that except at a float32 rounding boundary.  DISCRIMINATING below is such an input, by construction:
    boot = 1 + 2^-23, gamma = 1 - 2^-48, r = -1.  boot * gamma = 1 + 2^-23 - 2^-48 - 2^-71 exactly; a double keeps 1 + 2^-23 - 2^-48.
    unfused: (1 + 2^-23 - 2^-48) - 1 = 2^-23 - 2^-48 = 25 one-bits from 2^-24 down: halfway between two float32, ties to even: 2^-23.
    fused:   2^-23 - 2^-48 - 2^-71, exact in a double, is below the halfway point: 2^-23 - 2^-47.
fused_returns restates the fused recurrence with exact rationals (float(Fraction) rounds correctly); the tests assert that it differs
from the oracle on their inputs before the bit equality is taken to say anything about contraction.

Two legs, as in test_replay_kernels: `emu` runs the kernel lane by lane on the CPU, `gpu` (marked) the product library.
tests/native/replay_returns_asan.cc drives the entry in a stand-alone program under AddressSanitizer and UBSan (CPU only)."""
import os
import subprocess
import sys
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

import helpers as H
from test_replay_kernels import Restated, bits, guard, host_view, leg_of, make, play, row_data, synthetic_round

LEGS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
VIEWS = ["f32", "cells"]
DISCRIMINATING = (np.float32(1 + 2.0 ** -23), 1 - 2.0 ** -48, np.float32(-1.0))       # (boot, gamma, reward)


def fused_returns(rewards, bootstrap, gamma):
    """np_discounted_returns with keep * gamma + r rounded ONCE to double: what a contracted multiply-add computes"""
    out, keep = np.zeros(len(rewards)), float(bootstrap)
    for i in reversed(range(len(rewards))):
        keep = float(Fraction(keep) * Fraction(float(gamma)) + Fraction(float(rewards[i])))
        out[i] = keep
    return out


def oracle(want, boot, gamma, step=H.np_discounted_returns):
    """the returns of the restatement's episodes in packed order, float32"""
    out = [step(np.array([tr[3] for tr in ep], dtype=np.float32), boot[s], gamma) for s, ep in enumerate(want.episodes) if ep]
    return np.concatenate(out).astype(np.float32)


def with_rewards(calls, fn):
    """the calls with fn(call number, rows) -> float32 rewards in place of the round's own (which are all positive)"""
    return [c[:5] + (torch.from_numpy(np.asarray(fn(t, len(c[0])), dtype=np.float32)),) for t, c in enumerate(calls)]


def signed_rewards(seed):
    rs = np.random.RandomState(seed)
    return lambda t, n: rs.randn(n) * 2


def signed_boot(n, dev, seed=17):
    boot = (np.random.RandomState(seed).randn(n) * 3).astype(np.float32)
    return boot, torch.from_numpy(boot).to(dev)


def test_the_discriminating_input_tells_a_fused_multiply_add_from_the_contract():
    """on the CPU, in numpy: the construction of the module's docstring"""
    boot, gamma, r = DISCRIMINATING
    unfused, fused = H.np_discounted_returns([r], boot, gamma), fused_returns([r], boot, gamma)
    assert unfused[0] == 2.0 ** -23 - 2.0 ** -48 and fused[0] == 2.0 ** -23 - 2.0 ** -48 - 2.0 ** -71
    assert np.float32(unfused[0]) == np.float32(2.0 ** -23) and np.float32(fused[0]) == np.float32(2.0 ** -23 - 2.0 ** -47)


@pytest.mark.parametrize("gamma", [0.99, 0.0, 1.0])
@pytest.mark.parametrize("kind", VIEWS)
@pytest.mark.parametrize("leg", LEGS)
def test_returns_equal_the_host_loop_on_bits(leg, kind, gamma):
    """the synthetic round (episodes of length 1, episodes as long as the round, agents that die after their first call, agents first seen
    in call 3), rewards and bootstrap values of both signs"""
    calls, after = synthetic_round(kind)
    calls = with_rewards(calls, signed_rewards(3))
    rec, want = make(leg, kind, 64, 400), Restated(64, 400)
    play(rec, want, calls, after, kind)
    lens = [len(e) for e in want.episodes]
    assert 1 in lens and len(calls) in lens and len(lens) == 41
    boot, boot_dev = signed_boot(len(lens), rec.device)
    assert rec.tracked == len(lens)
    got = rec.returns(boot_dev, gamma)
    exp = oracle(want, boot, gamma)
    assert got.dtype == torch.float32 and tuple(got.shape) == exp.shape == (want.transitions,) and got.device == rec.device
    assert np.array_equal(bits(got), bits(exp))
    assert (exp < 0).any() and (exp > 0).any()
    if gamma == 0.0:
        assert np.array_equal(bits(exp), bits(rec.packed()[3]))          # (the rewards themselves: the bootstrap is multiplied away)
    # last_rows: the slots with transitions and each one's last packed row
    slots, rows = rec.last_rows()
    assert slots.dtype == rows.dtype == torch.int64 and slots.device == rows.device == rec.device
    assert slots.cpu().tolist() == [s for s, m in enumerate(lens) if m > 0]
    assert rows.cpu().tolist() == (np.cumsum([m for m in lens if m > 0]) - 1).tolist()


@pytest.mark.parametrize("leg", LEGS)
def test_a_fused_multiply_add_would_be_seen(leg):
    """every reward -1, every bootstrap value 1 + 2^-23, gamma 1 - 2^-48: the last return of EVERY episode is the halfway case, where
    a contracted multiply-add gives the float32 below the contract's"""
    boot1, gamma, r = DISCRIMINATING
    calls, after = synthetic_round("f32")
    rec, want = make(leg, "f32", 64, 400), Restated(64, 400)
    play(rec, want, with_rewards(calls, lambda t, n: np.full(n, r)), after, "f32")
    n_slots = len(want.episodes)
    boot = np.full(n_slots, boot1, dtype=np.float32)
    exp, fused = oracle(want, boot, gamma), oracle(want, boot, gamma, fused_returns)
    differ = bits(exp) != bits(fused)
    ends = np.cumsum([len(e) for e in want.episodes if e]) - 1
    assert differ[ends].all(), "the input does not tell the two roundings apart"
    got = rec.returns(torch.from_numpy(boot).to(rec.device), gamma)
    assert np.array_equal(bits(got), bits(exp)), "%d of %d returns differ; %d equal the fused restatement's where it differs" % (
        int((bits(got) != bits(exp)).sum()), len(exp), int((bits(got) == bits(fused))[differ].sum()))


@pytest.mark.parametrize("leg", LEGS)
def test_wide(leg):
    """1100 agents in a capacity of 1500 (no multiple of a workgroup's slots, tracked < capacity), three calls: 500 episodes of three
    transitions, 400 of two, 200 of one -- more slots than one scan block and than one workgroup of the returns"""
    n = 1100
    ids = np.random.RandomState(3).permutation(5000)[:n].astype(np.int32)
    rs = np.random.RandomState(8)
    calls = [(ids[:k].copy(), None) + row_data(2000 * t + np.arange(k), "cells")[:3] + (torch.from_numpy((rs.randn(k) * 2).astype(np.float32)),)
             for t, k in enumerate((n, 900, 500))]
    rec, want = make(leg, "cells", 1500, 3000), Restated(1500, 3000)
    play(rec, want, calls, (ids[:250].copy(), None), "cells", plain=True)
    assert rec.tracked == n and sorted(set(len(e) for e in want.episodes)) == [1, 2, 3]
    boot, boot_dev = signed_boot(n, rec.device)
    assert np.array_equal(bits(rec.returns(boot_dev, 0.99)), bits(oracle(want, boot, 0.99)))
    slots, rows = rec.last_rows()
    assert slots.cpu().tolist() == list(range(n)) and rows.cpu().tolist() == (np.cumsum([len(e) for e in want.episodes]) - 1).tolist()


@pytest.mark.parametrize("leg", LEGS)
def test_long_episodes_through_the_c_entry(leg):
    """a layout written into the recorder's state by hand -- 128 slots of 70 transitions (8960 rows: more than a workgroup stages), 72 of
    length 3 with every fifth one empty, the rest of the capacity untracked -- and replay_returns called as the recorder calls it, into
    an output LONGER than n_trans between sentinels: the rows behind n_trans keep their fill, the guard words their values"""
    rec = make(leg, "f32", 300, 12000)
    lib, dev = rec._lib, rec.device
    lens = np.array([70] * 128 + [0 if s % 5 == 0 else 3 for s in range(72)], dtype=np.int32)
    base = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n_slots, n = len(lens), int(base[-1])
    assert n > 8192 and n_slots < rec.capacity
    rec._len[:n_slots] = torch.from_numpy(lens).to(dev)
    base_dev = torch.full((rec.capacity,), n, dtype=torch.int32, device=dev)
    base_dev[:n_slots] = torch.from_numpy(base[:-1]).to(dev)
    rs = np.random.RandomState(12)
    rew = (rs.randn(n) * 2).astype(np.float32)
    boot = (rs.randn(n_slots) * 3).astype(np.float32)
    boot[128::5] = np.nan                                        # (the empty slots' entries are not read)
    exp = np.concatenate([H.np_discounted_returns(rew[b:b + m], boot[s], 0.99) for s, (b, m) in enumerate(zip(base, lens)) if m]).astype(np.float32)
    ins = [guard(torch.from_numpy(a), dev) for a in (rew, boot)]
    for entry in (lib.replay_returns,) + ((lib.replay_returns_direct,) if hasattr(lib, "replay_returns_direct") else ()):
        out = guard(torch.full((n + 9,), -77.0), dev)
        assert entry(rec._st_ref, n_slots, n, base_dev.data_ptr(), ins[0].interior.data_ptr(), ins[1].interior.data_ptr(), 0.99,
                     out.interior.data_ptr(), rec._stream()) == 0
        got = out.interior.cpu().numpy()
        assert np.array_equal(bits(got[:n]), bits(exp)) and (got[n:] == -77.0).all() and not np.isnan(got).any()
        H.assert_guards_intact(out, "out_ret")
        for g in ins:
            assert np.array_equal(H._guard_words(g), g.before), "a caller-owned input was written"


@pytest.mark.parametrize("kind", VIEWS)
@pytest.mark.parametrize("leg", LEGS)
def test_slots_of_length_zero_write_nothing(leg, kind):
    """test_overflow's shapes: max_transitions takes calls 1-2 and not the third, whose admissions (the two agents first seen by it) stay
    at length 0.  NaN in their bootstrap entries changes nothing; the rest equals the oracle"""
    calls, after = synthetic_round(kind)
    calls = with_rewards(calls, signed_rewards(4))
    probe = Restated(64, 10 ** 6)
    for c in calls[:3]:
        two = probe.transitions
        probe.record_step(c[0], host_view(c[2], kind), c[3].numpy(), c[4].numpy(), c[5].numpy(), c[1])
    room = probe.transitions - 1
    rec, want = make(leg, kind, 64, room), Restated(64, room)
    play(rec, want, calls, after, kind)
    with pytest.warns(RuntimeWarning):
        assert rec.packed()[3].shape[0] == two
    empty = [s for s, e in enumerate(want.episodes) if not e]
    assert want.overflow and len(empty) == 2 and rec.tracked == len(want.episodes)
    boot, _ = signed_boot(rec.tracked, rec.device)
    exp = oracle(want, boot, 0.99)
    boot[empty] = np.nan
    got = rec.returns(torch.from_numpy(boot).to(rec.device), 0.99)
    assert tuple(got.shape) == (two,) and np.array_equal(bits(got), bits(exp))
    slots, rows = rec.last_rows()
    assert slots.cpu().tolist() == [s for s, e in enumerate(want.episodes) if e]
    assert rows.cpu().tolist() == (np.cumsum([len(e) for e in want.episodes if e]) - 1).tolist()


@pytest.mark.parametrize("leg", LEGS)
def test_nothing_recorded(leg):
    rec = make(leg, "f32", 13, 400)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert rec.last_rows() is None and rec.returns(torch.zeros(0, device=rec.device), 0.99) is None and rec.tracked == 0
    calls, after = synthetic_round("f32")
    want = Restated(13, 400)
    play(rec, want, calls[:2], after, "f32")
    assert rec.returns(torch.zeros(13, device=rec.device), 0.99) is not None
    rec.reset()
    assert rec.last_rows() is None and rec.returns(torch.zeros(13, device=rec.device), 0.99) is None


@pytest.mark.parametrize("leg", LEGS)
def test_refused_calls_write_nothing(leg):
    calls, after = synthetic_round("f32")
    rec, want = make(leg, "f32", 64, 400), Restated(64, 400)
    play(rec, want, calls, after, "f32")
    p, dev, lib = rec.packed(), rec.device, rec._lib
    t, n = rec.tracked, want.transitions
    boot = torch.ones(t, device=dev)
    out = guard(torch.full((n,), -77.0), dev)
    call = lambda n_slots, n_trans, boot_p, out_p: lib.replay_returns(rec._st_ref, n_slots, n_trans, rec._base.data_ptr(), p[3].data_ptr(), boot_p, 0.99,
                                                                      out_p, rec._stream())
    o = out.interior.data_ptr()
    assert call(t, n, None, o) == 1 and call(t, n, boot.data_ptr(), None) == 1 and call(rec.capacity + 1, n, boot.data_ptr(), o) == 1
    assert call(t, -1, boot.data_ptr(), o) == 1 and call(-1, n, boot.data_ptr(), o) == 1
    assert lib.replay_returns(rec._st_ref, t, n, None, p[3].data_ptr(), boot.data_ptr(), 0.99, o, rec._stream()) == 1
    assert lib.replay_returns(rec._st_ref, t, n, rec._base.data_ptr(), None, boot.data_ptr(), 0.99, o, rec._stream()) == 1
    assert call(0, n, boot.data_ptr(), o) == 0 and call(t, 0, boot.data_ptr(), o) == 0      # (nothing to do: nothing written)
    assert np.array_equal(H._guard_words(out), out.before)   # (the whole allocation: the fill and both guards)
    assert call(t, n, boot.data_ptr(), o) == 0
    assert np.array_equal(bits(out.interior), bits(oracle(want, np.ones(t, dtype=np.float32), 0.99)))
    H.assert_guards_intact(out, "out_ret")
    # the recorder's own checks, in record_step's style
    for bad in (boot.double(), boot[:-1], torch.ones(2 * t, device=dev)[::2], boot.cpu().numpy()):
        with pytest.raises(ValueError, match="bootstrap"):
            rec.returns(bad, 0.99)


def test_a_library_without_the_entry_says_rebuild():
    """an older library records and packs; returns() says what to do"""
    rec = make("emu", "f32", 64, 400)
    calls, after = synthetic_round("f32")
    play(rec, Restated(64, 400), calls[:2], after, "f32")

    class Old(object):
        has_replay_api, has_replay_returns = True, False

        def __getattr__(self, name):
            if name.startswith("replay_returns"):
                raise AttributeError(name)
            return getattr(rec_lib, name)
    rec_lib, rec._lib = rec._lib, Old()
    assert rec.packed() is not None and rec.last_rows() is not None
    with pytest.raises(RuntimeError, match="rebuild"):
        rec.returns(torch.zeros(rec.tracked), 0.99)
    from magent_amd import c_lib

    class Symbols(object):                                       # declare_replay on a library that has everything but the new entries
        pass
    old = Symbols()
    for name, _ in c_lib.REPLAY_ABI:
        setattr(old, name, getattr(rec_lib, name))
    c_lib.declare_replay(old)
    assert old.has_replay_api and not old.has_replay_returns
    assert rec_lib.has_replay_api and rec_lib.has_replay_returns


def test_the_entry_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/replay_returns_asan.cc with the emulated replay.hip, built here with -fsanitize=address,undefined: out_ret is a heap
    block of exactly n_trans floats, boot of exactly the tracked count.  Skipped only where a one-line program does not link with the
    flags."""
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
    exe = str(tmp_path / "replay_returns_asan")
    subprocess.run([emu_build.CXX] + flags + ["-I", emu_build.HERE, "-I", out, "-I", emu_build.CSRC, "-I", os.path.join(H.ROOT, "include"),
                                              os.path.join(out, "replay_emu.cc"), os.path.join(emu_build.HERE, "emu_runtime.cc"),
                                              os.path.join(H.ROOT, "tests", "native", "replay_returns_asan.cc"), "-o", exe, "-lpthread"], check=True)
    env = H.merge_env(os.environ, {"ASAN_OPTIONS": "halt_on_error=1:exitcode=66", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "replay_returns_asan ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-4000:])
