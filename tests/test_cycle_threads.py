"""env_cycle_many's host-thread pool (magent_amd/csrc/cycle_pool.h) and env_step_many, against the oracle.

EnvBatch defaults to n_threads=8: the worlds of a call that join neither the two-launch batch nor the batched pipeline run their ordinary
cycles on the library's worker threads, on their own streams, while the batches' launches are in flight; with MAGENT_TUNE batch_cycle=0
every world does.  Here one EnvBatch holds worlds of all three routes, at least five of them alone in every cycle, and is cycled with 2 to
64 threads, with a width that changes from cycle to cycle, under the MAGENT_TUNE settings that move work onto the pool's threads, and
from two Python threads at once.  The expectation is always the oracle's: every scenario played alone through the reference call sequence
(batch_cells_driver.expectation), compared on integer words (helpers.assert_same), every buffer between sentinel guards that are checked
behind every cycle.  There is no tolerance in this file.  What the pool did is read from env_cycle_pool_stats and compared with what the
routes of the worlds, restated here from the oracle's group sizes (routes()), say it must have done -- exactly.

Two legs: `emu` runs the same .hip sources lane by lane on the CPU (emulated kernels serialise on the emulator's lock, the host code of
the worlds interleaves), `gpu` (marked) the product library.  MAGENT_TUNE is read once per process: non-default settings run in a child
under its own time limit; after a gpu child that ended by signal or at its time limit nothing more is started on the card from this file.

tests/native/pool_tsan.cc runs the pool class and tune() under ThreadSanitizer in a stand-alone program (no engine, no GPU).

Measured times of both legs: tests/README.md.
"""
import copy
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest

import batch_cells_driver as D
import helpers as H
import magent_amd

ROOT = H.ROOT
LEGS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
_GPU_DOWN = []
CYCLES = 12
WIDTHS = [8, 8, 2, 1, 5, 64, 3, 2, 8, 1, 4, 2]      # test_one_pool_serves_calls_of_changing_width: n_threads per cycle


def lib_of(leg):
    if leg == "emu":
        return H.ensure_emu()
    assert not _GPU_DOWN, "an earlier gpu leg of this file ended by signal or at its time limit (%s): nothing more is started on the card" % _GPU_DOWN[0]
    import torch
    assert torch.cuda.is_available()
    return H.HIP_LIB


# ---------------------------------------------------------------------------------------------------- the batch
def resized(sc, steps):
    sc = copy.deepcopy(sc)
    sc.steps = steps
    return sc


def pool_batch(cycles=CYCLES):
    """eight two-group worlds of one EnvBatch -> (scenarios, cell flags, misalign).
      pipe_a, pipe_b   : plain battle worlds beyond the one-launch step: the batched pipeline, in flight while the pool works
      battle_partial   : 400 agents, one side observed: the two-launch cycle
      gather           : both groups observed through different windows under minimap_mode: alone
      battle_food      : food_mode: neither the one-launch step nor the pipeline of plain games takes it: alone
      gather_turn      : gather's two windows again, under turn_mode: alone
      battle_63_65, battle_255_256 (helpers.buffer_worlds): every view buffer one float behind a 16-byte boundary: alone
    pipe_a and gather are given bf16 cells (7 channels), the others float32 (battle_food has 8 channels; a misaligned cell view is fatal)"""
    S, P, W = H.scenarios(), {sc.name: sc for sc in H.cycle_partial_scenarios()}, H.buffer_worlds()
    a, b = H.pipe_batch_scenarios()[:2]
    scs = [a, b, P["battle_partial"], S["gather"], S["battle_food"], S["gather_turn"], W["battle_63_65"], W["battle_255_256"]]
    assert [sc.name for sc in scs] == ["pipe_a", "pipe_b", "battle_partial", "gather", "battle_food", "gather_turn", "battle_63_65", "battle_255_256"]
    flags = [[True, True], [False, False], [False, False], [True, True], [False, False], [False, False], [False, False], [False, False]]
    return [resized(sc, cycles) for sc in scs], flags, [None, None, None, None, None, None, 1, 1]


def routes(scs, trajs, misalign, tune):
    """per cycle and world of one env_cycle_many call: "pipe" (the batched pipeline), "pair" (the two-launch batch) or "alone" (handed to the
    host threads) -- Env::cycle_many restated for battle and gather worlds whose groups all fit the batch's one-launch step (<= 16384 agents),
    from the oracle's group sizes at the start of every cycle (`trajs`, the id%d arrays) and this process's MAGENT_TUNE (`tune`, a dict):
      never batched   : a misaligned view of an observed group, two observed non-empty groups that look through different windows under
                        minimap_mode, host_shuffle=1, an empty world; food_mode (the one-launch step and the pipeline both refuse it)
      the pipeline    : plain worlds (no turn_mode / food_mode) of >= 1537 agents -- of any size when attack_pairs is fixed, which also switches
                        the one-launch step off -- when at least two worlds of the call qualify and batch_pipe is not 0; a single qualifier takes
                        the two-launch cycle up to 1536 agents and goes alone beyond
      two launches    : every other world, unless attack_pairs is fixed
    MAGENT_TUNE batch_cycle=0: no batch at all, every world is an item of the pool."""
    fixed, pipe_on = "attack_pairs" in tune, tune.get("batch_pipe", 1) != 0
    out = []
    for c in range(max(sc.steps for sc in scs)):
        kinds, cand = [], []
        for k, (sc, traj) in enumerate(zip(scs, trajs)):
            cfg = sc.config()
            NG = len(cfg.groups)
            nums = [len(traj[c]["id%d" % g]) if c < len(traj) else 0 for g in range(NG)]
            seen = [g for g in sc.groups_at(sc.observed, c, NG) if nums[g] > 0 and c % sc.obs_every == 0]
            win = [(cfg.agent_type_dict[cfg.groups[g]]["view_range"].radius, cfg.agent_type_dict[cfg.groups[g]]["view_range"].angle) for g in range(NG)]
            two_windows = bool(cfg.config_dict.get("minimap_mode")) and len(set(win[g] for g in seen)) > 1
            food, turn = bool(sc.settings.get("food_mode")), bool(sc.settings.get("turn_mode"))
            assert sum(nums) <= 16384 and sc.game in ("battle", "gather")
            never = (misalign[k] and seen) or two_windows or tune.get("host_shuffle", 0) == 1 or sum(nums) == 0
            solo = not never and not food and not fixed
            pipe = not never and not food and not turn and pipe_on and (fixed or sum(nums) >= 1537)
            kinds.append(("pipe" if pipe else "pair" if solo else "alone", solo, sum(nums)))
            cand.append(pipe)
        if sum(cand) == 1:
            k = cand.index(True)
            kinds[k] = ("pair" if kinds[k][1] and kinds[k][2] <= 1536 else "alone",)
        out.append(["alone" if tune.get("batch_cycle", 1) == 0 else kd[0] for kd in kinds])
    return out


def check_pool_batch(lib, n_threads, cycles=CYCLES, what=""):
    """pool_batch() on engine library `lib` under this process's MAGENT_TUNE with `n_threads` (a number, or a function cycle -> number):
    every trajectory the oracle's; per cycle and world, what the engine's own counters say about the route taken -- pipeline_stats()[6] moves
    for "pipe" worlds only (and is helpers.expected_pipe_cycles' for pipe_a and pipe_b), a world that goes alone launches one render per
    observed group and a batched one none of its own --; and the pool's counters: one round per cycle with two or more worlds alone and
    n_threads >= 2, as many items as worlds alone in those cycles, never more threads in a round than asked for or than items.
    Returns (pool counter deltas, worlds alone per cycle)."""
    tune_text = os.environ.get("MAGENT_TUNE", "")
    tune = H.tune_settings()
    scs, flags, misalign = pool_batch(cycles)
    want = [D.expectation(sc) for sc in scs]
    for k in (3, 5):      # (gather, gather_turn go alone for their two windows: both groups stay non-empty)
        assert len(want[k]) == cycles and all(len(rec["id0"]) > 0 and len(rec["id1"]) > 0 for rec in want[k]), scs[k].name
    route = routes(scs, want, misalign, tune)
    alone = [r.count("alone") for r in route]
    assert min(alone) >= 4 and all(r[3] == r[4] == r[5] == "alone" for r in route), route      # (three of them for reasons other than alignment)
    width = [n_threads(c) if callable(n_threads) else n_threads for c in range(cycles)]
    log, before = {}, D.pool_stats(lib)
    D.check(scs, lib, flags, "host threads %s, MAGENT_TUNE=%s%s" % (sorted(set(width)), tune_text, what), log=log, n_threads=n_threads, misalign=misalign)
    assert len(log["piped"]) == cycles
    # ---- the routes, from the engine's own counters
    NE = len(scs)
    for c in range(cycles):
        piped_before = log["piped"][c - 1] if c else [0] * NE
        for k in range(NE):
            tag = (scs[k].name, "cycle", c, route[c][k], "renders", log["renders"][c], "observed", log["observed"][c], "piped", log["piped"][c])
            assert log["piped"][c][k] - piped_before[k] == (route[c][k] == "pipe"), tag
            if tune.get("batch_cycle", 1) == 0:      # (Env::cycle itself takes the two-launch form where it can: one render launch)
                assert log["renders"][c][k] in (log["observed"][c][k], min(1, log["observed"][c][k])), tag
            else:
                assert log["renders"][c][k] == (log["observed"][c][k] if route[c][k] == "alone" else 0), tag
    if tune.get("batch_cycle", 1) != 0:
        # (expected_pipe_cycles knows the defaults and attack_pairs; under batch_pipe=0 and host_shuffle=1 nothing goes through the pipeline)
        expect = [[0, 0, 0]] * cycles if tune.get("batch_pipe", 1) == 0 or tune.get("host_shuffle", 0) == 1 else H.expected_pipe_cycles(scs[:3], want[:3], tune_text)
        assert [p[:3] for p in log["piped"]] == expect, (log["piped"], expect)
        assert all(p[3:] == [0] * 5 for p in log["piped"]), log["piped"]
    # ---- the pool
    rounds = [c for c in range(cycles) if alone[c] >= 2 and width[c] >= 2]
    stats = [before] + log["pool"]
    for c in range(cycles):
        d = [b - a for a, b in zip(stats[c], stats[c + 1])]
        on = c in rounds
        assert d[0] == (1 if on else 0) and d[1] == (alone[c] if on else 0) and 0 <= d[2] <= d[1], ("cycle", c, "pool", d, "alone", alone[c], "n_threads", width[c])
        # the most threads of one round, process-wide: a cycle raises it to no more than it was asked for, nor than it had items
        assert stats[c + 1][3] <= max(stats[c][3], min(width[c], alone[c]) if on else 0), ("cycle", c, stats[c], stats[c + 1], width[c], alone[c])
    total = [b - a for a, b in zip(before, log["pool"][-1])]
    assert total[0] == len(rounds) and total[1] == sum(alone[c] for c in rounds), (total, rounds, alone)
    return total, alone


CHILD = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
         "import helpers as H, test_cycle_threads as T\n"
         "total, alone = T.check_pool_batch(H.ensure_emu() if sys.argv[1] == 'emu' else H.HIP_LIB, 8)\n"
         "assert total[2] > 0, total\n"
         "print('ok', total, alone)\n") % (ROOT, os.path.join(ROOT, "tests"))


def run_child(leg, tune, timeout):
    lib_of(leg)
    env = H.merge_env(os.environ, {"OMP_NUM_THREADS": "1"}, {"MAGENT_TUNE": tune})
    try:
        p = subprocess.run([sys.executable, "-c", CHILD, leg], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        if leg == "gpu":
            _GPU_DOWN.append("%s: no end within %d s" % (tune, timeout))
        raise AssertionError("%s %s: the child did not end within %d s: %s" % (leg, tune, timeout, str(e.stderr)[-2000:]))
    if leg == "gpu" and (p.returncode < 0 or p.returncode in (124, 134, 137, 139)):
        _GPU_DOWN.append("%s: exit code %d" % (tune, p.returncode))
    assert p.returncode == 0 and p.stdout.startswith("ok"), (leg, tune, p.returncode, p.stdout[-1500:] + p.stderr[-3000:])
    return p.stdout


# ---------------------------------------------------------------------------------------------------- a. the pool, 2 to 64 threads
@pytest.mark.parametrize("n_threads", [2, 3, 8, 64])
@pytest.mark.parametrize("leg", LEGS)
def test_worlds_that_go_alone_run_on_the_pool(leg, n_threads):
    """pool_batch() with n_threads host threads: five worlds alone in every cycle (six once pipe_a has shrunk below 1537 agents and pipe_b is
    the pipeline's only candidate), the pipeline's and the two-launch batch's launches in flight meanwhile.  check_pool_batch's assertions;
    and some item was run by a worker thread -- an item is a whole cycle with host waits on the device in it, so a worker that never gets
    one in all these rounds was never woken"""
    total, alone = check_pool_batch(lib_of(leg), n_threads)
    assert total[0] == CYCLES and total[1] == sum(alone) >= 5 * CYCLES, (total, alone)
    assert total[2] > 0, total


# ---------------------------------------------------------------------------------------------------- b. one pool, changing width
@pytest.mark.parametrize("leg", LEGS)
def test_one_pool_serves_calls_of_changing_width(leg):
    """the same batch, n_threads 8, 8, 2, 1, 5, 64, 3, 2, 8, 1, 4, 2 from cycle to cycle: a pool grown to 7 workers (or more, by an earlier
    test) asked for 1, then 4, then more; n_threads <= 1 bypasses it.  One round per cycle with n_threads >= 2, none else"""
    n = len(WIDTHS)
    total, alone = check_pool_batch(lib_of(leg), lambda c: WIDTHS[c], cycles=n)
    assert n == 12 and total[0] == sum(w >= 2 for w in WIDTHS) == 10, total


# ---------------------------------------------------------------------------------------------------- c. the drivers' variants
@pytest.mark.parametrize("tune", ["batch_cycle=0", "batch_pipe=0", "attack_pairs=0", "host_shuffle=1"])
@pytest.mark.parametrize("leg", LEGS)
def test_driver_variants_on_the_pool(leg, tune):
    """the same batch with 8 threads in a child per MAGENT_TUNE setting:
      batch_cycle=0  : no batch: all eight worlds are items of the pool, the two-launch cycle (Env::cycle's thread_local item) and the
                       pipeline-sized worlds' own launches side by side on its threads
      batch_pipe=0   : no pipeline: the pipeline-sized worlds join the two-launch batch (they are within its 16384 agents)
      attack_pairs=0 : every plain step is finished by the host -- on the pool's threads for the worlds alone; the one-launch step is off,
                       so battle_partial joins the pipeline
      host_shuffle=1 : the host's generator work on the pool's threads: no world qualifies for a batch, all eight go alone"""
    out = run_child(leg, tune, 1500 if leg == "emu" else 90)
    if tune in ("batch_cycle=0", "host_shuffle=1"):
        assert out.startswith("ok [%d, %d," % (CYCLES, 8 * CYCLES)), out


# ---------------------------------------------------------------------------------------------------- d. two callers
def caller_batches():
    """two disjoint sets of four small worlds, three and two of them alone"""
    S, P, W = H.scenarios(), {sc.name: sc for sc in H.cycle_partial_scenarios()}, H.buffer_worlds()
    one = [P["battle_partial"], S["gather"], S["battle_food"], W["battle_63_65"]]
    two = [P["battle_partial_late"], S["gather_turn"], W["battle_255_256"], S["battle_brawl"]]
    return ([resized(sc, 10) for sc in one], [None, None, None, 1]), ([resized(sc, 10) for sc in two], [None, None, 1, None])


@pytest.mark.parametrize("leg", LEGS)
def test_two_callers_cycle_disjoint_batches(leg):
    """two Python threads, an EnvBatch(n_threads=4) of four worlds each, released together in front of their first cycle (ctypes drops the
    GIL for the call: the pool's round_mutex is what keeps the two calls' rounds apart), 10 cycles each: both batches' trajectories the
    oracle's, and the pool counted both callers' rounds and items"""
    lib = lib_of(leg)
    batches = caller_batches()
    tune = H.tune_settings()
    expected, built = [], threading.Lock()
    for scs, misalign in batches:
        want = [D.expectation(sc) for sc in scs]
        alone = [r.count("alone") for r in routes(scs, want, misalign, tune)]
        assert len(alone) == 10 and min(alone) >= 2, alone
        expected.append(alone)
        for sc in scs:      # (the worlds are set up one caller at a time: the contract is about the cycles)
            sc.build = lambda lib_, sc=sc: _locked(built, H.Scenario.build, sc, lib_)
    gate, failed = threading.Barrier(2, timeout=600), []

    def caller(k):
        scs, misalign = batches[k]
        try:
            D.check(scs, lib, [[False, False]] * 4, "caller %d of two, %s" % (k, leg), n_threads=lambda c: gate.wait() * 0 + 4 if c == 0 else 4, misalign=misalign)
        except BaseException as e:      # noqa: B902 (reported by the test's own thread)
            gate.abort()
            failed.append((k, e))

    before = D.pool_stats(lib)
    threads = [threading.Thread(target=caller, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failed, failed
    d = [b - a for a, b in zip(before, D.pool_stats(lib))]
    assert d[0] == 20 and d[1] == sum(expected[0]) + sum(expected[1]) and 0 <= d[2] <= d[1], (d, expected)


def _locked(lock, fn, *args):
    with lock:
        return fn(*args)


# ---------------------------------------------------------------------------------------------------- e. env_step_many
STEP_MANY = ["battle_small_dense", "battle60", "bodies", "arrange_goals_move"]


def play_step_many(scs, lib):
    """helpers.run's host-ABI call sequence for several worlds at once, env.step() replaced by ONE magent_amd.step_many over all of them"""
    built = [sc.build(lib) for sc in scs]
    envs, handles = [b[0] for b in built], [b[1] for b in built]
    rss = [np.random.RandomState(sc.action_seed) for sc in scs]
    out = [[] for _ in scs]
    for step in range(max(sc.steps for sc in scs)):
        recs = []
        for sc, env, hs, rs in zip(scs, envs, handles, rss):
            rec = {}
            acting = sc.acting if sc.acting is not None else list(range(len(hs)))
            sc.apply_events(env, step)
            for g, h in enumerate(hs):
                n = env.get_num(h)
                if step % sc.obs_every == 0 and n > 0:
                    view, feat = env.get_observation(h)
                    rec["view%d" % g], rec["feat%d" % g] = view.copy(), feat.copy()
                rec["id%d" % g] = env.get_agent_id(h)
                if g in acting:
                    env.set_action(h, sc.draw(rs, env, g, h, n))
            recs.append(rec)
        dones = magent_amd.step_many(envs)
        for k, (sc, env, hs, rec) in enumerate(zip(scs, envs, handles, recs)):
            rec["done"] = np.array([dones[k]], dtype=np.int32)
            for g, h in enumerate(hs):
                rec["reward%d" % g] = env.get_reward(h)
                rec["alive%d" % g] = env.get_alive(h).astype(np.uint8)
                rec["pos%d" % g] = env.get_pos(h)
                rec["num%d" % g] = np.array([env.get_num(h)], dtype=np.int32)
            if step % 7 == 3:
                rec["global_minimap"] = env.get_global_minimap(5, 6).copy()
            if (step + 1) % sc.clear_every == 0:
                env.clear_dead()
            out[k].append(rec)
    return out


@pytest.mark.parametrize("leg", LEGS)
def test_step_many_equals_the_call_sequence(leg):
    """four worlds of four step drivers -- battle_small_dense (one launch), battle60 (the plain pipeline), bodies (the generic phases),
    arrange_goals_move (the literal loop on one lane) -- stepped by ONE env_step_many per step inside the reference call sequence, 12 steps:
    every output of every step equals the oracle's, each world played alone with env_step"""
    lib = lib_of(leg)
    scs = [resized(H.scenarios()[name], min(H.scenarios()[name].steps, 12)) for name in STEP_MANY]
    assert all(sc.steps == 12 for sc in scs)
    want = [H.run(sc, H.ensure_oracle()) for sc in scs]
    assert all(len(w) == 12 for w in want) and [len(sc.config().groups) for sc in scs] == [2, 2, 3, 3]
    got = play_step_many(scs, lib)
    for sc, w, g in zip(scs, want, got):
        H.assert_same(w, g, "%s (step_many, %s)" % (sc.name, leg))


# ---------------------------------------------------------------------------------------------------- the pool and tune() under ThreadSanitizer
PROBE = "#include <thread>\nint x;\nint main() { std::thread t([] { x = 1; }); t.join(); return x - 1; }\n"


def test_the_pool_and_tune_are_clean_under_thread_sanitizer(tmp_path):
    """tests/native/pool_tsan.cc, built here with -fsanitize=thread: 3,000 rounds of changing width and item count from two callers on one
    pool, a grown pool asked for fewer threads, tune() from eight threads at once.  Exit code 0 and no report (a report ends the program
    with 66).  Skipped only where a three-line program does not link with the flag.  (The emulated engine is not built this way: its fibers
    switch stacks in hand-written assembly, which ThreadSanitizer does not follow.)"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    flags = ["-fsanitize=thread", "-O1", "-g", "-pthread", "-std=c++17"]
    (tmp_path / "probe.cc").write_text(PROBE)
    probe = subprocess.run([cxx] + flags + [str(tmp_path / "probe.cc"), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("%s does not link with -fsanitize=thread: %s" % (cxx, probe.stderr[-300:]))
    exe = str(tmp_path / "pool_tsan")
    subprocess.run([cxx] + flags + ["-I", os.path.join(ROOT, "magent_amd", "csrc"), os.path.join(ROOT, "tests", "native", "pool_tsan.cc"), "-o", exe], check=True)
    env = H.merge_env(os.environ, {"TSAN_OPTIONS": "halt_on_error=1:exitcode=66"})
    env.pop("MAGENT_TUNE", None)
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "pool_tsan ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-4000:])
