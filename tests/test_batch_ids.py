"""EnvBatch.agent_ids / env_info_many: the agent ids of every (environment, group) of a batch, written into packed int32 buffers at
EnvBatch.packed_offsets' rows by ONE launch (a launch per 192 non-empty entries).

Three battle worlds of different sizes (hp 4, damage 3: clear_dead shrinks them within a few cycles), one of them without its second side;
one entry of the pointer array is NULL.  Before every cycle the ids go into fresh guarded buffers (helpers.guarded): every segment equals
that world's get_agent_id, and every other word -- the stale rows behind a shrunken segment, the pad rows, the NULL entry's rows, both
guards -- still holds the sentinel.  Compared on integer words; no tolerance.

Two legs: `emu` runs the engine's .hip sources lane by lane on the CPU (the way tests/test_batch_cells.py reaches them), `gpu` (marked)
the product library.  An unknown name ends the process as env_get_info_device's does: asked of the emulated library, in a child."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import magent_amd

ROOT = H.ROOT
LEGS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
INFO_ITEMS = 192          # magent_amd/csrc/launch.h: the entries of one launch's table


def lib_of(leg):
    if leg == "emu":
        return H.ensure_emu()
    import torch
    assert torch.cuda.is_available()
    return H.HIP_LIB


def worlds():
    rnd = lambda g, n: (g, "random", {"n": n})
    over = {"small": {"hp": 4, "damage": 3}}
    return [H.Scenario("ids_a", "battle", 22, seed=801, place=[rnd(0, 63), rnd(1, 130)], steps=5, action_seed=11, over=over),
            H.Scenario("ids_b", "battle", 26, seed=802, place=[rnd(0, 301), rnd(1, 5)], steps=5, action_seed=12, over=over),
            H.Scenario("ids_c", "battle", 14, seed=803, place=[rnd(0, 41)], steps=5, action_seed=13, over=over)]      # (no second side)


def check_ids(batch, envs, handles, lib, off, tot, skip, nested, tag):
    """agent_ids into fresh guarded buffers; `skip`: the (environment, group) entries passed as NULL.  Every segment is get_agent_id's,
    every other word the sentinel."""
    dev = H.torch_device(envs[0], lib)
    NE, NG = len(envs), len(handles[0])
    bufs = [H.guarded((int(tot[g]),), "int32", dev, 0, int(tot[g]) + 1) for g in range(NG)]
    want = [[envs[e].get_agent_id(handles[e][g]) for g in range(NG)] for e in range(NE)]
    if nested:
        arg = [[None if (e, g) in skip else bufs[g].interior[int(off[e][g]):] for g in range(NG)] for e in range(NE)]
    else:
        arg = batch.packed_pointers([b.interior for b in bufs], off)
        for e, g in skip:
            arg[e * NG + g] = None
    H.device_sync(lib)
    batch.agent_ids(arg)
    H.device_sync(lib)
    for g, b in enumerate(bufs):
        w = H._guard_words(b)
        written = np.zeros(w.size, dtype=bool)
        for e in range(NE):
            n, o = len(want[e][g]), b.front + int(off[e][g])
            if (e, g) in skip or n == 0:
                continue
            assert np.array_equal(w[o:o + n].view(np.int32), np.asarray(want[e][g], dtype=np.int32)), "%s: world %d group %d" % (tag, e, g)
            written[o:o + n] = True
        bad = np.flatnonzero((w != b.sentinel) & ~written)
        assert bad.size == 0, "%s group %d: %d words outside the segments were written, first at word %d of the interior" % (tag, g, bad.size, bad[0] - b.front)
    return want


@pytest.mark.parametrize("leg", LEGS)
def test_every_segment_holds_its_worlds_ids(leg):
    import torch
    lib = lib_of(leg)
    scs = worlds()
    built = [sc.build(lib) for sc in scs]
    envs, handles = [b[0] for b in built], [b[1] for b in built]
    dev = H.torch_device(envs[0], lib)
    batch = magent_amd.EnvBatch(envs, n_threads=1)
    batch.order_streams = not H.is_emu(lib)
    nums0 = batch.nums_array().copy()
    assert nums0.tolist() == [[63, 130], [301, 5], [41, 0]]
    off, tot = batch.packed_offsets(nums0)
    assert off.tolist() == [[0, 0], [64, 132], [368, 140]] and tot.tolist() == [412, 140]
    rss = [np.random.RandomState(sc.action_seed) for sc in scs]
    seen = []
    for step in range(scs[0].steps):
        skip = {(1, 1)} if step % 2 == 0 else {(0, 0), (2, 1)}            # (a NULL entry; also one for the empty group)
        want = check_ids(batch, envs, handles, lib, off, tot, skip, nested=step == 1, tag="%s cycle %d" % (leg, step))
        seen.append([[len(w) for w in per] for per in want])
        acts = [[torch.from_numpy(sc.draw(rs, env, g, h, env.get_num(h))).to(dev) for g, h in enumerate(hs)] for sc, rs, env, hs in zip(scs, rss, envs, handles)]
        H.device_sync(lib)
        batch.cycle(None, None, acts, None)
        for env in envs:
            env.sync()
    assert seen[-1][0][0] < 63 and seen[-1][0][1] < 130 and seen[-1][1][1] < 5, seen   # (agents died: shrunken segments with stale rows behind them)
    ids = envs[0].get_agent_id(handles[0][1])
    assert not np.array_equal(ids, np.arange(len(ids)))                        # (the survivors' ids are no longer their rows)


def test_an_unknown_name_fails_loudly():
    """env_info_many(.., "hp", ..) of the emulated library in a child: the process ends with the engine's FATAL line naming the entry"""
    code = ("import ctypes, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import helpers as H, magent_amd\n"
            "env = H.gridworld('battle', lib=H.ensure_emu(), map_size=12)\n"
            "env.reset()\n"
            "batch = magent_amd.EnvBatch([env], n_threads=1)\n"
            "print('made', flush=True)\n"
            "batch._lib.env_info_many(batch._handles, 1, 2, b'hp', (ctypes.c_void_p * 2)(), None)\n"
            "print('returned')\n") % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=H.merge_env(os.environ, {"OMP_NUM_THREADS": "1"}), capture_output=True, text=True, timeout=900)
    assert p.returncode != 0 and "made" in p.stdout and "returned" not in p.stdout, (p.stdout, p.stderr[-800:])
    assert "magent-amd FATAL" in p.stderr and "env_info_many" in p.stderr and "hp" in p.stderr, p.stderr[-800:]


@pytest.mark.gpu
def test_more_entries_than_one_launch_takes():
    """110 tiny battle worlds x 2 groups = 220 entries, 215 of them non-empty and given: past the 192 entries of one launch's table"""
    lib = lib_of("gpu")
    envs = []
    for k in range(110):
        env = H.gridworld("battle", lib=lib, map_size=10)
        env.set_seed(50 + k)
        env.reset()
        hs = env.get_handles()
        env.add_agents(hs[0], "random", n=1 + k % 5)
        if k % 40 != 7:
            env.add_agents(hs[1], "random", n=1 + k % 3)
        envs.append(env)
    handles = [env.get_handles() for env in envs]
    batch = magent_amd.EnvBatch(envs, n_threads=1)
    nums = batch.nums_array().copy()
    off, tot = batch.packed_offsets(nums)
    skip = {(3, 0), (100, 1)}
    given = sum(1 for e in range(110) for g in range(2) if nums[e][g] > 0 and (e, g) not in skip)
    assert given > INFO_ITEMS
    check_ids(batch, envs, handles, lib, off, tot, skip, nested=False, tag="220 entries")
    for env in envs:
        env.close()
