"""The driver of tests/test_batch_cells.py: scenarios of helpers.py cycled through magent_amd.EnvBatch with a view FORMAT per (environment,
group) -- helpers.run_cycle_batch cannot pass one -- and every caller-owned buffer between sentinel guards (helpers.guarded).

The expectation never comes from the engine: every scenario is played alone on the oracle through the reference call sequence
(helpers.run_cycle(sc, ensure_oracle(), fused=False)); where an entry is rendered as bf16 cells the expected words are
helpers.bf16_cells(view), the oracle's float32 view rounded on the bits.  Everything is compared on integer words (helpers.assert_same).
"""
import copy
import ctypes
import os

import numpy as np

import helpers as H
import magent_amd

_WANT = {}


def expectation(sc):
    """the oracle's trajectory of `sc`, played alone (once per process and scenario name, never changed)"""
    key = (sc.name, sc.steps)
    if key not in _WANT:
        _WANT[key] = H.run_cycle(sc, H.ensure_oracle(), fused=False)
    return _WANT[key]


def with_cells(want, flags):
    """the trajectory `want` with view%d of every group g with flags[g] replaced by cells%d = bf16_cells(view%d)"""
    out = []
    for rec in want:
        rec = dict(rec)
        for g, on in enumerate(flags):
            if on and "view%d" % g in rec:
                rec["cells%d" % g] = H.bf16_cells(rec.pop("view%d" % g))
        out.append(rec)
    return out


def _ptr_array(n_env, n_group, at):
    arr = (ctypes.c_void_p * (n_env * n_group))()
    for e in range(n_env):
        for g in range(n_group):
            arr[e * n_group + g] = at(e, g)
    return arr


def _segment(buf, off, n, tag):
    """rows off .. off + n of guarded buffer `buf` as host words [n, row]"""
    w = H._guard_words(buf)
    return w[buf.front + off * buf.row:buf.front + (off + n) * buf.row].reshape(n, buf.row)


def _typed(words, dtype, shape):
    return np.ascontiguousarray(words).view(dtype).reshape(shape)


def pool_stats(lib):
    """env_cycle_pool_stats of engine library `lib`: [rounds, items, items run by workers, most threads in one round] of this process"""
    from magent_amd import c_lib
    out = (ctypes.c_longlong * 4)()
    c_lib.load(lib).env_cycle_pool_stats(out)
    return list(out)


def play(scs, lib, flags, align_rows=None, log=None, n_threads=1, misalign=None):
    """`scs` in ONE EnvBatch on engine library `lib`, all their steps; flags[k][g]: environment k's group g is rendered as bf16 cells.
    align_rows None: every buffer an allocation of its own with one row of capacity to spare; a number: the packed layout -- per group ONE
    guarded buffer for each of views, feature rows, actions and rewards, laid out by EnvBatch.packed_offsets(nums, align_rows) and addressed
    through EnvBatch.packed_pointers; pad rows must come back holding the sentinel.  Guards are checked behind every cycle.
    log: a dict that receives per cycle "piped" (pipeline_stats()[6] of every environment), "renders" (render launches the profile counted
    in this cycle), "observed" (groups observed), "aligned" (Env::observed_groups_ok's alignment condition restated on the pointers built),
    "pool" (pool_stats(lib) behind the cycle).
    n_threads: the host threads env_cycle_many may use for the worlds that go alone -- a number, or a function cycle -> number.
    misalign (align_rows None only): per environment None or an offset in float elements; every view buffer of that environment starts that
    far behind a 16-byte boundary (helpers.guarded(offset_elems=...)), so Env::observed_groups_ok refuses the world and it goes alone,
    through the call sequence.  Not for an environment with a cell entry: the engine aborts on a misaligned cell view.
    Returns one trajectory per scenario, in helpers.run_cycle_batch's form with cells%d in place of view%d where flags say so."""
    import torch
    built = [sc.build(lib) for sc in scs]
    envs, handles = [b[0] for b in built], [b[1] for b in built]
    NE, NG = len(envs), len(handles[0])
    dev = H.torch_device(envs[0], lib)
    batch = magent_amd.EnvBatch(envs, n_threads=1)
    batch.order_streams = not H.is_emu(lib)
    assert misalign is None or (align_rows is None and not any(m and any(fl) for m, fl in zip(misalign, flags)))
    shift = [0] * NE if misalign is None else [int(m or 0) for m in misalign]
    rss = [np.random.RandomState(sc.action_seed) for sc in scs]
    out, live = [[] for _ in scs], [True] * NE
    for env in envs:
        env.profile_enable(1)
        env.profile_read("render")
    vspace = [[envs[k].get_view_space(h) for h in handles[k]] for k in range(NE)]
    fspace = [[envs[k].get_feature_space(h) for h in handles[k]] for k in range(NE)]
    vrow = lambda k, g: (vspace[k][g][:2] + (8,), "bfloat16") if flags[k][g] else (vspace[k][g], "float32")
    for step in range(max(sc.steps for sc in scs)):
        recs, nums, acts, observe, paid = [], [], [], [], []
        for k, (sc, env, hs) in enumerate(zip(scs, envs, handles)):
            assert sc.clear_every == 1
            acting = sc.acting if sc.acting is not None else list(range(NG))
            rec = {}
            sc.apply_events(env, step)
            n = [env.get_num(h) for h in hs]
            acts.append([sc.draw(rss[k], env, g, h, n[g]) if g in acting else None for g, h in enumerate(hs)])
            seen, pd = sc.groups_at(sc.observed, step, NG), sc.groups_at(sc.rewarded, step, NG)
            observe.append([step % sc.obs_every == 0 and n[g] > 0 and g in seen for g in range(NG)])
            paid.append([g in pd for g in range(NG)])
            if live[k] and step < sc.steps:
                sc.probe_before(env, hs, step, rec)
            for g, h in enumerate(hs):
                rec["id%d" % g] = env.get_agent_id(h)
            recs.append(rec); nums.append(n)
        # ---- the buffers
        if align_rows is None:
            off = np.zeros((NE, NG), dtype=np.int64)
            mk = lambda shape, dtype, on, n, shift=0: H.guarded((n,) + tuple(shape), dtype, dev, shift, n + 1) if on else None
            V = [[mk(*vrow(k, g), observe[k][g], nums[k][g], shift[k]) for g in range(NG)] for k in range(NE)]
            F = [[mk(fspace[k][g], "float32", observe[k][g], nums[k][g]) for g in range(NG)] for k in range(NE)]
            R = [[mk((), "float32", paid[k][g], nums[k][g]) for g in range(NG)] for k in range(NE)]
            A = [[None if a is None else torch.from_numpy(a).to(dev) for a in acts[k]] for k in range(NE)]
            at = lambda B: (lambda e, g: None if B[e][g] is None else B[e][g].ptr)
            pv, pf, pr = _ptr_array(NE, NG, at(V)), _ptr_array(NE, NG, at(F)), _ptr_array(NE, NG, at(R))
            pa = _ptr_array(NE, NG, lambda e, g: None if A[e][g] is None else A[e][g].data_ptr())
            buf = lambda B, e, g: B[e][g]
        else:       # one buffer per group and array (the formats are per group here: flags[0])
            off, totals = batch.packed_offsets(nums, align_rows)
            assert np.array_equal(off, np.cumsum(-(-np.array(nums) // align_rows) * align_rows, axis=0) - (-(-np.array(nums) // align_rows) * align_rows))
            one = lambda shape, dtype, g: H.guarded((int(totals[g]),) + tuple(shape), dtype, dev, 0, int(totals[g]) + 1) if totals[g] > 0 else None
            Vg = [one(*vrow(0, g), g) for g in range(NG)]
            Fg = [one(fspace[0][g], "float32", g) for g in range(NG)]
            Rg = [one((), "float32", g) for g in range(NG)]
            Ag = [one((), "int32", g) for g in range(NG)]
            for k in range(NE):
                for g in range(NG):
                    if acts[k][g] is not None and nums[k][g] > 0:
                        Ag[g].interior[int(off[k][g]):int(off[k][g]) + nums[k][g]] = torch.from_numpy(acts[k][g]).to(dev)
            base = lambda B: [None if b is None else b.interior for b in B]
            mask = lambda arr, on: _ptr_array(NE, NG, lambda e, g: arr[e * NG + g] if on(e, g) else None)
            pv = mask(batch.packed_pointers(base(Vg), off), lambda e, g: observe[e][g])
            pf = mask(batch.packed_pointers(base(Fg), off), lambda e, g: observe[e][g])
            pr = mask(batch.packed_pointers(base(Rg), off), lambda e, g: paid[e][g] and nums[e][g] > 0)
            pa = mask(batch.packed_pointers(base(Ag), off), lambda e, g: acts[e][g] is not None and nums[e][g] > 0)
            buf = lambda B, e, g: B[g]
            V, F, R = Vg, Fg, Rg
        cells = (ctypes.c_ubyte * (NE * NG))(*[1 if flags[e][g] and pv[e * NG + g] else 0 for e in range(NE) for g in range(NG)])
        H.device_sync(lib)
        for env in envs:      # (a probe step's observations through the ordinary calls are render launches too: counted from here)
            env.profile_read("render")
        batch.n_threads = n_threads(step) if callable(n_threads) else n_threads
        dones = batch.cycle(pv, pf, pa, pr, view_cells=cells if any(cells) else None)
        if log is not None:
            log.setdefault("pool", []).append(pool_stats(lib))
            log.setdefault("piped", []).append([env.pipeline_stats()[6] for env in envs])
            log.setdefault("swept", []).append([env.pipeline_stats()[7] for env in envs])
            log.setdefault("renders", []).append([env.profile_read("render")[0] for env in envs])
            log.setdefault("observed", []).append([sum(o) for o in observe])
            # Env::observed_groups_ok: every observed, non-empty group's view AND feature pointer 16-byte aligned
            log.setdefault("aligned", []).append([all((pv[e * NG + g] or 0) % 16 == 0 and (pf[e * NG + g] or 0) % 16 == 0 for g in range(NG) if observe[e][g])
                                                  for e in range(NE)])
        for env in envs:
            env.sync()
        H.device_sync(lib)
        # ---- what came back
        if align_rows is not None:      # every pad row, the rows past the total and both guards still hold the sentinel
            for what, B in (("view", Vg), ("feat", Fg), ("reward", Rg), ("actions", Ag)):
                for g, b in enumerate(B):
                    if b is None:
                        continue
                    w = H._guard_words(b)
                    written = np.zeros(w.size, dtype=bool)
                    for k in range(NE):
                        on = {"view": observe[k][g], "feat": observe[k][g], "reward": paid[k][g], "actions": acts[k][g] is not None}[what]
                        if on:
                            written[b.front + int(off[k][g]) * b.row:b.front + (int(off[k][g]) + nums[k][g]) * b.row] = True
                    bad = np.flatnonzero((w != b.sentinel) & ~written)
                    assert bad.size == 0, "step %d %s of group %d (align_rows %d): %d words outside the segments were written, first at word %d of the interior" % (
                        step, what, g, align_rows, bad.size, bad[0] - b.front)
        for k, (sc, env, hs) in enumerate(zip(scs, envs, handles)):
            rec = recs[k]
            for g in range(NG):
                n, o = nums[k][g], int(off[k][g])
                tag = "%s step %d group %d (n %d)" % (sc.name, step, g, n)
                if observe[k][g]:
                    if align_rows is None:
                        H.assert_guards_intact(V[k][g], tag + " view"); H.assert_guards_intact(F[k][g], tag + " feat")
                        # (no output holds the sentinel: a world whose cycle was never run is named here, behind that cycle)
                        H.assert_all_written(V[k][g], tag + " view"); H.assert_all_written(F[k][g], tag + " feat")
                    vw, fw = _segment(buf(V, k, g), o, n, tag), _segment(buf(F, k, g), o, n, tag)
                    if flags[k][g]:
                        rec["cells%d" % g] = _typed(vw, np.uint16, (n,) + vspace[k][g][:2] + (8,))
                    else:
                        rec["view%d" % g] = _typed(vw, np.float32, (n,) + vspace[k][g])
                    rec["feat%d" % g] = _typed(fw, np.float32, (n,) + fspace[k][g])
                if paid[k][g]:
                    if align_rows is None:
                        H.assert_guards_intact(R[k][g], tag + " reward")
                    if align_rows is None or n > 0:
                        rec["reward%d" % g] = _typed(_segment(buf(R, k, g), o, n, tag), np.float32, (n,))
                    else:
                        rec["reward%d" % g] = np.zeros(0, dtype=np.float32)
            rec["done"] = np.array([dones[k]], dtype=np.int32)
            for g, h in enumerate(hs):
                rec["num%d" % g] = np.array([env.get_num(h)], dtype=np.int32)
                rec["pos%d" % g] = env.get_pos(h)
                rec["alive%d" % g] = env.get_alive(h).astype(np.uint8)
                rec["ids_after%d" % g] = env.get_agent_id(h)
            if live[k] and step < sc.steps:
                sc.probe_after(env, hs, step, rec)
                out[k].append(rec)
                if all(env.get_num(h) == 0 for h in hs) and not any(e > step for e in sc.events):
                    live[k] = False
    return out


def check(scs, lib, flags, what, align_rows=None, log=None, n_threads=1, misalign=None):
    """play(...) against the oracle's trajectories, word for word"""
    got = play(scs, lib, flags, align_rows, log, n_threads, misalign)
    for sc, fl, g in zip(scs, flags, got):
        H.assert_same(with_cells(expectation(sc), fl), g, "%s (%s)" % (sc.name, what))
    return got


# ---------------------------------------------------------------------------------------------------- the batches of the tests
def pipe_batch():
    """pipe_a, pipe_b (reinforcements change every grid size mid-episode), gather_bench_a and battle_blind_actor, 12 steps; pipe_b is given
    float32 views, the others cells"""
    a, b = H.pipe_batch_scenarios()[:2]
    part = {sc.name: sc for sc in H.pipe_partial_scenarios()}
    scs = [a, b, part["gather_bench_a"], part["battle_blind_actor"]]
    assert [sc.name for sc in scs] == ["pipe_a", "pipe_b", "gather_bench_a", "battle_blind_actor"] and all(sc.steps == 12 for sc in scs)
    return scs, [[True, True], [False, False], [True, True], [True, True]]


def check_pipe_batch(lib):
    """the batch of pipe_batch() under this process's MAGENT_TUNE: every output the oracle's, and pipeline_stats()[6] what
    helpers.expected_pipe_cycles says -- nothing left the pipeline because of the format.  Returns the last counters and how many of the
    cycles the batch's render launch was the sweeping kernel (pipeline_stats()[7] of the first environment)."""
    scs, flags = pipe_batch()
    log = {}
    check(scs, lib, flags, "batched pipeline, MAGENT_TUNE=%s" % os.environ.get("MAGENT_TUNE", ""), log=log)
    expect = H.expected_pipe_cycles(scs, [expectation(sc) for sc in scs], os.environ.get("MAGENT_TUNE", ""))
    assert log["piped"] == expect, (log["piped"], expect)
    assert min(expect[-1]) >= 10, expect[-1]
    own = H.tune_settings().get("pipe_own", 48) == 1
    # a world rendering for itself launches once per observed group (Env::observe_device); in the batch's launch the profile counts none
    for piped_before, piped, renders, observed in zip([[0] * len(scs)] + log["piped"], log["piped"], log["renders"], log["observed"]):
        for k in range(len(scs)):
            if piped[k] > piped_before[k]:
                assert renders[k] == (observed[k] if own else 0), (k, renders, observed, own)
    return log["piped"][-1], "swept", log["swept"][-1]
