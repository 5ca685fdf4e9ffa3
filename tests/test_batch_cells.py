"""bf16 observation cells through env_cycle_many_cells / EnvBatch.cycle, and the packed layout of a batch's buffers.

Every form of the batched cycle -- the two-launch cycle of one environment (k_render_multi) and of many (k_render_batch), the batched
pipeline (k_pipe_render, the sweeping kernel), a world's own render launches inside the pipeline, the call sequence of a world that goes
alone -- writes the views of the entries flagged as cells in env_get_observation_device_bf16's format and the others as float32, in one
call.  The expectation is the oracle's: every scenario played alone through the reference call sequence, its float32 views rounded to bf16
on the bits (helpers.bf16_cells) where cells were asked for.  Every comparison is on integer words; there is no tolerance in this file
(the one policy test compares int32 actions).  All buffers sit between sentinel guards.

Two legs: `emu` runs the same .hip sources lane by lane on the CPU, `gpu` (marked) the product library.  MAGENT_TUNE is read once per
process: non-default settings run in a child under its own time limit; after a gpu child that ended by signal or at its time limit nothing
more is started on the card from this file.
"""
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_cells_driver as D
import helpers as H
import magent_amd

ROOT = H.ROOT
LEGS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
_GPU_DOWN = []


def lib_of(leg):
    if leg == "emu":
        return H.ensure_emu()
    assert not _GPU_DOWN, "an earlier gpu leg of this file ended by signal or at its time limit (%s): nothing more is started on the card" % _GPU_DOWN[0]
    import torch
    assert torch.cuda.is_available()
    return H.HIP_LIB


CHILD = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
         "import helpers as H, batch_cells_driver as D\n"
         "print('ok', D.check_pipe_batch(H.ensure_emu() if sys.argv[1] == 'emu' else H.HIP_LIB))\n") % (ROOT, os.path.join(ROOT, "tests"))


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


def partial(name):
    return {sc.name: sc for sc in H.cycle_partial_scenarios()}[name]


# ---------------------------------------------------------------------------------------------------- 1. two launches, one environment
@pytest.mark.parametrize("name", ["battle_partial", "gather_partial"])
@pytest.mark.parametrize("leg", LEGS)
def test_one_world_renders_its_cells_in_one_launch(leg, name):
    """k_render_multi's cell form: a world of the two-launch cycle alone in its EnvBatch, every view as cells, all its steps; the profile
    counts ONE render launch per cycle"""
    sc, log = partial(name), {}
    D.check([sc], lib_of(leg), [[True, True]], "alone, cells, %s" % leg, log=log)
    assert len(log["renders"]) == sc.steps and log["observed"][0][0] >= 1, log       # (a cycle in which the observed group has died out renders nothing)
    assert all(r == [min(1, o[0])] for r, o in zip(log["renders"], log["observed"])), (log["renders"], log["observed"])
    assert log["piped"][-1] == [0]


# ---------------------------------------------------------------------------------------------------- 2. two launches, a batch
@pytest.mark.parametrize("leg", LEGS)
def test_a_batch_of_small_worlds_renders_cells_and_float32_in_one_launch(leg):
    """k_render_batch's cell form: the four cycle_partial_scenarios in one EnvBatch, battle_partial with side 0 float32 and side 1 cells, the
    others all cells; every buffer guarded with a row of capacity to spare"""
    scs = H.cycle_partial_scenarios()
    flags = [[False, True] if sc.name == "battle_partial" else [True, True] for sc in scs]
    D.check(scs, lib_of(leg), flags, "batch of four, %s" % leg)


@pytest.mark.parametrize("leg", LEGS)
def test_a_batch_at_the_wave_and_span_edges_renders_cells(leg):
    """the three battle worlds of test_a_batched_cycle_stays_inside_its_buffers (sizes around a wave step and a span), cells -- but for side 0
    of battle_509_3, float32: both formats in one k_render_batch launch; no render launch of an environment's own"""
    W = H.buffer_worlds()
    scs = [W[n] for n in ("battle_63_65", "battle_509_3", "battle_255_256")]
    log = {}
    D.check(scs, lib_of(leg), [[True, True], [False, True], [True, True]], "batch of three, %s" % leg, log=log)
    assert all(r == [0, 0, 0] for r in log["renders"]) and all(all(a) for a in log["aligned"]), log


# ---------------------------------------------------------------------------------------------------- 3. the batched pipeline
@pytest.mark.parametrize("leg", LEGS)
def test_the_batched_pipeline_renders_cells_and_float32(leg):
    """pipe_a, gather_bench_a and battle_blind_actor as cells, pipe_b as float32, ONE EnvBatch, 12 steps, under the defaults;
    pipeline_stats()[6] is what the float32 call's would be (helpers.expected_pipe_cycles)"""
    D.check_pipe_batch(lib_of(leg))


@pytest.mark.parametrize("tune", ["pipe_sweep=0", "pipe_sweep=3", "batch_pipe_min=1,pipe_sweep=2"])
@pytest.mark.parametrize("leg", LEGS)
def test_both_render_kernels_of_the_pipeline_write_cells(leg, tune):
    """the same batch with the sweeping render switched off (the generic workgroups: k_pipe_render's cell form) and on with few
    workgroups per segment (many rounds each), in children"""
    run_child(leg, tune, 1500 if leg == "emu" else 90)


# ---------------------------------------------------------------------------------------------------- 4. the own-render branch
@pytest.mark.parametrize("leg", LEGS)
def test_worlds_that_render_for_themselves_inside_the_pipeline_write_cells(leg):
    """MAGENT_TUNE pipe_own=1: every observed group renders through observe_device(..., cells16) inside pipe_prepare -- one launch per
    observed group in the profile -- and every cycle still counts as the pipeline's"""
    run_child(leg, "pipe_own=1", 1500 if leg == "emu" else 90)


# ---------------------------------------------------------------------------------------------------- 5. a world that goes alone
@pytest.mark.parametrize("leg", LEGS)
def test_a_world_that_goes_alone_writes_cells(leg):
    """scenarios()["gather"]: both groups observed through different windows under minimap_mode -- pipe_eligible and cycle_eligible refuse it.
    Beside pipe_a, all cells, 6 steps: its pipeline counter stays 0, it renders once per observed group, its cells are the oracle's"""
    gather, pipe_a = copy.deepcopy(H.scenarios()["gather"]), copy.deepcopy(H.pipe_batch_scenarios()[0])
    gather.steps = pipe_a.steps = 6
    log = {}
    D.check([gather, pipe_a], lib_of(leg), [[True, True], [True, True]], "goes alone, %s" % leg, log=log)
    assert [p[0] for p in log["piped"]] == [0] * 6, log["piped"]
    assert [r[0] for r in log["renders"]] == [o[0] for o in log["observed"]] and log["observed"][0][0] == 2, log


# ---------------------------------------------------------------------------------------------------- 6. the packed layout
class FakeTensor(object):
    def __init__(self, addr, shape, elem):
        self.addr, self.shape, self.elem = addr, tuple(shape), elem

    def data_ptr(self):
        return self.addr

    def element_size(self):
        return self.elem

    def numel(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def is_contiguous(self):
        return True


class FakeEnv(object):
    game, group_handles = None, [0, 1]


def test_packed_offsets_and_pointers_are_the_documented_arithmetic():
    """EnvBatch.packed_offsets against a numpy restatement on hand-picked counts (0, 1, 3, 4, 5, a group empty in one environment), and
    packed_pointers on made-up base addresses.  No library, no device."""
    batch = magent_amd.EnvBatch.__new__(magent_amd.EnvBatch)
    batch.envs, batch.n_group = [FakeEnv() for _ in range(5)], 2
    nums = np.array([[0, 5], [1, 0], [3, 4], [4, 1], [5, 3]])
    for align in (4, 1, 8):
        off, tot = batch.packed_offsets(nums, align)
        pad = (nums + align - 1) // align * align
        want = np.concatenate([np.zeros((1, 2), dtype=np.int64), np.cumsum(pad, axis=0)[:-1]])
        assert np.array_equal(off, want) and np.array_equal(tot, pad.sum(axis=0)), (align, off, tot)
    off, tot = batch.packed_offsets(nums)
    assert off.tolist() == [[0, 0], [0, 8], [4, 8], [8, 12], [12, 16]] and tot.tolist() == [20, 20]
    # rows of 13 x 13 cells (2704 B), feature rows of 34 floats (136 B: 4 rows are 544 = 34 x 16), int32 actions
    for base, shape, elem in ((0x7F0000001000, (20, 13, 13, 8), 2), (0x7F0000100010, (20, 34), 4), (0x7F0000200020, (20,), 4)):
        row = int(np.prod(shape[1:], dtype=np.int64)) * elem
        arr = batch.packed_pointers([FakeTensor(base, shape, elem), None], off)
        assert len(arr) == 10
        for e in range(5):
            assert arr[2 * e] == base + int(off[e][0]) * row and arr[2 * e] % 16 == 0 and arr[2 * e + 1] is None, (e, arr[2 * e], arr[2 * e + 1])
    with pytest.raises(AssertionError):
        batch.packed_pointers([FakeTensor(0x7F0000001004, (20, 34), 4), None], off)       # (a base that is not 16-byte aligned)
    with pytest.raises(AssertionError):
        batch.packed_pointers([FakeTensor(0x7F0000001000, (20, 3), 2), None], off)        # (rows of 6 bytes)


PACKED = ["battle_63_65", "battle_509_3", "battle_255_256"]


@pytest.mark.parametrize("leg", LEGS)
def test_a_packed_batch_keeps_its_batched_form_and_its_pad_rows(leg):
    """three battle worlds whose sides are no multiples of 4, views (cells), feature rows, actions and rewards each ONE guarded buffer per side
    laid out by packed_offsets / packed_pointers, 3 steps: every segment the oracle's, every pad row and both guards the sentinel, every
    pointer 16-byte aligned and no render launch of an environment's own (the batch's two launches did the work)"""
    W, log = H.buffer_worlds(), {}
    D.check([W[n] for n in PACKED], lib_of(leg), [[True, True]] * 3, "packed, %s" % leg, align_rows=4, log=log)
    assert all(all(a) for a in log["aligned"]) and all(r == [0, 0, 0] for r in log["renders"]) and log["piped"][-1] == [0, 0, 0], log


@pytest.mark.parametrize("leg", LEGS)
def test_the_same_worlds_packed_without_padding_are_seen_to_go_alone(leg):
    """the control: align_rows=1.  Env::observed_groups_ok's condition restated on the pointers built (every observed group's view and
    feature pointer 16-byte aligned; a feature row is 136 bytes) says which world leaves the batch in which cycle; such a world renders by
    launches of its own, one per observed group, the others by none -- and every output is the oracle's all the same"""
    W, log = H.buffer_worlds(), {}
    D.check([W[n] for n in PACKED], lib_of(leg), [[True, True]] * 3, "packed without padding, %s" % leg, align_rows=1, log=log)
    assert not all(all(a) for a in log["aligned"]), "the sizes were chosen so that some segment starts off a 16-byte boundary"
    for aligned, renders, observed in zip(log["aligned"], log["renders"], log["observed"]):
        assert renders == [0 if a else o for a, o in zip(aligned, observed)], (aligned, renders, observed)


# ---------------------------------------------------------------------------------------------------- 7. refusals
def test_cells_of_a_game_with_more_than_seven_channels_are_refused_in_python():
    """a bf16 view for a three-group world (10 channels), and one whose last dimension is not 8: ValueError from EnvBatch.cycle before the
    library is entered (the engine's fatal() would end the process)"""
    import torch
    env = H.gridworld(H.custom_tri(20, 20), lib=H.ensure_oracle())
    env.reset()
    h, w, c = env.get_view_space(env.get_handles()[0])
    assert c > 7
    batch = magent_amd.EnvBatch([env], n_threads=1)
    with pytest.raises(ValueError):
        batch.cycle([[torch.zeros((1, h, w, 8), dtype=torch.bfloat16), None, None]], None, None, None)
    with pytest.raises(ValueError):
        batch.cell_flags([[torch.zeros((1, h, w, 8), dtype=torch.bfloat16), None, None]])
    small = H.gridworld("battle", lib=H.ensure_oracle(), map_size=20)
    small.reset()
    h, w, c = small.get_view_space(small.get_handles()[0])
    assert c == 7
    batch = magent_amd.EnvBatch([small], n_threads=1)
    with pytest.raises(ValueError):
        batch.cycle([[torch.zeros((1, h, w, 7), dtype=torch.bfloat16), None]], None, None, None)
    flags = batch.cell_flags([[torch.zeros((1, h, w, 8), dtype=torch.bfloat16), torch.zeros((1, h, w, 7))]])
    assert list(flags) == [1, 0] and batch.cell_flags([[torch.zeros((1, h, w, 7)), None]]) is None


# ---------------------------------------------------------------------------------------------------- 8. one policy call over a batch
@pytest.mark.gpu
def test_one_bf16_policy_call_over_a_packed_batch_equals_the_calls_per_environment():
    """three battle worlds (2 x 200, 2 x 400, 2 x 600), cells packed per side and rendered by ONE EnvBatch.cycle; DeepQNetwork(infer_dtype=
    "bf16").infer_action(policy="greedy") on the packed tensor, cut at the segments, equals the same model's actions on each environment's
    own get_observation_device_bf16 tensor -- exactly: a row's arithmetic does not depend on which rows share its tile"""
    import torch
    from magent_amd.builtin.torch_model import DeepQNetwork
    lib_of("gpu")
    envs = []
    for k, n in enumerate((200, 400, 600)):
        env = magent_amd.GridWorld("battle", map_size=60)
        env.set_seed(900 + k)
        env.reset()
        for h in env.get_handles():
            env.add_agents(h, "random", n=n - 3 * k - 1)       # (199, 396, 593: no multiples of 4)
        envs.append(env)
    handles = envs[0].get_handles()
    dev = torch.device("cuda", envs[0].device_id)
    batch = magent_amd.EnvBatch(envs, n_threads=1)
    nums = batch.nums_array().copy()
    off, tot = batch.packed_offsets(nums)
    hgt, wid, _ = envs[0].get_view_space(handles[0])
    F = envs[0].get_feature_space(handles[0])[0]
    alone = [[env.get_observation_device_bf16(h) for h in env.get_handles()] for env in envs]
    for env in envs:
        env.sync()
    views = [torch.zeros((int(tot[g]), hgt, wid, 8), dtype=torch.bfloat16, device=dev) for g in range(2)]
    feats = [torch.zeros((int(tot[g]), F), dtype=torch.float32, device=dev) for g in range(2)]
    torch.cuda.synchronize()
    batch.cycle(batch.packed_pointers(views, off), batch.packed_pointers(feats, off), None, None,
                view_cells=batch.cell_flags([[views[0], views[1]]] * 3))
    for env in envs:
        env.sync()
    for g, h in enumerate(handles):
        model = DeepQNetwork(envs[0], h, "side%d" % g, memory_size=16, infer_dtype="bf16")
        assert model._hip is not None
        packed = model.infer_action((views[g], feats[g]), None, policy="greedy").cpu().numpy()
        for e in range(3):
            n, o = int(nums[e][g]), int(off[e][g])
            assert torch.equal(views[g][o:o + n].view(torch.int16), alone[e][g][0].view(torch.int16)), (e, g)
            own = model.infer_action(alone[e][g], None, policy="greedy").cpu().numpy()
            assert np.array_equal(packed[o:o + n], own), (e, g, int((packed[o:o + n] != own).sum()))
