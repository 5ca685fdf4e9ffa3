"""Every caller-owned output buffer of the engine between sentinel guards.

The engine writes observations, feature rows, rewards and infos into memory the caller owns -- in the device ABI a torch tensor of the
caching allocator, where a store past the end lands in another live tensor and an unwritten cell keeps the previous step's plausible value.
Here every such buffer is the interior of ONE allocation [guard | interior | guard] prefilled with a word no correct output holds
(helpers.guarded): the interior must come back bit for bit what the oracle returns through the plain host calls for the same world -- which
also proves every byte was written -- and the guards, with the rows between n and the buffer's capacity, must still hold the sentinel.
Every comparison is on integer words; there is no tolerance in this file.

Two legs, as in the policy tests: `emu` runs the kernels lane by lane on the CPU (tests/hipemu), `gpu` (marked) the product library
in-process on torch tensors.  The worlds (helpers.buffer_worlds) are played for three steps and cleared, so that n has shrunk under an
unchanged capacity.  MAGENT_TUNE is read once per process: every non-default kernel form runs helpers.check_engine_buffer_forms in a child.
The checks assert which kernel / which form of env_cycle_many ran from the engine's own counters.
"""
import os
import subprocess
import sys

import pytest

import helpers as H

ROOT = H.ROOT
LEGS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
WORLDS = H.BUFFER_BATTLES + H.BUFFER_SHAPES

# a child of a gpu leg that ended by signal or at its time limit: nothing more is started on the card from this file
_GPU_DOWN = []


def lib_of(leg):
    if leg == "emu":
        return H.ensure_emu()
    assert not _GPU_DOWN, "an earlier gpu leg of this file ended by signal or at its time limit (%s): nothing more is started on the card" % _GPU_DOWN[0]
    import torch
    assert torch.cuda.is_available()
    return H.HIP_LIB


@pytest.mark.parametrize("name", WORLDS)
@pytest.mark.parametrize("leg", LEGS)
def test_observations_stay_inside_their_buffers(leg, name):
    """env_get_observation_device: view and feature interiors at float offsets 0 and 4 (the 16-byte stores and their tail), 1, 2 and 3 (the
    scalar path), one of each (the stand-alone k_features launch); env_get_observation_device_bf16 (games of up to 7 channels): the view at 0
    and 8 bf16 elements, the feature rows aligned and not -- expected: RNE-to-bf16 of the oracle's view, zeros up to channel 6, 1.0 in channel 7"""
    seen = H.check_observation_buffers(lib_of(leg), name)
    if name in H.BUFFER_BATTLES:       # by default a small battle world's float32 view is k_render's, its bf16 cells k_render_fast's
        assert (0, False) in seen and (1, True) in seen, seen


@pytest.mark.parametrize("name", WORLDS)
@pytest.mark.parametrize("leg", LEGS)
def test_rewards_and_infos_stay_inside_their_buffers(leg, name):
    """env_get_reward_device and env_get_info_device for id, hp, pos, alive -- every name the entry takes -- with the dead still in the arrays
    and behind clear_dead, against the oracle's host getters"""
    H.check_getter_buffers(lib_of(leg), name)


@pytest.mark.parametrize("name", WORLDS + ["battle60"])
@pytest.mark.parametrize("leg", LEGS)
def test_a_cycle_of_one_world_stays_inside_its_buffers(leg, name):
    """env_cycle_many over one environment (run_cycle(fused=True)'s call form) with caller-owned views, feature rows and rewards: the two-launch
    cycle up to 1536 agents, the call sequence above (battle60) -- asserted from the render launches the engine's profile counts"""
    H.check_cycle_buffers(lib_of(leg), [name])


@pytest.mark.parametrize("leg", LEGS)
def test_a_batched_cycle_stays_inside_its_buffers(leg):
    """EnvBatch.cycle over three battle worlds in one call (one pair of launches for all of them)"""
    H.check_cycle_buffers(lib_of(leg), ["battle_63_65", "battle_509_3", "battle_255_256"])


@pytest.mark.parametrize("name,group", [("battle_64_257", 0), ("battle_255_256", 1), ("gather", 0)])
@pytest.mark.parametrize("leg", LEGS)
def test_a_cycle_with_a_group_left_out_completes_the_other_buffers(leg, name, group):
    """NULL view / feat / reward entries for one group: the other groups' guarded buffers are complete all the same"""
    H.check_cycle_buffers(lib_of(leg), [name], leave_out=group)


@pytest.mark.parametrize("name", ["battle_1_2", "battle_509_3", "gather", "quad", "bodies", "arrange", "battle_empty_side"])
@pytest.mark.parametrize("leg", LEGS)
def test_the_host_abi_stays_inside_its_buffers(leg, name):
    """env_get_observation, env_get_reward and env_get_info (id, alive, pos, mean_info, view2attack, a 5 x 6 global_minimap) into NumPy
    interiors carved from guarded arrays: the device-to-host copies have sizes of their own"""
    H.check_host_abi_buffers(lib_of(leg), name)


SWEEPS = ["render=4,render_sweep=3", "render=4,render_sweep=2,render_su=3,render_depth=3", "render=4,render_sweep=7,render_su=1,render_depth=1"]
FORMS = ["render=0", "render=1"] + SWEEPS + ["batch_pipe_min=1", "batch_pipe_min=1,pipe_own=1", "batch_pipe_min=1,pipe_own=4096,pipe_sweep=3",
                                             "batch_pipe_min=1,pipe_sweep=0", "solo_step=0,scan_solo_max=100"]
CHILD = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
         "import helpers as H\n"
         "print('ok', H.check_engine_buffer_forms(H.ensure_emu() if sys.argv[1] == 'emu' else H.HIP_LIB))\n") % (ROOT, os.path.join(ROOT, "tests"))


def run_child(leg, extra, timeout):
    """helpers.check_engine_buffer_forms in a process of its own.  A gpu child that ends by signal or at its time limit fails its test and
    closes the file's remaining gpu legs; nothing is tried again."""
    lib_of(leg)
    env = H.merge_env(os.environ, {"OMP_NUM_THREADS": "1"}, extra)
    try:
        p = subprocess.run([sys.executable, "-c", CHILD, leg], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        if leg == "gpu":
            _GPU_DOWN.append("%s: no end within %d s" % (extra, timeout))
        raise AssertionError("%s %s: the child did not end within %d s: %s" % (leg, extra, timeout, str(e.stderr)[-2000:]))
    if leg == "gpu" and (p.returncode < 0 or p.returncode in (124, 134, 137, 139)):
        _GPU_DOWN.append("%s: exit code %d" % (extra, p.returncode))
    assert p.returncode == 0 and p.stdout.startswith("ok"), (leg, extra, p.returncode, p.stdout[-1500:] + p.stderr[-3000:])
    return p.stdout


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("leg", LEGS)
def test_kernel_forms_stay_inside_their_buffers(leg, form):
    """every render kernel the defaults do not pick at these sizes (k_render_fast for float32, k_render_sweep2 with few workgroups and many
    rounds, 1-3 strips, depth 1-3), the batched pipeline's render forms (the batch's sweeping or generic launch, a world's own launches) and
    its folded get_reward, the multi-launch step: the battle pairs, gather and pursuit_dense through the observation and cycle checks"""
    out = run_child(leg, {"MAGENT_TUNE": form}, 900 if leg == "emu" else 60)       # (a gpu child takes ~3 s, most of it process start)
    if form.startswith("render=4"):
        assert "(4, False)" in out and "(4, True)" in out, out       # float32 (battle, gather, pursuit's 5 channels) and bf16 cells
    if form == "render=1":
        assert "(1, False)" in out and "(1, True)" in out, out


@pytest.mark.parametrize("form", SWEEPS)
def test_sweeping_render_in_scrambled_order_stays_inside_its_buffers(form):
    """the sweeping kernel's rounds with lanes and workgroups in a pseudo-random order (emulator only)"""
    out = run_child("emu", {"MAGENT_TUNE": form, "HIPEMU_SCRAMBLE": "5"}, 900)
    assert "(4, False)" in out and "(4, True)" in out, out
