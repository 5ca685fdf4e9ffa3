"""AdvantageActorCritic.train(rec) of a magent_amd.DeviceEpisodesBuffer: the packed route (a2c.py: _packed_round) -- packed()'s tensors as
they are, ONE batched bootstrap pass over every episode's last observation, the returns from rec.returns on the device -- on
test_replay_batch.play_round's recorders (three battle worlds, more than 100 episodes, terminal and unfinished ones), plain and with
CommNet.

Against float64: test_learning.np_a2c_step on the episodes of rec.buffer and a float64 copy of the parameters from before the step, under
test_learning's own yardsticks (bound("a2c", "returns"), bound("a2c", "loss")); no tolerance is set here.  The returns are, besides, bit
for bit helpers.np_discounted_returns of the bootstrap values the model computed.  A twin with the same parameters trained through the
episodes route (a wrapper that offers episodes() only: what every release before this route did) reports the same losses within
2 x bound("a2c", "loss") -- both lie within one bound of the same float64 value --, and each twin's Adam update passes
test_learning.check_update.  The twins' PARAMETERS are not compared with adam_bound: Adam's first step is lr * g / (|g| + eps), which turns
the round-off of a gradient entry near zero into a step of the other sign, 2 lr apart; check_update feeds Adam the gradients the model
itself produced for that reason, and does not fit two models.

Two legs as in test_replay_kernels: `emu` (the recorder's kernels lane by lane on the CPU, the model on the CPU) and `gpu` (marked)."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import helpers as H
from magent_amd.builtin.torch_model import AdvantageActorCritic
from test_learning import Env, Spy, bound, check_update, load_params, make_buffer, np_a2c_step, rel, within
from test_replay_batch import play_round
from test_replay_kernels import bits

LEGS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
COMM = [pytest.param(False, id="plain"), pytest.param(True, id="comm")]
SIDE = 1
_trained = {}


class EpisodesOnly(object):
    """a recorder as the episodes route sees it"""

    def __init__(self, rec):
        self._rec = rec

    def episodes(self):
        return self._rec.episodes()


def run_train(model, buf):
    """(losses, value, forward calls' row counts, printed text, spy) of one model.train(buf)"""
    spy, calls, text = Spy(model, model.net), [], io.StringIO()
    handle = model.net.register_forward_hook(lambda module, args, output: calls.append(int(args[0].shape[0])))
    try:
        with contextlib.redirect_stdout(text):
            losses, value = model.train(buf)
    finally:
        handle.remove()
        spy.close()
    return losses, value, calls, text.getvalue(), spy


def trained(leg, comm):
    """one train(rec) on the round's recorder of side SIDE and one of the twin, run once per (leg, comm)"""
    if (leg, comm) in _trained:
        return _trained[leg, comm]
    recs, wants, told, alive, envs, handles, dev = play_round(leg)
    rec = recs[SIDE]
    models = []
    for k in range(2):
        torch.manual_seed(16 + comm)
        models.append(AdvantageActorCritic(envs[0], handles[0][SIDE], "packed_a2c%d" % k, use_comm=comm, device=dev))
    before = [p.detach().clone() for p in models[0].net.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(before, models[1].net.parameters()))
    seen, real = {}, rec.returns

    def returns(bootstrap, gamma):
        out = real(bootstrap, gamma)
        seen.update(bootstrap=bootstrap.detach().clone(), gamma=gamma, out=out.detach().clone())
        return out
    rec.returns, rec._entries = returns, None
    try:
        packed = run_train(models[0], rec)
        entries_after = rec._entries
    finally:
        del rec.returns
    twin = run_train(models[1], EpisodesOnly(rec))
    eps = []
    for ep in rec.buffer.values():                               # slot order; capacity 512 takes everybody, nobody is empty
        to64 = lambda x: torch.stack(x).cpu().numpy().astype(np.float64)
        eps.append((to64(ep.views), to64(ep.features), np.asarray(ep.actions, np.int64), np.asarray(ep.rewards, np.float64), bool(ep.terminal)))
    net64 = copy.deepcopy(models[0].net).cpu().double()
    load_params(net64, before)
    want64 = np_a2c_step(np.float64, net64, eps, comm, 0.99, 0.1, 0.08)
    _trained[leg, comm] = {"models": models, "packed": packed, "twin": twin, "seen": seen, "eps": eps, "want": want64, "rec": rec,
                           "entries_after": entries_after, "want_rec": wants[SIDE], "gpu": leg == "gpu"}
    return _trained[leg, comm]


@pytest.mark.parametrize("comm", COMM)
@pytest.mark.parametrize("leg", LEGS)
def test_train_from_the_recorder_against_float64(leg, comm):
    t = trained(leg, comm)
    w, gpu, tag = t["want"], t["gpu"], "a2c packed %s %s" % (leg, "comm" if comm else "plain")
    losses, value = t["packed"][0], t["packed"][1]
    got = t["seen"]["out"].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == w["returns"].shape and t["seen"]["gamma"] == 0.99
    assert sum(1 for e in t["eps"] if e[4]) > 0 and sum(1 for e in t["eps"] if not e[4]) > 0 and len(t["eps"]) > 100
    within(tag + " returns", rel(got, w["returns"], 1.0 + float(np.abs(w["returns"]).max())), bound("a2c", "returns", gpu))
    assert len(losses) == 3
    for name, g, want in zip(("pg_loss", "vf_loss", "neg_entropy"), losses, w["losses"]):
        within("%s %s" % (tag, name), abs(g - want) / abs(want), bound("a2c", "loss", gpu))
    within(tag + " returned value", abs(value - w["value"]) / (1.0 + abs(w["value"])), bound("a2c", "loss", gpu))
    check_update(tag, t["packed"][4], 1e-3)


@pytest.mark.parametrize("comm", COMM)
@pytest.mark.parametrize("leg", LEGS)
def test_the_returns_are_the_host_loops_function_of_the_bootstrap_values(leg, comm):
    """bit for bit, given the values the batched pass computed"""
    t = trained(leg, comm)
    boot = t["seen"]["bootstrap"].cpu().numpy()
    lens = [len(e[3]) for e in t["eps"]]
    assert boot.dtype == np.float32 and boot.shape == (len(lens),) and np.abs(boot).min() > 0
    want = np.concatenate([H.np_discounted_returns(e[3], boot[s], 0.99) for s, e in enumerate(t["eps"])]).astype(np.float32)
    assert np.array_equal(bits(t["seen"]["out"]), bits(want))
    slots, rows = t["rec"].last_rows()
    assert slots.cpu().tolist() == list(range(len(lens))) and rows.cpu().tolist() == (np.cumsum(lens) - 1).tolist()


@pytest.mark.parametrize("comm", COMM)
@pytest.mark.parametrize("leg", LEGS)
def test_two_forward_passes_and_no_episode_objects(leg, comm):
    """the bootstrap batch (one row per episode) and the training pass (every transition); the recorder's per-agent view was not built"""
    t = trained(leg, comm)
    losses, value, calls, text, spy = t["packed"]
    n, n_eps = t["want_rec"].transitions, len(t["eps"])
    assert calls == [n_eps, n], calls
    assert t["entries_after"] is None
    assert t["models"][0].train_ct == 1 and len(spy.steps) == 1 and text.startswith("sample %d " % n)


@pytest.mark.parametrize("comm", COMM)
@pytest.mark.parametrize("leg", LEGS)
def test_a_twin_trained_through_the_episodes_route(leg, comm):
    """one forward pass per episode and the training pass; the same losses within 2 x bound (the module's docstring), its own Adam update
    within the format bound"""
    t = trained(leg, comm)
    w, gpu, tag = t["want"], t["gpu"], "a2c twins %s %s" % (leg, "comm" if comm else "plain")
    losses, value, calls, text, spy = t["twin"]
    n, n_eps = t["want_rec"].transitions, len(t["eps"])
    assert calls == [1] * n_eps + [n] and text.startswith("sample %d " % n) and t["models"][1].train_ct == 1
    for name, a, b, want in zip(("pg_loss", "vf_loss", "neg_entropy"), t["packed"][0], losses, w["losses"]):
        within("%s %s" % (tag, name), abs(a - b) / abs(want), 2 * bound("a2c", "loss", gpu))
    within(tag + " returned value", abs(t["packed"][1] - value) / (1.0 + abs(w["value"])), 2 * bound("a2c", "loss", gpu))
    check_update(tag, spy, 1e-3)


@pytest.mark.parametrize("comm", COMM)
def test_a_host_buffer_goes_the_episodes_route(comm):
    """utility.EpisodesBuffer has packed() and episodes(), no last_rows / returns: one bootstrap pass per episode, as before"""
    vs, feat, A = (5, 5, 3), 6, 7
    torch.manual_seed(3)
    model = AdvantageActorCritic(Env(vs, feat, A), 0, "host_a2c", use_comm=comm, device=torch.device("cpu"))
    buf = make_buffer(vs, feat, A, 40)
    assert hasattr(buf, "packed") and not hasattr(buf, "returns")
    lens = [len(ep.rewards) for ep in buf.episodes()]
    losses, value, calls, text, spy = run_train(model, buf)
    assert calls == [1] * len(lens) + [sum(lens)] and model.train_ct == 1 and text.startswith("sample %d " % sum(lens))


@pytest.mark.parametrize("leg", LEGS)
def test_a_round_with_nothing_recorded(leg):
    recs, wants, told, alive, envs, handles, dev = play_round(leg)
    from magent_amd.replay import DeviceEpisodesBuffer
    from test_replay_kernels import leg_of
    empty = DeviceEpisodesBuffer(8, 8, recs[0].view_shape, recs[0].feature_shape, device=dev, lib=leg_of(leg)[0])
    model = AdvantageActorCritic(envs[0], handles[0][0], "empty_a2c", device=dev)
    assert model.train(empty) == ([0.0, 0.0, 0.0], 0.0) and model.train_ct == 0
