"""Rule-based actors: the reference's four (python/magent/builtin/rule_model/): `RandomActor`, and the scripted opponents of
pursuit and gather that sit on its `temp_c_booster` -- `RushPredator`, `RunawayPrey`, `RushGatherer`.

Work on both observation forms of `GridWorld.get_observation`: numpy arrays give a numpy int32 action vector, torch
tensors (device_obs mode) give an int32 tensor on the same device, so that the actions never leave the GPU.

The three scripted actors run include/magent_runtime_api.h PART 3: numpy observations go to the reference's own host symbols
(the same actions, and the same libc random() / rand() state afterwards, as the reference on one thread); float32 device
observations go to `actor_infer_action_device`, enqueued on torch's current stream.  The device cannot share libc's state:
an agent whose action is drawn draws from a stream of (seed, call counter, agent) instead, and `last_drew`
marks those agents; every other agent gets exactly the reference's action."""
import ctypes

import numpy as np

from .. import c_lib
from ..model import BaseModel


class RandomActor(BaseModel):
    def __init__(self, env, handle, *args, seed=None, **kwargs):
        super().__init__(env, handle)
        self.env, self.handle = env, handle
        self.n_action = int(env.get_action_space(handle)[0])
        self._host_rng = np.random if seed is None else np.random.RandomState(seed)
        self._device_rng = None
        self._seed = seed

    def infer_action(self, obs, *args, **kwargs):
        view = obs[0]
        count = len(view)
        if isinstance(view, np.ndarray):
            return self._host_rng.randint(self.n_action, size=count, dtype=np.int32)
        import torch
        if self._device_rng is None and self._seed is not None:
            self._device_rng = torch.Generator(device=view.device)
            self._device_rng.manual_seed(int(self._seed))
        return torch.randint(self.n_action, (count,), dtype=torch.int32, device=view.device, generator=self._device_rng)


class MagentActorArgs(ctypes.Structure):
    """include/magent_runtime_api.h MagentActorArgs"""
    _fields_ = [("kind", ctypes.c_int), ("n", ctypes.c_int), ("height", ctypes.c_int), ("width", ctypes.c_int),
                ("n_channel", ctypes.c_int), ("attack_base", ctypes.c_int), ("channel", ctypes.c_int), ("move_back", ctypes.c_int),
                ("threshold", ctypes.c_float), ("seed", ctypes.c_ulonglong), ("counter", ctypes.c_ulonglong)]


RUNAWAY, RUSH_PREY, GATHER = 0, 1, 2        # MAGENT_ACTOR_*
DEFAULT_SEED = 0x6D6167656E74              # seed=None: the device draws are still reproducible


class _BoosterActor(BaseModel):
    """common part of the three actors over temp_c_booster: host symbol on numpy observations, device kernel on CUDA tensors"""
    _actor_lib_path = None      # None: the product library (c_lib.DEFAULT_LIB)

    def __init__(self, env, handle, seed=None):
        super().__init__(env, handle)
        self.env, self.handle = env, handle
        self.attack_base, self.view2attack = env.get_view2attack(handle)
        self.view2attack = np.ascontiguousarray(self.view2attack, dtype=np.int32)
        self.seed = DEFAULT_SEED if seed is None else int(seed)
        self.counter = 0                        # device calls so far: the stream position of the next call's draws
        self.last_drew = None                   # device calls: uint8 tensor [n], 1 where the action was drawn
        self._lib = c_lib.load(self._actor_lib_path)
        if not getattr(self._lib, "has_actor_api", False):
            raise RuntimeError("this library does not export the rule-based actors (include/magent_runtime_api.h PART 3)")
        self._v2a_dev = {}

    def _args(self, n, h, w, c):
        raise NotImplementedError

    def _host(self, view, feature, n, h, w, c, out):
        raise NotImplementedError

    def infer_action(self, observations, *args, **kwargs):
        view, feature = observations[0], observations[1]
        if isinstance(view, np.ndarray):
            return self._infer_host(view, feature)
        import torch
        if view.dtype != torch.float32:
            raise TypeError("%s: observations must be float32 (got %s; bf16-cell observations are not served)" % (type(self).__name__, view.dtype))
        if view.device.type != "cuda":
            return torch.from_numpy(self._infer_host(view.numpy(), feature.numpy()))
        return self._infer_device(view, feature)

    def _infer_host(self, view, feature):
        if view.dtype != np.float32 or view.ndim != 4:
            raise TypeError("%s: observations must be float32 [n, H, W, C] (got %s %s)" % (type(self).__name__, view.dtype, view.shape))
        view = np.ascontiguousarray(view)
        feature = np.ascontiguousarray(feature, dtype=np.float32)
        n, h, w, c = view.shape
        self._check_view(h, w, c)
        self._check_feature(n, feature.size)
        out = np.empty((n,), dtype=np.int32)
        if n:
            self._host(view, feature, n, h, w, c, out)
        return out

    def _infer_device(self, view, feature):
        import torch
        if view.dim() != 4:
            raise TypeError("%s: observations must be [n, H, W, C] (got %s)" % (type(self).__name__, tuple(view.shape)))
        view, feature = view.contiguous(), feature.contiguous()
        if feature.dtype != torch.float32:
            raise TypeError("%s: features must be float32 (got %s)" % (type(self).__name__, feature.dtype))
        n, h, w, c = view.shape
        self._check_view(h, w, c)
        self._check_feature(n, feature.numel())
        dev = view.device
        actions = torch.empty((n,), dtype=torch.int32, device=dev)
        drew = torch.empty((n,), dtype=torch.uint8, device=dev)
        v2a = self._v2a_dev.get(dev)
        if v2a is None:
            v2a = self._v2a_dev[dev] = torch.from_numpy(self.view2attack.reshape(-1)).to(dev)
        args = self._args(n, h, w, c)
        args.seed, args.counter = self.seed & (2 ** 64 - 1), self.counter
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._lib.actor_infer_action_device(ctypes.byref(args), view.data_ptr(), feature.data_ptr(), v2a.data_ptr(),
                                            actions.data_ptr(), drew.data_ptr(), stream)
        self.counter += 1
        self.last_drew = drew
        return actions

    def _check_feature(self, n, size):
        if size < n:        # (the predator's threshold test reads one float per agent of the flattened array)
            raise ValueError("%s: %d agents but %d feature floats" % (type(self).__name__, n, size))

    def _check_view(self, h, w, c):
        if self.view2attack.shape != (h, w):
            raise ValueError("%s: view %dx%d does not match the group's view2attack %s" % (type(self).__name__, h, w, self.view2attack.shape))


class RushPredator(_BoosterActor):
    """rushes at the nearest attackable enemy (reference rule_model/rush.py, temp_c_booster.cc:39-83)"""
    def __init__(self, env, handle, attack_handle, *args, seed=None, **kwargs):
        super().__init__(env, handle, seed=seed)
        self.attack_channel = env.get_channel(attack_handle, handle)
        self.threshold = 100.0

    def _check_view(self, h, w, c):
        super()._check_view(h, w, c)
        if not 1 <= self.attack_channel < c:
            raise ValueError("RushPredator: channel %d of a %d-channel view" % (self.attack_channel, c))

    def _args(self, n, h, w, c):
        return MagentActorArgs(kind=RUSH_PREY, n=n, height=h, width=w, n_channel=c, attack_base=self.attack_base,
                               channel=self.attack_channel, threshold=self.threshold)

    def _host(self, view, feature, n, h, w, c, out):
        self._lib.rush_prey_infer_action(view.ctypes.data, feature.ctypes.data, n, h, w, c, out.ctypes.data, self.attack_channel,
                                         self.attack_base, self.view2attack.ctypes.data, ctypes.c_float(self.threshold))


class RunawayPrey(_BoosterActor):
    """steps back from whatever of `away_handle` comes close in front (reference rule_model/runaway.py, temp_c_booster.cc:14-37)"""
    def __init__(self, env, handle, away_handle, *args, seed=None, **kwargs):
        super().__init__(env, handle, seed=seed)
        self.away_channel = env.get_channel(away_handle, handle)
        self.move_back = 4

    def _args(self, n, h, w, c):
        return MagentActorArgs(kind=RUNAWAY, n=n, height=h, width=w, n_channel=c, attack_base=self.attack_base,
                               channel=self.away_channel, move_back=self.move_back)

    def _host(self, view, feature, n, h, w, c, out):
        self._lib.runaway_infer_action(view.ctypes.data, feature.ctypes.data, n, h, w, c, self.attack_base, out.ctypes.data,
                                       self.away_channel, self.move_back)

    def _check_view(self, h, w, c):
        if not 0 <= self.away_channel < c:      # (runaway reads no view2attack)
            raise ValueError("RunawayPrey: channel %d of a %d-channel view" % (self.away_channel, c))


class RushGatherer(_BoosterActor):
    """walks to food in view, else to the richest food of the minimap (reference rule_model/rushgather.py, temp_c_booster.cc:115-181)"""
    def __init__(self, env, handle, *args, seed=None, **kwargs):
        super().__init__(env, handle, seed=seed)
        self.n_action = env.get_action_space(handle)
        self.view_size = env.get_view_space(handle)

    def _args(self, n, h, w, c):
        return MagentActorArgs(kind=GATHER, n=n, height=h, width=w, n_channel=c, attack_base=self.attack_base)

    def _check_view(self, h, w, c):
        super()._check_view(h, w, c)
        if c < 7:
            raise ValueError("RushGatherer reads channels 3, 4 and 6: the view has %d" % c)

    def _host(self, view, feature, n, h, w, c, out):
        self._lib.gather_infer_action(view.ctypes.data, feature.ctypes.data, n, h, w, c, out.ctypes.data, self.attack_base,
                                      self.view2attack.ctypes.data)
