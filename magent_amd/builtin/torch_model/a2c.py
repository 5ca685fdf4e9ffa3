"""Advantage actor-critic on PyTorch-ROCm with the constructor / method surface of the reference's TensorFlow model
(python/magent/builtin/tf_model/a2c.py:10-14, 189-287).

Network (a2c.py:140-167): dense 256 (flattened view) || dense 256 (feature) -> dense 512 -> softmax policy head and a
scalar value head; optional CommNet block (mean of the OTHER agents' hidden units, two steps).  One update per
`train()` over every sample of the round: discounted returns bootstrapped with the value of each episode's last
observation, loss = -E[adv * log pi] + value_coef * E[(R - V)^2] + ent_coef * E[sum pi log pi], Adam."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...model import BaseModel


class _CommStep(nn.Module):
    """h' = tanh(mean_other(h) C + h H + skip)"""
    def __init__(self, size):
        super().__init__()
        self.C = nn.Linear(size, size, bias=False)
        self.H = nn.Linear(size, size, bias=False)

    def forward(self, h, skip, alone=False):
        n = h.shape[0]
        others = (h.sum(dim=0, keepdim=True) - h) / (n - 1) if n > 1 and not alone else torch.zeros_like(h)
        return torch.tanh(self.C(others) + self.H(h) + skip)


class _ActorCritic(nn.Module):
    def __init__(self, view_space, feature_space, n_action, use_comm):
        super().__init__()
        self.dense_view = nn.Linear(int(np.prod(view_space)), 256)
        self.dense_emb = nn.Linear(feature_space[0], 256)
        self.dense = nn.Linear(512, 512)
        self.comm = nn.ModuleList([_CommStep(512), _CommStep(512)]) if use_comm else None
        self.policy = nn.Linear(512, n_action)
        self.value = nn.Linear(512, 1)

    def forward(self, view, feature, alone=False):
        """alone: every row is a call of its own (the CommNet means are zeros)"""
        h = torch.cat([F.relu(self.dense_view(view.reshape(view.shape[0], -1))), F.relu(self.dense_emb(feature))], dim=1)
        h = F.relu(self.dense(h))
        if self.comm is not None:
            skip = h
            for step in self.comm:
                h = step(h, skip, alone)
        policy = F.softmax(self.policy(h), dim=1).clamp(1e-10, 1 - 1e-10)
        return policy, self.value(h).squeeze(1)


class AdvantageActorCritic(BaseModel):
    def __init__(self, env, handle, name, learning_rate=1e-3, batch_size=64, reward_decay=0.99, eval_obs=None,
                 train_freq=1, value_coef=0.1, ent_coef=0.08, use_comm=False, custom_view_space=None,
                 custom_feature_space=None, device=None, infer_dtype=None):
        BaseModel.__init__(self, env, handle)
        self.env, self.handle, self.name, self.subclass_name = env, handle, name, "torcha2c"
        self.view_space = tuple(custom_view_space or env.get_view_space(handle))
        self.feature_space = tuple(custom_feature_space or env.get_feature_space(handle))
        self.num_actions = env.get_action_space(handle)[0]
        self.reward_decay, self.batch_size, self.learning_rate, self.train_freq = reward_decay, batch_size, learning_rate, train_freq
        self.value_coef, self.ent_coef, self.use_comm, self.train_ct = value_coef, ent_coef, use_comm, 0
        if device is None:
            device = torch.device("cuda", getattr(env, "device_id", 0)) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        self.net = _ActorCritic(self.view_space, self.feature_space, self.num_actions, use_comm).to(self.device)
        self.optimizer = torch.optim.Adam(self.net.parameters(), lr=learning_rate)
        # Acting on device-resident float32 observations goes through hand-written kernels (magent_amd/csrc/policy_a2c_f32.hip: the network,
        # CommNet included, the softmax and an inverse-CDF draw from torch.rand); MAGENT_POLICY_F32=torch keeps the PyTorch forward pass and
        # torch.multinomial below, as for the DQN.  Numpy inputs, CPU devices and shapes the kernels do not take use that path too.
        # infer_dtype "bf16" (the argument, or MAGENT_POLICY_DTYPE=bf16 for scripts run unmodified) is the DQN's and the DRQN's opt-in: acting
        # then goes through the bf16 MFMA kernels (magent_amd/csrc/policy_a2c_bf16.hip: bf16 matrix operands and inter-layer rows, float32
        # accumulation, biases, column sums, softmax and draw) where the shape is theirs, and through what "f32" would use where it is not.
        # `bf16_kernels` says which.  Training is untouched by it.
        from . import hip_policy
        self.infer_dtype, self._hip, self.bf16_kernels = hip_policy.acting_policy(
            infer_dtype, self.device, hip_policy.HipA2cPolicy, hip_policy.HipA2cPolicyF32, self.net, self.view_space, self.feature_space,
            self.num_actions, self.device)

    def _on_kernels(self, view, feature):
        n = len(view)
        if not (self._hip is not None and isinstance(view, torch.Tensor) and isinstance(feature, torch.Tensor) and view.is_cuda
                and self.device.index in (None, view.device.index)
                and feature.device == view.device and feature.dtype == torch.float32 and view.is_contiguous()
                and feature.is_contiguous() and tuple(feature.shape) == (n,) + self.feature_space):
            return False
        if view.dtype == torch.bfloat16:     # the engine's bf16 cells [n, H, W, 8]: the bf16 kernels' operands as they are
            return self.bf16_kernels and self._hip.cells and tuple(view.shape) == (n,) + self.view_space[:2] + (8,)
        return view.dtype == torch.float32 and tuple(view.shape) == (n,) + self.view_space

    def _tensor(self, x, dtype=torch.float32):
        if isinstance(x, torch.Tensor):
            return x.to(self.device, dtype)
        return torch.as_tensor(np.ascontiguousarray(x)).to(self.device, dtype)

    def _policy_segments(self, view, feature, seg):
        """the PyTorch network's probabilities [n][A] of a segmented call: the network per segment, and once, every row alone, over the
        rows in no segment"""
        n = view.shape[0]
        policy = torch.empty((n, self.num_actions), device=view.device)
        free = torch.ones(n, dtype=torch.bool)
        for b, c in seg.tolist():
            if c > 0:
                policy[b:b + c] = self.net(view[b:b + c], feature[b:b + c])[0]
                free[b:b + c] = False
        idx = torch.nonzero(free).squeeze(1).to(view.device)
        if len(idx):
            policy[idx] = self.net(view[idx], feature[idx], alone=True)[0]
        return policy

    @torch.no_grad()
    def infer_action(self, raw_obs, ids, *args, segments=None, **kwargs):
        """one action per agent, sampled from the policy; raw_obs = (view [n,H,W,C], feature [n,F]), numpy or torch.

        segments: None, or an int array [n_seg][2] of (begin, count) rows for observations that pack several environments into one
        buffer (EnvBatch.packed_segments): the CommNet means then run inside each segment, and a row in no segment (a pad row, a stale
        row) acts alone.  The meaning is the same on the kernels and on the PyTorch path; without CommNet the table changes nothing."""
        view, feature = raw_obs[0], raw_obs[1]
        if len(view) == 0:
            return np.empty(0, dtype=np.int32)
        if segments is not None:
            from .hip_policy import check_segments
            segments = check_segments(segments, len(view))
        if self._on_kernels(view, feature):
            return self._hip.infer(view, feature, segments=segments)
        if isinstance(view, torch.Tensor) and view.dtype == torch.bfloat16:
            # bf16 cells [n, H, W, 8] (channels, zeros, a constant 1) without the bf16 kernels: the channels go back to float32
            view = view[..., :self.view_space[-1]].float().contiguous()
            if self._on_kernels(view, feature):
                return self._hip.infer(view, feature, segments=segments)
        if segments is not None and self.use_comm:
            policy = self._policy_segments(self._tensor(view), self._tensor(feature), segments)
        else:
            policy, _ = self.net(self._tensor(view), self._tensor(feature))
        acts = torch.multinomial(policy, 1).squeeze(1).to(torch.int32)
        return acts if isinstance(view, torch.Tensor) else acts.cpu().numpy()

    def _episodes_round(self, sample_buffer):
        """(view, feature, action, returns) of the round from the buffer's episodes, one at a time; None: nothing recorded"""
        views, features, actions, returns = [], [], [], []
        for ep in sample_buffer.episodes():
            m = len(ep.rewards)
            if m == 0:
                continue
            v = torch.stack(ep.views).to(self.device) if isinstance(ep.views[0], torch.Tensor) else self._tensor(np.stack(ep.views))
            f = torch.stack(ep.features).to(self.device) if isinstance(ep.features[0], torch.Tensor) else self._tensor(np.stack(ep.features))
            with torch.no_grad():
                keep = float(self.net(v[-1:], f[-1:])[1][0])      # bootstrap from the last observation (a2c.py:244-251)
            r = np.asarray(ep.rewards, dtype=np.float64)
            for i in reversed(range(m)):
                keep = keep * self.reward_decay + r[i]
                r[i] = keep
            views.append(v); features.append(f)
            actions.append(self._tensor(np.asarray(ep.actions), torch.int64)); returns.append(self._tensor(r))
        if not views:
            return None
        return torch.cat(views), torch.cat(features), torch.cat(actions), torch.cat(returns)

    def _packed_round(self, rec):
        """the same four tensors from a device recorder (magent_amd.DeviceEpisodesBuffer) without a per-episode step: packed()'s rows are
        the episodes' rows in slot order, as they are; the bootstrap values are ONE batched pass over every episode's last observation,
        each row alone (the episodes route's one-row calls: no CommNet message); the recurrence runs on the device, rec.returns, bit for
        bit the host loop's function of those values"""
        p = rec.packed()
        if p is None:
            return None
        view, feature = p[0], p[1]
        slots, rows = rec.last_rows()
        with torch.no_grad():
            values = self.net(view[rows], feature[rows], alone=True)[1]
        bootstrap = torch.zeros(rec.tracked, dtype=torch.float32, device=view.device)
        bootstrap[slots] = values
        return view, feature, p[2].to(torch.int64), rec.returns(bootstrap, self.reward_decay)

    def train(self, sample_buffer, print_every=1000):
        """one gradient step over all samples of the round; returns ([pg_loss, vf_loss, ent_loss], mean state value).  A buffer that
        offers packed(), last_rows() and returns() (DeviceEpisodesBuffer) is read through them, any other through episodes()"""
        if self._hip is not None:
            self._hip.dirty = True            # (the parameters change below; the kernels' packed copy is rebuilt at the next call)
        on_device = all(hasattr(sample_buffer, name) for name in ("packed", "last_rows", "returns"))
        batch = self._packed_round(sample_buffer) if on_device else self._episodes_round(sample_buffer)
        if batch is None:
            return [0.0, 0.0, 0.0], 0.0
        view, feature, action, reward = batch
        policy, value = self.net(view, feature)
        log_policy = torch.log(policy + 1e-6)
        log_prob = log_policy.gather(1, action.unsqueeze(1)).squeeze(1)
        advantage = (reward - value).detach()
        pg_loss = -(advantage * log_prob).mean()
        vf_loss = self.value_coef * ((reward - value) ** 2).mean()
        neg_entropy = self.ent_coef * (policy * log_policy).sum(dim=1).mean()
        self.optimizer.zero_grad(set_to_none=True)
        (pg_loss + vf_loss + neg_entropy).backward()
        self.optimizer.step()
        self.train_ct += 1
        losses = [float(x.detach()) for x in (pg_loss, vf_loss, neg_entropy)]
        print("sample", len(reward), *losses)
        return losses, float(value.detach().mean())

    def get_info(self):
        return "a2c train_time: %d" % self.train_ct

    def _path(self, dir_name, name, epoch):
        return os.path.join(dir_name, name, "%s_%d.pt" % (self.subclass_name, epoch))

    def save(self, dir_name, epoch):
        os.makedirs(os.path.join(dir_name, self.name), exist_ok=True)
        torch.save({"net": self.net.state_dict(), "optimizer": self.optimizer.state_dict(), "train_ct": self.train_ct},
                   self._path(dir_name, self.name, epoch))

    def load(self, dir_name, epoch=0, name=None):
        state = torch.load(self._path(dir_name, name or self.name, epoch), map_location=self.device)
        self.net.load_state_dict(state["net"])
        self.optimizer.load_state_dict(state["optimizer"])
        self.train_ct = state.get("train_ct", 0)
        if self._hip is not None:
            self._hip.dirty = True
