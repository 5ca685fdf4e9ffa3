"""DeviceEpisodesBuffer: the episode recorder of a packed EnvBatch, on the device (kernels: magent_amd/csrc/replay.hip, C-ABI:
include/magent_replay.h).

utility.EpisodesBuffer is a host object for one world: it reads the ids back every step and keys agents by bare id.  This recorder takes
what the batched acting path already has -- the packed observation, action and reward buffers, EnvBatch.agent_ids' packed ids and the
packed_segments table --, keys agents by (world, id) as the segmented DRQN table does, and never waits for the host inside a round.  At
the round's end it hands DeepQNetwork.train / DeepRecurrentQNetwork.train / AdvantageActorCritic.train what they already accept:
packed() and episodes() -- and the A2C's discounted returns of the round, computed where it lies: last_rows() and returns()."""
import ctypes
import warnings

import numpy as np
import torch

from . import c_lib

NO_KEY = 0x7FFFFFFFFFFFFFFF      # include/magent_replay.h: REPLAY_NO_KEY
SCAN_BLOCK = 1024                # REPLAY_SCAN_BLOCK
_TRACKED, _COUNTERS = 0, 8       # REPLAY_C_TRACKED, REPLAY_COUNTERS
_FILL = lambda parity: 2 + 2 * parity
_OVERFLOW = lambda parity: 3 + 2 * parity


class ReplayState(ctypes.Structure):
    """include/magent_replay.h: ReplayState"""
    _fields_ = [(name, ctypes.c_void_p) for name in (
        "key_of_slot", "sorted_keys", "sorted_slot", "row_of_slot", "len", "flags", "src_row", "blk", "counters", "log_view", "log_feat",
        "log_act", "log_rew", "log_slot", "log_ord")] + [(name, ctypes.c_int) for name in (
            "capacity", "max_transitions", "view_row_bytes", "feat_row_bytes")]


class DeviceEpisode(object):
    """the transitions of ONE agent during one round, as the models' train() iterate them (utility.EpisodesBufferEntry's fields): views and
    features are tuples of device rows, actions and rewards host arrays"""
    __slots__ = ("views", "features", "actions", "rewards", "terminal")

    def __init__(self, views, features, actions, rewards, terminal):
        self.views, self.features, self.actions, self.rewards, self.terminal = views, features, actions, rewards, terminal


class DeviceEpisodesBuffer(object):
    """Per-agent episode store of ONE side (group) of a packed EnvBatch for ONE round, at most `capacity` agents, kept on the device.

    A round runs from construction or reset() to packed().  Worlds are NOT reset inside a round: a world that is reset numbers its agents
    from 0 again, and they would continue the episodes of the agents that had those ids.

    Keys.  An agent is (segment << 32) | uint32(id); segment s of a call is world s (EnvBatch.packed_segments).  segments=None: one
    world, one segment (0, rows).

    record_step(ids, obs, acts, rewards, segments=None, order=None), once per cycle, after EnvBatch.cycle and before the action buffer
    is overwritten: `ids` int32 [rows] are the ids taken BEFORE that cycle (EnvBatch.agent_ids), `segments` the table taken before it,
    obs = (views, features) the packed tensors the cycle wrote, `acts` the int32 actions it READ, `rewards` the float32 rewards it wrote.
    A row in no segment (a pad row, a stale row behind a world's living agents) is never recorded and never admitted.  Of two rows of
    one segment with the same id the LAST is the agent's.
      Admission (the reference's policy, utility.py:33-77, with the randomness handed in): while fewer than `capacity` agents are tracked,
    the in-segment rows whose keys are not tracked are admitted in the order of `order`, an int32 permutation of the row indices on the
    device (torch.randperm(rows, dtype=torch.int32, device=...)); None: row order.  The slot number is the admission rank; a row admitted
    by a call is recorded by it.  Once full only tracked agents are recorded.
      Death.  The batched cycle reports no alive flags; it compacts.  A tracked agent recorded by call t and absent from call t + 1 died:
    its last transition is terminal.  Every recorded world is therefore described in every call (a segment of count 0 says its agents
    are gone).  close(ids, segments=None) runs the same detection on the ids taken AFTER the last recorded cycle and records nothing;
    without it the agents recorded by the last call end unfinished (mask 0).

    packed() -> (views, features, actions, rewards, terminal, mask) in EpisodesBuffer.packed's order -- slots ascending, each slot's
    transitions in time order -- as torch tensors on the recorder's device (actions int32, rewards float32, terminal bool, mask float32), or
    None when nothing was recorded.  It is the one place that reads a count back from the device.  Views come back in the format given;
    bf16 cells [.., H, W, 8] with view_channels=C as cells[..., :C].float() (exact), which a float32 replay memory takes.
    last_rows() -> (slots, rows): int64 device tensors of the slots with at least one transition, ascending, and the packed row of each
    one's last transition; None when nothing was recorded.  returns(bootstrap, gamma) -> float32 [transitions]: the discounted returns in
    packed()'s order, keep = keep * gamma + reward from every episode's last row to its first, started from bootstrap[slot] (float32
    [tracked] on the device; `tracked` is the count packed() read) -- in double, rounded once to float32: bit for bit what
    AdvantageActorCritic.train computes on the host (include/magent_replay.h: replay_returns).  Both are valid until the next record_step,
    close or reset, as packed() is.
    episodes() / buffer: the per-agent view, built on demand from the packed arrays; buffer is keyed by (segment, id), by id when every
    call had segments=None.  stats() reads back tracked agents, transitions and the overflow flag.  reset() empties the recorder.

    Limits.  `capacity` agents and `max_transitions` rows of storage, allocated once here: about max_transitions x (view row + feature
    row + 16 bytes) of device memory, plus the packed arrays at the round's end.  If a call's transitions do not all fit, that call and
    every later one record nothing at all and detect nothing, and a sticky overflow flag is set -- decided on the device, the host does
    not wait to find out: episodes end unfinished and never have a hole.  packed() then returns what was recorded, with a RuntimeWarning.

    No host wait in record_step / close, and no allocation: the per-row workspace is sized by the first call (and again only if a later
    call has more rows).  The two sorts of an admitting call are torch.sort into preallocated outputs; a call that knows the recorder
    is full -- from a count that arrives without a wait -- skips them.  All work is enqueued on torch's current stream: EnvBatch.cycle
    returns with its outputs complete and agent_ids writes on torch's stream, so no other ordering is needed.

    `lib`: an emulated build of replay.hip (the tests'); the tensors are then CPU tensors."""

    def __init__(self, capacity, max_transitions, view_shape, feature_shape, view_dtype=torch.float32, view_channels=None, device=None, lib=None):
        self.capacity, self.max_transitions = int(capacity), int(max_transitions)
        if self.capacity <= 0 or self.max_transitions <= 0:
            raise ValueError("capacity and max_transitions are positive")
        self.view_shape, self.feature_shape = tuple(int(x) for x in view_shape), tuple(int(x) for x in feature_shape)
        if view_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("views are float32 [.., H, W, C] or bfloat16 cells [.., H, W, 8], not %s" % view_dtype)
        self.view_dtype, self.view_channels = view_dtype, view_channels
        if view_channels is not None and not 0 < int(view_channels) <= self.view_shape[-1]:
            raise ValueError("view_channels %r of a view of %d channels" % (view_channels, self.view_shape[-1]))
        if device is None:
            device = torch.device("cpu") if lib is not None else torch.device("cuda", torch.cuda.current_device())
        d = torch.device(device)
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        self.device = d
        if lib is None:
            if d.type != "cuda":
                raise ValueError("DeviceEpisodesBuffer records on a GPU (utility.EpisodesBuffer is the host recorder)")
            lib = c_lib.load()
        if not getattr(lib, "has_replay_api", False):
            raise RuntimeError("the engine library has no replay_* entries (include/magent_replay.h): rebuild it -- "
                               "python -c 'import __graft_entry__ as g; g.build()'")
        self._lib = lib
        cap, T = self.capacity, self.max_transitions
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=d)
        self._key_of_slot = torch.full((cap,), NO_KEY, dtype=torch.int64, device=d)
        self._sorted_keys = torch.full((cap,), NO_KEY, dtype=torch.int64, device=d)
        self._sorted_slot, self._sorted_slot64 = i32(cap), torch.zeros(cap, dtype=torch.int64, device=d)
        self._row_of_slot, self._len, self._flags, self._src_row = torch.full((cap,), -1, dtype=torch.int32, device=d), i32(cap), i32(cap), i32(cap)
        self._blk, self._counters = i32((cap + SCAN_BLOCK - 1) // SCAN_BLOCK), i32(_COUNTERS)
        self._log_view = torch.zeros((T,) + self.view_shape, dtype=view_dtype, device=d)
        self._log_feat = torch.zeros((T,) + self.feature_shape, dtype=torch.float32, device=d)
        self._log_act, self._log_rew = i32(T), torch.zeros(T, dtype=torch.float32, device=d)
        self._log_slot, self._log_ord = i32(T), i32(T)
        row_bytes = lambda t: t[0].numel() * t.element_size()
        st = self._st = ReplayState()
        for name in ("key_of_slot", "sorted_keys", "sorted_slot", "row_of_slot", "len", "flags", "src_row", "blk", "counters", "log_view", "log_feat",
                     "log_act", "log_rew", "log_slot", "log_ord"):
            setattr(st, name, getattr(self, "_" + name).data_ptr())
        st.capacity, st.max_transitions = cap, T
        st.view_row_bytes, st.feat_row_bytes = row_bytes(self._log_view), row_bytes(self._log_feat)
        self._st_ref = ctypes.byref(st)
        self._rows = 0                   # the rows the per-row workspace takes
        self._one = (np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32))       # the table of a call without segments
        self._new_round()

    # ------------------------------------------------------------------ the round
    def _new_round(self):
        self._calls, self._full, self._keyed, self._packed, self._entries = 0, False, False, False, None
        # the tracked count as the host sees it WITHOUT waiting: a pinned word the device count is copied to behind an admitting call.  It
        # only grows during a round, so a stale value says "not full yet" at worst.  A fresh word per round: a copy of the round before
        # that is still in flight lands in the old one.
        self._probe = torch.zeros(1, dtype=torch.int32, pin_memory=True) if self.device.type == "cuda" else None

    def reset(self):
        """empties the recorder: a new round"""
        self._key_of_slot.fill_(NO_KEY); self._sorted_keys.fill_(NO_KEY)
        self._row_of_slot.fill_(-1)
        self._len.zero_(); self._flags.zero_(); self._counters.zero_()
        self._new_round()

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else None

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d)" % (what, rc))

    def _known_full(self):
        if not self._full:
            seen = int(self._probe[0]) if self._probe is not None else int(self._counters[_TRACKED])
            self._full = seen >= self.capacity
        return self._full

    def _table(self, ids, segments):
        """(n, begin, count, n_seg, rows in segments) of a call; the table validated by hip_policy.check_segments' rules"""
        if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int32 and ids.dim() == 1 and ids.device == self.device and ids.is_contiguous()):
            raise ValueError("ids is a contiguous int32 tensor [rows] on %s" % self.device)
        n = int(ids.shape[0])
        if segments is None:
            begin, count = self._one
            count[0] = n
            return n, begin, count, 1, n
        from .builtin.torch_model.hip_policy import check_segments
        seg = check_segments(segments, n)
        self._keyed = True
        begin, count = np.ascontiguousarray(seg[:, 0], dtype=np.int32), np.ascontiguousarray(seg[:, 1], dtype=np.int32)
        return n, begin, count, len(seg), int(seg[:, 1].sum())

    def _grow(self, n):
        if n > self._rows:
            d = self.device
            self._row_key, self._cand_key, self._cand_sorted, self._cand_pos = (torch.empty(n, dtype=torch.int64, device=d) for _ in range(4))
            self._row_slot, self._first = (torch.empty(n, dtype=torch.int32, device=d) for _ in range(2))
            self._rows = n

    def _find(self, ids, table, order, admit):
        n, begin, count, n_seg, in_seg = table
        lib, st, stream = self._lib, self._st_ref, self._stream()
        ip = ctypes.POINTER(ctypes.c_int32)
        bp, cp = begin.ctypes.data_as(ip), count.ctypes.data_as(ip)
        if admit and in_seg > 0 and not self._known_full():
            self._grow(n)
            if order is not None and not (isinstance(order, torch.Tensor) and order.dtype == torch.int32 and tuple(order.shape) == (n,)
                                          and order.device == self.device and order.is_contiguous()):
                raise ValueError("order is a contiguous int32 permutation [rows] of the row indices on %s" % self.device)
            self._check(lib.replay_find(st, ids.data_ptr(), n, bp, cp, n_seg, self._row_key.data_ptr(), self._row_slot.data_ptr(), 0, stream), "replay_find")
            self._check(lib.replay_candidates(st, self._row_key.data_ptr(), self._row_slot.data_ptr(), None if order is None else order.data_ptr(), n,
                                              self._cand_key.data_ptr(), stream), "replay_candidates")
            torch.sort(self._cand_key[:n], stable=True, out=(self._cand_sorted[:n], self._cand_pos[:n]))
            self._check(lib.replay_admit(st, self._cand_key.data_ptr(), self._cand_sorted.data_ptr(), self._cand_pos.data_ptr(), n, self._first.data_ptr(),
                                         stream), "replay_admit")
            torch.sort(self._key_of_slot, stable=True, out=(self._sorted_keys, self._sorted_slot64))
            self._sorted_slot.copy_(self._sorted_slot64)
            if self._probe is not None:
                self._probe.copy_(self._counters[_TRACKED:_TRACKED + 1], non_blocking=True)
        self._check(lib.replay_find(st, ids.data_ptr(), n, bp, cp, n_seg, None, None, 1, stream), "replay_find")

    def record_step(self, ids, obs, acts, rewards, segments=None, order=None):
        views, feats = obs[0], obs[1]
        table = self._table(ids, segments)
        n = table[0]
        for t, shape, dtype, what in ((views, self.view_shape, self.view_dtype, "views"), (feats, self.feature_shape, torch.float32, "features"),
                                      (acts, (), torch.int32, "acts"), (rewards, (), torch.float32, "rewards")):
            if not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == (n,) + shape and t.device == self.device and t.is_contiguous()):
                raise ValueError("%s is a contiguous %s tensor %s on %s" % (what, dtype, (n,) + shape, self.device))
        self._packed, self._entries = False, None
        self._find(ids, table, order, admit=True)
        self._check(self._lib.replay_step(self._st_ref, self._calls, 1, min(self.capacity, table[4]), views.data_ptr(), feats.data_ptr(), acts.data_ptr(),
                                          rewards.data_ptr(), self._stream()), "replay_step")
        self._calls += 1

    def close(self, ids, segments=None):
        """the deaths between the last recorded cycle and now: `ids` / `segments` as taken AFTER that cycle; records nothing"""
        table = self._table(ids, segments)
        self._packed, self._entries = False, None
        self._find(ids, table, None, admit=False)
        self._check(self._lib.replay_step(self._st_ref, self._calls, 0, 0, None, None, None, None, self._stream()), "replay_step")
        self._calls += 1

    # ------------------------------------------------------------------ the round's end
    def stats(self):
        """{"tracked", "transitions", "overflow"} read back from the device (a host wait)"""
        c = self._counters.cpu().tolist()
        par = self._calls & 1
        return {"tracked": c[_TRACKED], "transitions": c[_FILL(par)], "overflow": bool(c[_OVERFLOW(par)])}

    def packed(self):
        if self._packed is False:
            s = self.stats()
            if s["overflow"]:
                warnings.warn("DeviceEpisodesBuffer: max_transitions = %d rows were not enough: the round was recorded up to the call that did not "
                              "fit, its episodes end unfinished" % self.max_transitions, RuntimeWarning, stacklevel=2)
            n, d = s["transitions"], self.device
            if n == 0:
                self._packed = None
            else:
                views = torch.empty((n,) + self.view_shape, dtype=self.view_dtype, device=d)
                feats = torch.empty((n,) + self.feature_shape, dtype=torch.float32, device=d)
                acts, rews = torch.empty(n, dtype=torch.int32, device=d), torch.empty(n, dtype=torch.float32, device=d)
                terminal, mask = torch.empty(n, dtype=torch.bool, device=d), torch.empty(n, dtype=torch.float32, device=d)
                self._base, dst = torch.empty(self.capacity, dtype=torch.int32, device=d), torch.empty(n, dtype=torch.int32, device=d)
                self._check(self._lib.replay_pack(self._st_ref, n, views.data_ptr(), feats.data_ptr(), acts.data_ptr(), rews.data_ptr(), terminal.data_ptr(),
                                                  mask.data_ptr(), self._base.data_ptr(), dst.data_ptr(), self._stream()), "replay_pack")
                if self.view_channels is not None and self.view_dtype == torch.bfloat16:
                    views = views[..., :self.view_channels].float()
                self._packed = (views, feats, acts, rews, terminal, mask)
            self._tracked = s["tracked"]
        return self._packed

    @property
    def tracked(self):
        """the agents tracked, as packed() read the count: the length of returns()' bootstrap"""
        self.packed()
        return self._tracked

    def last_rows(self):
        if self.packed() is None:
            return None
        t = self._tracked
        lens = self._len[:t].to(torch.int64)
        slots = torch.nonzero(lens > 0).squeeze(1)
        return slots, self._base[:t].to(torch.int64)[slots] + lens[slots] - 1

    def returns(self, bootstrap, gamma):
        if not getattr(self._lib, "has_replay_returns", False):
            raise RuntimeError("the engine library has no replay_returns entry (include/magent_replay.h): rebuild it -- "
                               "python -c 'import __graft_entry__ as g; g.build()'")
        p = self.packed()
        if p is None:
            return None
        t, n = self._tracked, int(p[3].shape[0])
        if not (isinstance(bootstrap, torch.Tensor) and bootstrap.dtype == torch.float32 and tuple(bootstrap.shape) == (t,)
                and bootstrap.device == self.device and bootstrap.is_contiguous()):
            raise ValueError("bootstrap is a contiguous %s tensor %s on %s" % (torch.float32, (t,), self.device))
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        self._check(self._lib.replay_returns(self._st_ref, t, n, self._base.data_ptr(), p[3].data_ptr(), bootstrap.data_ptr(), float(gamma),
                                             out.data_ptr(), self._stream()), "replay_returns")
        return out

    @property
    def buffer(self):
        if self._entries is None:
            entries, p = {}, self.packed()
            if p is not None:
                t = self._tracked
                keys, lens = self._key_of_slot[:t].cpu().numpy(), self._len[:t].cpu().numpy()
                acts, rews, terminal = p[2].cpu().numpy(), p[3].cpu().numpy(), p[4].cpu().numpy()
                at = 0
                for key, m in zip(keys.tolist(), lens.tolist()):
                    seg, aid = key >> 32, ((key & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000      # (the id's 32 bits, signed)
                    entries[(seg, aid) if self._keyed else aid] = DeviceEpisode(
                        p[0][at:at + m].unbind(0), p[1][at:at + m].unbind(0), acts[at:at + m], rews[at:at + m], bool(m and terminal[at + m - 1]))
                    at += m
            self._entries = entries
        return self._entries

    def episodes(self):
        return self.buffer.values()
