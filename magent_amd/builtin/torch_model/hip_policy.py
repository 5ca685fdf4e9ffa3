"""Binding of the hand-written MI355X inference kernels for the reference's deep Q network (include/magent_policy.h,
magent_amd/csrc/policy.hip) to the PyTorch model that owns the parameters (dqn.py: _QNet) -- and, further down, of the float32 kernels,
the recurrent network's (float32 and bf16: one state table, _DrqnPolicy) and the actor-critic's (float32 and bf16).

The kernels want every weight matrix in the operand order of v_mfma_f32_32x32x16_bf16 ("fragment order") and every
activation in the order a lane of the MFMA result holds its 16 outputs ("slot order"); both are plain index permutations of
the torch parameters, done here with tensor ops on the device whenever the parameters have changed: every policy notices by itself that a
parameter was written or replaced since it packed (_SourceStamp), whoever did it -- train(), load(), load_state_dict, an optimiser of
the caller's.  Setting `.dirty = True` forces a repack."""
import ctypes
import os

import numpy as np
import torch

from ... import c_lib


class _Shape(ctypes.Structure):
    _fields_ = [("view_h", ctypes.c_int), ("view_w", ctypes.c_int), ("view_c", ctypes.c_int), ("feat", ctypes.c_int),
                ("n_action", ctypes.c_int)]


class _Weights(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("conv1", "conv2", "dense_view", "dense_emb", "head", "conv2_bias",
                                               "dense_view_bias", "dense_emb_bias")] + [("value_bias", ctypes.c_float)]


def slot_channels(device):
    """channel (output) held in slot s of a 32-wide tile: (s & 3) + 8 ((s & 15) >> 2) + 4 (s >> 4)  (policy_f32_dev.h: out_of)"""
    s = torch.arange(32, device=device)
    return (s & 3) + 8 * ((s & 15) >> 2) + 4 * (s >> 4)


def fragment_order(w):
    """[N (multiple of 32)][K (multiple of 16)] -> bf16 [K / 16][N / 32][64 lanes][8]: lane l of k-step s and tile T holds
    w[32 T + (l & 31)][16 s + 8 (l >> 5) + 0..7]"""
    n, k = w.shape
    assert n % 32 == 0 and k % 16 == 0
    return w.reshape(n // 32, 32, k // 16, 2, 8).permute(2, 0, 3, 1, 4).contiguous().to(torch.bfloat16).reshape(k // 16, n // 32, 64, 8)


CONV1_TAP_ORDER = [0, 3, 1, 4, 2, 5, 6, 7, 8, 9]       # tap (ky * 3 + kx; 9 = padding) in position 2 s + g of conv1's reduction index


class _SourceStamp(object):
    """What a packed copy of a module's parameters was made from: every parameter's storage address and version counter.

    The packed copy is stale when a parameter has been written in place (an optimiser step, load_state_dict, copy_, add_: each bumps the
    tensor's `_version`) or replaced (`.to()`, `.float()`, a new nn.Parameter: another storage address).  The stamp holds the parameters'
    tensors (detached views of the same storage), so a replaced storage stays allocated until the next pack and its address cannot come
    back under a new tensor.  Not seen: a write through `p.data` (it bypasses the version counter) -- the `dirty` flag is for that."""
    __slots__ = ("tensors", "slots")

    def __init__(self, module):
        self.tensors, self.slots = [], []        # slots: (the owning module's parameter dict, name, address, version) -- no tree walk per call
        for m in module.modules():
            for name, p in m._parameters.items():
                if p is not None:
                    t = p.detach()
                    self.tensors.append(t)
                    self.slots.append((m._parameters, name, t.data_ptr(), t._version))

    def differs(self, module):
        for params, name, address, version in self.slots:
            p = params.get(name)
            if p is None or p.data_ptr() != address or p._version != version:
                return True
        return False


class _Packed(object):
    """a policy that keeps a packed copy of its module's parameters (`_source` names the attribute that holds the module) and a workspace
    for the library's calls.  `lib`: a library other than the product's (the tests' emulated build; its "device" memory is the host's,
    so the tensors are CPU tensors)."""
    _source = "qnet"

    def __init__(self, module, view_space, feature_space, n_action, device, chunk, lib=None):
        self._lib = c_lib.declare_policy(lib) if lib is not None else c_lib.load()
        setattr(self, self._source, module)
        self.device, self.chunk = torch.device(device), int(chunk)
        h, w, c = view_space
        self.shape = _Shape(h, w, c, feature_space[0], n_action)
        self._packed, self._work, self._stamp = None, None, None
        self.dirty = True      # (set by a caller: repack whatever the stamp says)

    def stale(self):
        """does the packed copy have to be rebuilt before the next kernel call?  (a dozen address / counter reads per call)"""
        return self.dirty or self._stamp is None or self._stamp.differs(getattr(self, self._source))

    def _set_packed(self, tensors, weights, stamp):
        """(the tensors stay alive as long as the pointers are in use)"""
        self._packed, self._w, self._stamp, self.dirty = tensors, weights, stamp, False

    def _grow_work(self, device, bytes_fn, *args):
        """the workspace on `device`, at least as large as the library's `bytes_fn(shape, *args)` reports"""
        nbytes = ctypes.c_size_t(0)
        bytes_fn(ctypes.byref(self.shape), *args, ctypes.byref(nbytes))
        if self._work is None or self._work.numel() < nbytes.value:
            self._work = torch.empty(nbytes.value, dtype=torch.uint8, device=device)

    def _chunked(self, name, n, chunk, call):
        """call(beg, m) -> the library's return code, for every chunk of at most `chunk` of the n agents"""
        for beg in range(0, n, max(chunk, 1)):
            rc = call(beg, min(chunk, n - beg))
            if rc != 0:
                raise RuntimeError("%s failed (%d)" % (name, rc))


def acting_policy(infer_dtype, device, bf16_class, f32_class, *args, f32_after_bf16=True):
    """what a model's constructor needs to act through the kernels: (infer_dtype, policy or None, bf16_kernels).
    infer_dtype: the argument, else MAGENT_POLICY_DTYPE, else "f32"; validated.  On a CUDA device the policy is the first of bf16_class
    (asked for by "bf16") and f32_class (unless MAGENT_POLICY_F32=torch; behind the bf16 class only if f32_after_bf16) whose constructor
    takes `args`: an unsupported shape (ValueError) or a library without these kernels (OSError, AttributeError) passes to the next;
    None: the PyTorch network acts.  bf16_kernels: the policy is the bf16 class's."""
    infer_dtype = (infer_dtype or os.environ.get("MAGENT_POLICY_DTYPE", "f32")).lower()
    if infer_dtype not in ("f32", "bf16"):
        raise ValueError("infer_dtype must be 'f32' or 'bf16', not %r" % (infer_dtype,))
    kinds = [bf16_class] if infer_dtype == "bf16" else []
    if (f32_after_bf16 or not kinds) and os.environ.get("MAGENT_POLICY_F32", "hip").lower() != "torch":
        kinds.append(f32_class)
    if torch.device(device).type == "cuda":
        for kind in kinds:
            try:
                return infer_dtype, kind(*args), kind is bf16_class
            except (ValueError, OSError, AttributeError):
                pass
    return infer_dtype, None, False


def _stream(device):
    """torch's current stream on a CUDA device; None (the null stream) for the emulated library's CPU tensors"""
    return torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else None


def _ptr(t):
    return None if t is None else t.data_ptr()


def _set_pointers(struct, tensors, keys=None):
    """the addresses of `tensors` (a dict; `keys`: some of it) into the same-named fields of a ctypes struct"""
    for k in (tensors if keys is None else keys):
        setattr(struct, k, tensors[k].data_ptr())


def _head_32x512(rows, device, biases=()):
    """the padded head [32][512] (and its bias [32]) from (first output row, weight [r][512]) pairs (and (first row, bias [r]) pairs)"""
    head, hb = torch.zeros(32, 512, device=device), torch.zeros(32, device=device)
    for at, w in rows:
        head[at:at + w.shape[0]] = w.detach().float()
    for at, b in biases:
        hb[at:at + b.shape[0]] = b.detach().float()
    return head, hb


def _pad_k(w, k):
    return torch.cat([w, w.new_zeros(w.shape[0], k - w.shape[1])], dim=1) if w.shape[1] < k else w


def _conv1_cells(q, c):
    """conv1 of a trunk as [32][ky][kx][8], K = tap * 8 + channel: the C channels padded to a cell's 8, the bias as the weight of channel 7
    of tap 0 (the kernels feed a constant 1.0 there: the MFMA adds the bias)"""
    w1 = q.conv1.weight.detach().float()                              # [32][C][3][3]
    w1 = torch.cat([w1, w1.new_zeros(32, 8 - c, 3, 3)], dim=1).permute(0, 2, 3, 1).contiguous()
    w1[:, 0, 0, 7] = q.conv1.bias.detach().float()
    return w1


def _trunk_bf16(q, shape, dev):
    """conv1, conv2, dense_view, dense_emb of a _QNet / _RecurrentQNet (the same trunk) in bf16 fragment order with their biases in slot
    order, and `hidden`: the hidden unit held in each of the 512 hidden slots (the order the kernels keep the hidden layer in)"""
    ch = slot_channels(dev)
    k_dense = (shape.view_h - 4) * (shape.view_w - 4) * 32
    # the kernel pairs the taps (0|3) (1|4) (2|5) (6|7) (8|pad) into its five k-steps (policy.hip: k_dqn_conv)
    w1 = _pad_k(_conv1_cells(q, shape.view_c).reshape(32, 72), 80).reshape(32, 10, 8)[:, CONV1_TAP_ORDER].reshape(32, 80)
    w2 = q.conv2.weight.detach().float()[:, ch].permute(0, 2, 3, 1).reshape(32, 288)            # K = tap * 32 + slot
    wv = q.dense_view.weight.detach().float().reshape(256, -1, 32)[:, :, ch].reshape(256, k_dense)   # K = position * 32 + slot
    fk = (shape.feat + 15) // 16 * 16
    we = _pad_k(q.dense_emb.weight.detach().float(), fk)
    hidden = (torch.arange(16, device=dev)[:, None] * 32 + ch[None, :]).reshape(512)              # hidden slot -> hidden unit
    return {
        "conv1": fragment_order(w1), "conv2": fragment_order(w2), "dense_view": fragment_order(wv),
        "dense_emb": fragment_order(we),
        "conv2_bias": q.conv2.bias.detach().float()[ch].contiguous(),
        "dense_view_bias": q.dense_view.bias.detach().float()[hidden[:256]].contiguous(),
        "dense_emb_bias": q.dense_emb.bias.detach().float()[hidden[:256]].contiguous(),
    }, hidden


class _DqnPolicy(_Packed):
    """what the two DQN policies share: the constructor's check, the head around a packed trunk and the chunked step.  A subclass names
    its entries of the library (`_abi`: supported, act_bytes, the entry named in errors, the kernels named in errors) and gives pack() /
    infer()."""
    _abi = None

    def __init__(self, qnet, view_space, feature_space, n_action, device, chunk=131072):
        super().__init__(qnet, view_space, feature_space, n_action, device, chunk)
        if not (qnet.use_conv and qnet.use_dueling) or not getattr(self._lib, self._abi[0])(ctypes.byref(self.shape)):
            raise ValueError("network shape not taken by the %s" % self._abi[3])
        self.k_dense = (view_space[0] - 4) * (view_space[1] - 4) * 32

    def _pack_head(self, t, stamp, frag, hidden=None):
        """the dueling head into `t` (a packed trunk; hidden: the hidden unit in each position of the kernels' hidden layer, None: natural
        order) and the whole into the library's struct"""
        q = self.qnet
        head, _ = _head_32x512([(0, q.advantage.weight), (self.shape.n_action, q.value.weight)], self.device)
        t["head"] = frag(head if hidden is None else head[:, hidden])
        w = _Weights()
        _set_pointers(w, t)
        w.value_bias = float(q.value.bias.detach().float().item())
        self._set_packed(t, w, stamp)

    def _step(self, entry, view, feature, want_q):
        """the library's `entry` on every chunk of the call"""
        call = getattr(self._lib, entry)
        if self.stale():
            self.pack()
        n = view.shape[0]
        actions = torch.empty(n, dtype=torch.int32, device=view.device)
        q = torch.empty((n, self.shape.n_action), dtype=torch.float32, device=view.device) if want_q else None
        self._grow_work(view.device, getattr(self._lib, self._abi[1]), min(n, self.chunk))      # (activations in the kernels' own layout + the conv kernel's dump line)
        stream = _stream(view.device)
        self._chunked(self._abi[2], n, self.chunk, lambda beg, m: call(
            ctypes.byref(self.shape), ctypes.byref(self._w), view[beg:].data_ptr(), feature[beg:].data_ptr(), m, self._work.data_ptr(),
            actions[beg:].data_ptr(), _ptr(q[beg:] if want_q else None), stream))
        return (actions, q) if want_q else actions


class HipDqnPolicy(_DqnPolicy):
    """greedy actions (and, for tests, the Q values) of a dueling conv _QNet, computed by k_dqn_conv + k_dqn_head"""
    _abi = ("policy_dqn_supported", "policy_dqn_act_bytes", "policy_dqn_infer", "HIP policy kernels")

    @torch.no_grad()
    def pack(self):
        stamp = _SourceStamp(self.qnet)
        t, hidden = _trunk_bf16(self.qnet, self.shape, self.device)
        self._pack_head(t, stamp, fragment_order, hidden)

    @torch.no_grad()
    def infer(self, view, feature, want_q=False):
        """view float32 [n][H][W][C] -- or bfloat16 [n][H][W][8], the engine's cells (GridWorld.get_observation_device_bf16) --,
        feature float32 [n][F]: contiguous CUDA tensors.  Returns int32 actions [n] (and Q [n][A])"""
        cells16 = view.dtype == torch.bfloat16
        assert view.is_cuda and view.is_contiguous() and feature.is_contiguous() and feature.dtype == torch.float32
        assert (cells16 and view.shape[-1] == 8) or (view.dtype == torch.float32 and view.shape[-1] == self.shape.view_c)
        return self._step("policy_dqn_infer_bf16" if cells16 else "policy_dqn_infer", view, feature, want_q)


# ---------------------------------------------------------------------------------------------------- float32 (the reference's arithmetic)
def fragment_order_f32(w):
    """[N (multiple of 32)][K (multiple of 8)] -> float32 [K / 8][N / 32][64 lanes][4]: lane l of group m and tile T holds
    w[32 T + (l & 31)][8 m + 4 (l >> 5) + 0..3]  (include/magent_policy.h: "f32 fragment order")"""
    n, k = w.shape
    assert n % 32 == 0 and k % 8 == 0
    return w.reshape(n // 32, 32, k // 8, 2, 4).permute(2, 0, 3, 1, 4).contiguous().float().reshape(k // 8, n // 32, 64, 4)


def _trunk_f32(q, shape, dev):
    """conv1, conv2, dense_view, dense_emb of a _QNet / _RecurrentQNet (the same trunk) in f32 fragment order, with their biases"""
    w1 = _conv1_cells(q, shape.view_c)
    w2 = q.conv2.weight.detach().float().permute(0, 2, 3, 1).reshape(32, 288)                      # K = tap * 32 + channel
    wv = q.dense_view.weight.detach().float()                                                      # K = position * 32 + channel (NHWC flatten)
    fk = (shape.feat + 7) // 8 * 8
    we = _pad_k(q.dense_emb.weight.detach().float(), fk)
    return {
        "conv1": fragment_order_f32(w1.reshape(32, 72)), "conv2": fragment_order_f32(w2), "dense_view": fragment_order_f32(wv),
        "dense_emb": fragment_order_f32(we),
        "conv2_bias": q.conv2.bias.detach().float().contiguous(),
        "dense_view_bias": q.dense_view.bias.detach().float().contiguous(),
        "dense_emb_bias": q.dense_emb.bias.detach().float().contiguous(),
    }


class HipDqnPolicyF32(_DqnPolicy):
    """greedy actions (and the Q values) of a dueling conv _QNet in float32 -- inputs, weights, activations, accumulation: the reference
    network's own arithmetic -- computed by k_dqn_conv_f32 + k_dqn_head_f32 on v_mfma_f32_32x32x2_f32 (magent_amd/csrc/policy_f32.hip)"""
    _abi = ("policy_dqn_f32_supported", "policy_dqn_f32_act_bytes", "policy_dqn_infer_f32", "HIP f32 policy kernels")

    @torch.no_grad()
    def pack(self):
        stamp = _SourceStamp(self.qnet)
        self._pack_head(_trunk_f32(self.qnet, self.shape, self.device), stamp, fragment_order_f32)

    @torch.no_grad()
    def infer(self, view, feature, want_q=False):
        """view float32 [n][H][W][C], feature float32 [n][F]: contiguous CUDA tensors (the engine's observation tensors as they are).
        Returns int32 actions [n] (and Q [n][A])"""
        assert view.is_cuda and view.is_contiguous() and feature.is_contiguous() and view.dtype == torch.float32 and feature.dtype == torch.float32
        assert view.shape[-1] == self.shape.view_c
        return self._step("policy_dqn_infer_f32", view, feature, want_q)


# ---------------------------------------------------------------------------------------------------- the recurrent network (drqn.py)
class _DrqnWeights(ctypes.Structure):
    _fields_ = [("trunk", _Weights), ("gru", ctypes.c_void_p), ("gru_bias", ctypes.c_void_p), ("gru_bias0", ctypes.c_void_p),
                ("head", ctypes.c_void_p), ("head_bias", ctypes.c_void_p), ("dueling", ctypes.c_int)]


class _DrqnPolicy(_Packed):
    """what the two DRQN policies share: the GRU state of every agent id in device memory, the packing of the GRU and the head around a
    trunk, and the chunked step.  A subclass names its entries of the library (`_abi`: supported, workspace_bytes) and gives pack() / infer().

    The state table is the last call's output: its ids in call order, their states float32 [.][512] (row k: the k-th id's), and for the
    next call's lookup the ids sorted stably with their rows.  An id of the next call takes the state of its last occurrence in the table,
    any other id starts from zeros; ids absent from the call drop out (drqn.py: the dict path's semantics).  Both kernel paths keep this
    one format: a table can be handed from one to the other (states_dict / load_states).  `lib`: _Packed.

    `segments` (infer): an int array [n_seg][2] of (begin, count) rows -- the worlds of a packed EnvBatch buffer (EnvBatch.packed_segments),
    each numbering its agents from 0.  The table is then keyed by (segment, id): segment s of the call is world s, and the table's second
    format holds int64 keys (segment << 32) | uint32(id) (`_keys` in call order, `_sorted` their stable sort) where the plain one holds
    int32 ids.  One look-up launch (policy_drqn_lookup_seg*) over all n rows finds every row's previous state; the steps then run per
    chunk through the *_rows entries (a chunk may cut a segment: rows are independent); one stable sort of the keys follows.  A segment's
    rows have the bits of a plain call on those rows alone with that world's own table.  A row in no segment (pad, stale) starts from
    zeros, its action is returned, and its state enters the table under NO_KEY, which no look-up produces and which sorts to the end:
    nothing is dropped, so nothing waits for the host.  More than MAX_SEGMENTS segments: several look-ups, cut at segment boundaries.
    Between the forms: a plain table read by a segmented call is segment 0's; a segmented table read by a plain call keeps segment 0's
    entries and drops the rest (that conversion reads the keys back: it waits for the device once)."""
    STATE = 512
    NO_KEY = 0x7FFFFFFFFFFFFFFF
    _abi = None

    def __init__(self, qnet, view_space, feature_space, n_action, device, chunk=131072, lib=None):
        super().__init__(qnet, view_space, feature_space, n_action, device, chunk, lib)
        supported = getattr(self._lib, self._abi[0])          # (AttributeError: a library without these kernels)
        if qnet.rnn.hidden_size != self.STATE or not supported(ctypes.byref(self.shape)):
            raise ValueError("network shape not taken by the HIP DRQN kernels (%s)" % self._abi[0])
        self.clear()

    # ---- the state table
    def clear(self):
        z = torch.zeros(0, dtype=torch.int32, device=self.device)
        self._ids, self._sorted, self._rows = z, z, z
        self._keys = None                # (not None: the (segment, id) format -- _sorted is then int64, _ids None)
        self._states = torch.zeros((0, self.STATE), device=self.device)

    def _set_table(self, ids, states):
        self._ids, self._states, self._keys = ids, states, None
        self._sorted, perm = torch.sort(ids, stable=True)
        self._rows = perm.to(torch.int32)

    def _set_keyed_table(self, keys, states):
        """the (segment, id) format: int64 keys in call order, their states"""
        self._ids, self._states, self._keys = None, states, keys
        self._sorted, perm = torch.sort(keys, stable=True)
        self._rows = perm.to(torch.int32)

    def _to_keyed(self):
        """a plain table becomes segment 0's (no host wait)"""
        if self._keys is None:
            self._set_keyed_table(self._ids.to(torch.int64) & 0xFFFFFFFF, self._states)

    def _to_plain(self):
        """a (segment, id) table keeps segment 0's entries under their ids and drops the rest (waits for the device: the count)"""
        if self._keys is not None:
            keep = (self._keys >> 32) == 0
            ids = self._keys[keep].view(torch.int32).reshape(-1, 2)[:, 0].contiguous()        # (the low word: little-endian)
            self._set_table(ids, self._states[keep].contiguous())

    def forget_segments(self, segments):
        """the states of these segments (ints) are forgotten -- a world of the batch that was reset numbers its agents from 0 again, and they
        start from zeros: the segments' keys become NO_KEY and the table is sorted again.  No host wait."""
        segments = sorted(set(int(s) for s in segments))
        if not segments or self._sorted.numel() == 0:
            return
        if self._keys is None:
            if 0 in segments:
                self.clear()
            return
        gone = torch.isin(self._keys >> 32, torch.tensor(segments, dtype=torch.int64, device=self._keys.device))
        self._set_keyed_table(torch.where(gone, torch.full_like(self._keys, self.NO_KEY), self._keys), self._states)

    def states_dict(self):
        """{id: state [512]} as the dict path keeps it (insertion in call order, a duplicated id's last row); after a segmented call
        {(segment, id): state}, the rows in no segment left out"""
        if self._keys is None:
            return {int(i): self._states[k] for k, i in enumerate(self._ids.tolist())}
        out = {}
        for k, key in enumerate(self._keys.tolist()):
            if key != self.NO_KEY:
                low = key & 0xFFFFFFFF
                out[(key >> 32, low - (1 << 32) if low >= (1 << 31) else low)] = self._states[k]
        return out

    def load_states(self, mapping):
        """the table from a {id: state} or {(segment, id): state} mapping (an empty one empties it; with tuple keys, an int key is
        segment 0's)"""
        if len(mapping) == 0:
            self.clear()
            return
        states = torch.stack([torch.as_tensor(v).to(self.device, torch.float32).reshape(self.STATE) for v in mapping.values()]).contiguous()
        if any(isinstance(k, tuple) for k in mapping.keys()):
            pairs = [k if isinstance(k, tuple) else (0, k) for k in mapping.keys()]
            keys = torch.tensor([(int(s) << 32) | (int(i) & 0xFFFFFFFF) for s, i in pairs], dtype=torch.int64, device=self.device)
            self._set_keyed_table(keys, states)
        else:
            ids = torch.tensor([int(k) for k in mapping.keys()], dtype=torch.int32, device=self.device)
            self._set_table(ids, states)

    # ---- weights
    def _pack_recurrent(self, t, stamp, frag, x_order=None, round_to=None):
        """the GRU and the head into `t` (a packed trunk) and the whole into the library's struct.  frag: the fragment order of the matrix
        operands; x_order: the hidden unit in each position of the trunk's x (None: natural order); round_to: the operands' dtype, for
        gru_bias0 (a weight that is finite in float32 can round to Inf)"""
        q, dev, S, A = self.qnet, self.device, self.STATE, self.shape.n_action
        rnn = q.rnn
        wih, whh = rnn.weight_ih_l0.detach().float(), rnn.weight_hh_l0.detach().float()        # [3 S][S], gates r, z, n
        bih, bhh = rnn.bias_ih_l0.detach().float(), rnn.bias_hh_l0.detach().float()
        if x_order is not None:
            wih = wih[:, x_order]
        wcat = torch.cat([wih, whh], dim=1).reshape(3, S // 32, 32, 2 * S).permute(1, 0, 2, 3).reshape(3 * S, 2 * S)   # tile 3 T + gate
        t["gru"] = frag(wcat)
        bias = lambda bh: torch.stack([bih[:S] + bh[:S], bih[S:2 * S] + bh[S:2 * S], bih[2 * S:], bh[2 * S:]]).contiguous()
        t["gru_bias"] = bias(bhh)
        # a zero state: W_h 0 is 0, or NaN where a row of W_h (as the kernels hold it) is not finite (torch's W_h @ 0)
        held = whh if round_to is None else whh.to(round_to).float()
        w0 = torch.where(torch.isfinite(held).all(dim=1), torch.zeros_like(bhh), torch.full_like(bhh, float("nan")))
        t["gru_bias0"] = bias(bhh + w0)
        if q.use_dueling:
            head, hb = _head_32x512([(0, q.advantage.weight), (A, q.value.weight)], dev, [(A, q.value.bias)])
        else:
            head, hb = _head_32x512([(0, q.value.weight)], dev, [(0, q.value.bias)])
        t["head"], t["head_bias"] = frag(head), hb
        w = _DrqnWeights()
        _set_pointers(w.trunk, t, ("conv1", "conv2", "dense_view", "dense_emb", "conv2_bias", "dense_view_bias", "dense_emb_bias"))
        _set_pointers(w, t, ("gru", "gru_bias", "gru_bias0", "head", "head_bias"))
        w.dueling = int(bool(q.use_dueling))
        self._set_packed(t, w, stamp)

    # ---- one step
    def _step(self, entry, view, feature, ids, want_q, segments=None):
        """the library's `entry` on every chunk of the call (all chunks read the same previous table), then the new table; with
        `segments` the look-up launch, then `entry`_rows on every chunk"""
        assert view.device == feature.device == ids.device and view.device.type == self.device.type
        assert view.is_contiguous() and feature.is_contiguous() and feature.dtype == torch.float32
        assert ids.dtype == torch.int32 and view.shape[0] == feature.shape[0] == ids.shape[0]
        n, dev = view.shape[0], view.device
        seg = None if segments is None else check_segments(segments, n)
        call = getattr(self._lib, entry if seg is None else entry + "_rows")
        if self.stale():
            self.pack()
        actions = torch.empty(n, dtype=torch.int32, device=dev)
        q = torch.empty((n, self.shape.n_action), dtype=torch.float32, device=dev) if want_q else None
        new_states = torch.empty((n, self.STATE), dtype=torch.float32, device=dev)
        self._grow_work(dev, getattr(self._lib, self._abi[1]), min(n, self.chunk))
        stream = _stream(dev)
        if seg is not None:
            self._to_keyed()
            ids = ids.contiguous()
            count = int(self._sorted.numel())
            from_row = torch.empty(n, dtype=torch.int32, device=dev)
            keys = torch.empty(n, dtype=torch.int64, device=dev)
            lookup = getattr(self._lib, self._abi[2])
            for k in (range(0, len(seg), MAX_SEGMENTS) or [0]):      # one look-up per MAX_SEGMENTS segments, cut at segment boundaries:
                part = seg[k:k + MAX_SEGMENTS]                       # rows from its first segment's begin (the first: row 0) to the next's
                r0 = 0 if k == 0 else int(part[0, 0])
                r1 = n if k + MAX_SEGMENTS >= len(seg) else int(seg[k + MAX_SEGMENTS, 0])
                if r1 > r0:
                    begin = (ctypes.c_int32 * max(len(part), 1))(*(part[:, 0] - r0).tolist())
                    cnt = (ctypes.c_int32 * max(len(part), 1))(*part[:, 1].tolist())
                    rc = lookup(ids[r0:].data_ptr(), r1 - r0, begin, cnt, len(part), k, _ptr(self._sorted if count else None),
                                _ptr(self._rows if count else None), count, from_row[r0:].data_ptr(), keys[r0:].data_ptr(), stream)
                    if rc != 0:
                        raise RuntimeError("%s failed (%d)" % (self._abi[2], rc))
            states = self._states.data_ptr() if count else None
            self._chunked(entry + "_rows", n, self.chunk, lambda beg, m: call(
                ctypes.byref(self.shape), ctypes.byref(self._w), view[beg:].data_ptr(), feature[beg:].data_ptr(), m, from_row[beg:].data_ptr(),
                states, new_states[beg:].data_ptr(), self._work.data_ptr(), actions[beg:].data_ptr(), _ptr(q[beg:] if want_q else None), stream))
            self._set_keyed_table(keys, new_states)
            return (actions, q) if want_q else actions
        self._to_plain()
        ids = ids.clone(memory_format=torch.contiguous_format)        # (the table keeps it: the caller's buffer may be reused)
        count = int(self._sorted.numel())
        table = (self._sorted.data_ptr(), self._rows.data_ptr(), self._states.data_ptr()) if count else (None, None, None)
        self._chunked(entry, n, self.chunk, lambda beg, m: call(
            ctypes.byref(self.shape), ctypes.byref(self._w), view[beg:].data_ptr(), feature[beg:].data_ptr(), m, ids[beg:].data_ptr(),
            table[0], table[1], table[2], count, new_states[beg:].data_ptr(), self._work.data_ptr(), actions[beg:].data_ptr(),
            _ptr(q[beg:] if want_q else None), stream))
        self._set_table(ids, new_states)
        return (actions, q) if want_q else actions


class HipDrqnPolicyF32(_DrqnPolicy):
    """one acting step of a _RecurrentQNet in float32 -- the DQN's trunk (k_dqn_conv_f32 + k_dqn_head_f32), a GRU(512) cell (k_drqn_gru_f32),
    the head and argmax (k_drqn_head_f32): magent_amd/csrc/policy_drqn_f32.hip -- and the GRU state of every agent id in device memory
    (_DrqnPolicy)."""
    _abi = ("policy_drqn_f32_supported", "policy_drqn_f32_workspace_bytes", "policy_drqn_lookup_seg_f32")

    @torch.no_grad()
    def pack(self):
        stamp = _SourceStamp(self.qnet)
        self._pack_recurrent(_trunk_f32(self.qnet, self.shape, self.device), stamp, fragment_order_f32)

    @torch.no_grad()
    def infer(self, view, feature, ids, want_q=False, segments=None):
        """view float32 [n][H][W][C], feature float32 [n][F] (contiguous, on the policy's device), ids int32 [n] on that device.
        Enqueues the step on torch's current stream and replaces the state table; returns int32 actions [n] (and Q [n][A]).
        segments: the (begin, count) rows of the worlds of a packed call, each with its own ids (_DrqnPolicy); None: the plain call"""
        assert view.dtype == torch.float32 and view.shape[-1] == self.shape.view_c
        return self._step("policy_drqn_infer_f32", view, feature, ids, want_q, segments)


class HipDrqnPolicy(_DrqnPolicy):
    """one acting step of a _RecurrentQNet with bf16 matrix operands -- the bf16 DQN's trunk (k_dqn_conv + k_dqn_head stopped after the
    hidden layer), the GRU cell (k_drqn_gru_bf16), the head and argmax (k_drqn_head_bf16): magent_amd/csrc/policy_drqn_bf16.hip.  Gates,
    blend and the state table are float32 (_DrqnPolicy): the rounding points are listed in include/magent_policy.h."""
    _abi = ("policy_drqn_supported", "policy_drqn_workspace_bytes", "policy_drqn_lookup_seg")

    @torch.no_grad()
    def pack(self):
        stamp = _SourceStamp(self.qnet)
        t, hidden = _trunk_bf16(self.qnet, self.shape, self.device)
        self._pack_recurrent(t, stamp, fragment_order, x_order=hidden, round_to=torch.bfloat16)

    @torch.no_grad()
    def infer(self, view, feature, ids, want_q=False, segments=None):
        """view float32 [n][H][W][C] -- or bfloat16 [n][H][W][8], the engine's cells (GridWorld.get_observation_device_bf16) --, feature
        float32 [n][F] (contiguous, on the policy's device), ids int32 [n] on that device.  Enqueues the step on torch's current stream
        and replaces the state table; returns int32 actions [n] (and Q [n][A]).  segments: as HipDrqnPolicyF32.infer"""
        cells16 = view.dtype == torch.bfloat16
        assert (cells16 and view.shape[-1] == 8) or (view.dtype == torch.float32 and view.shape[-1] == self.shape.view_c)
        return self._step("policy_drqn_infer_bf16" if cells16 else "policy_drqn_infer", view, feature, ids, want_q, segments)


# ---------------------------------------------------------------------------------------------------- the actor-critic (a2c.py)
class _A2cWeights(ctypes.Structure):
    _fields_ = [("dense_view", ctypes.c_void_p), ("dense_emb", ctypes.c_void_p), ("dense", ctypes.c_void_p), ("comm", ctypes.c_void_p * 2),
                ("head", ctypes.c_void_p), ("dense_view_bias", ctypes.c_void_p), ("dense_emb_bias", ctypes.c_void_p),
                ("dense_bias", ctypes.c_void_p), ("head_bias", ctypes.c_void_p), ("use_comm", ctypes.c_int)]


class _A2cWeightsBf16(ctypes.Structure):
    _fields_ = [("dense_view", ctypes.c_void_p), ("dense_view_cells", ctypes.c_void_p), ("dense_emb", ctypes.c_void_p), ("dense", ctypes.c_void_p),
                ("comm", ctypes.c_void_p * 2), ("head", ctypes.c_void_p), ("dense_view_bias", ctypes.c_void_p),
                ("dense_emb_bias", ctypes.c_void_p), ("dense_bias", ctypes.c_void_p), ("head_bias", ctypes.c_void_p), ("use_comm", ctypes.c_int)]


MAX_SEGMENTS = 256          # include/magent_policy.h: POLICY_A2C_MAX_SEGMENTS, the most segments of one C call


def check_segments(segments, n):
    """the (begin, count) table of a segmented A2C call over n rows as int64 [n_seg][2], validated as the library validates it
    (include/magent_policy.h: policy_a2c_infer_f32_seg): ValueError naming the first offending segment"""
    if isinstance(segments, torch.Tensor):
        segments = segments.cpu().numpy()
    seg = np.asarray(segments)
    if seg.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if seg.ndim != 2 or seg.shape[1] != 2 or seg.dtype.kind not in "iu":
        raise ValueError("segments is an integer array [n_seg][2] of (begin, count), not %s %s" % (seg.dtype, seg.shape))
    seg = seg.astype(np.int64)
    at = 0
    for k, (b, c) in enumerate(seg.tolist()):
        if b < 0 or c < 0:
            raise ValueError("segment %d (begin %d, count %d): negative" % (k, b, c))
        if b + c > n:
            raise ValueError("segment %d (begin %d, count %d) ends past the call's %d rows" % (k, b, c, n))
        if b < at:
            raise ValueError("segment %d (begin %d, count %d) starts before the end of segment %d (row %d): segments ascend without overlap" % (k, b, c, k - 1, at))
        at = b + c
    return seg


class _A2cPolicy(_Packed):
    """what the two A2C policies share: the constructor's check, the packing of the dense layers, the CommNet steps and the heads, and the
    chunked step.  A subclass names its entries of the library (`_abi`: supported, workspace_bytes, the kernels named in errors) and its
    struct (`_struct`) and gives pack() / infer().

    The draw is the inverse CDF of one uniform number per agent (include/magent_policy.h: policy_a2c_infer_f32).  Without CommNet a call
    of n agents goes to the kernels `chunk` agents at a time (every agent's row is its own).  With CommNet the mean of the other agents
    spans the call, so the whole n goes to ONE C call whatever `chunk` is: the column sums are then taken over the same blocks of agents
    in the same order, and the result does not depend on `chunk`.  `lib`: _Packed.

    `segments` (infer): an int array [n_seg][2] of (begin, count) rows -- the environments of a packed EnvBatch buffer
    (EnvBatch.packed_segments).  Every CommNet mean then runs over the rows of the agent's own segment; a row in no segment (pad, stale)
    is alone: others = 0, its action is in range, nobody's mean sees it.  A segment's outputs have the bits of a plain call on that
    segment's rows alone.  The call still goes to the library whole -- one C call per MAX_SEGMENTS segments, cut at segment boundaries
    (segments are independent; the rows between two cuts go with the call in front).  Without CommNet the table is validated and changes
    nothing.  None: the plain call."""
    _source = "net"
    _abi = _struct = None

    def __init__(self, net, view_space, feature_space, n_action, device, chunk=131072, lib=None):
        super().__init__(net, view_space, feature_space, n_action, device, chunk, lib)
        self.use_comm = net.comm is not None
        region = getattr(self._lib, self._abi[0])(ctypes.byref(self.shape))        # (AttributeError: a library without these kernels)
        if net.dense.in_features != 512 or net.dense.out_features != 512 or not region:
            raise ValueError("network shape not taken by the HIP %s A2C kernels" % self._abi[2])
        self.cells = bool(region & 2)          # (a bf16 cell entry: bit 2 of the bf16 kernels' region, never of the f32 kernels')

    def _pack_dense(self, frag, k_multiple, extra=None):
        """the whole network in `frag` order with K padded to `k_multiple`; extra(t, wv): a subclass's further entries of the struct"""
        net, dev, A = self.net, self.device, self.shape.n_action
        stamp = _SourceStamp(net)
        up = lambda k: (k + k_multiple - 1) // k_multiple * k_multiple
        wv = net.dense_view.weight.detach().float()                              # [256][H W C], K in the view's own order
        t = {
            "dense_view": frag(_pad_k(wv, up(wv.shape[1]))),
            "dense_emb": frag(_pad_k(net.dense_emb.weight.detach().float(), up(self.shape.feat))),
            "dense": frag(net.dense.weight.detach().float()),
            "dense_view_bias": net.dense_view.bias.detach().float().contiguous(),
            "dense_emb_bias": net.dense_emb.bias.detach().float().contiguous(),
            "dense_bias": net.dense.bias.detach().float().contiguous(),
        }
        if extra is not None:
            extra(t, wv)
        head, hb = _head_32x512([(0, net.policy.weight), (A, net.value.weight)], dev, [(0, net.policy.bias), (A, net.value.bias)])
        t["head"], t["head_bias"] = frag(head), hb
        w = self._struct()
        _set_pointers(w, t)
        if self.use_comm:
            for k, step in enumerate(net.comm):         # K = the others' mean (C), then the agent's own units (H)
                t["comm%d" % k] = frag(torch.cat([step.C.weight.detach().float(), step.H.weight.detach().float()], dim=1))
                w.comm[k] = t["comm%d" % k].data_ptr()
        w.use_comm = int(self.use_comm)
        self._set_packed(t, w, stamp)

    def _step(self, entry, view, feature, u, want_policy, want_value, segments=None):
        """the library's `entry` on every chunk of the call (CommNet: on the whole call; with `segments`, its segmented form)"""
        assert view.device == feature.device and view.device.type == self.device.type
        assert view.is_contiguous() and feature.is_contiguous() and feature.dtype == torch.float32 and view.shape[0] == feature.shape[0]
        if self.stale():
            self.pack()
        n, dev, A = view.shape[0], view.device, self.shape.n_action
        if u is None:
            u = torch.rand(n, device=dev)
        assert u.device == dev and u.dtype == torch.float32 and u.is_contiguous() and u.shape == (n,)
        actions = torch.empty(n, dtype=torch.int32, device=dev)
        policy = torch.empty((n, A), dtype=torch.float32, device=dev) if want_policy else None
        value = torch.empty(n, dtype=torch.float32, device=dev) if want_value else None
        out = (actions,) + ((policy,) if want_policy else ()) + ((value,) if want_value else ())
        stream = _stream(dev)

        def piece(name, r0, m, *table):      # the library's `name` on rows r0 .. r0 + m - 1; table: a segmented entry's begin, count, n_seg
            rc = getattr(self._lib, name)(
                ctypes.byref(self.shape), ctypes.byref(self._w), view[r0:].data_ptr(), feature[r0:].data_ptr(), m, u[r0:].data_ptr(),
                self._work.data_ptr(), actions[r0:].data_ptr(), _ptr(policy[r0:] if want_policy else None),
                _ptr(value[r0:] if want_value else None), stream, *table)
            if rc != 0:
                raise RuntimeError("%s failed (%d)" % (name, rc))

        seg = None if segments is None else check_segments(segments, n)
        if seg is not None and self.use_comm:
            for p in self._segment_pieces(seg, n, dev):
                piece(entry + "_seg", *p)
        else:                                                         # the plain call: the piece (0, chunk) without a table, and so on
            chunk = n if self.use_comm else self.chunk                # (CommNet: the call goes to the library whole)
            self._grow_work(dev, getattr(self._lib, self._abi[1]), min(n, chunk), int(self.use_comm))
            for beg in range(0, n, max(chunk, 1)):
                piece(entry, beg, min(chunk, n - beg))
        return out if len(out) > 1 else actions

    def _segment_pieces(self, seg, n, dev):
        """the segmented entry's calls over the validated table `seg`: (first row, rows, begin, count, n_seg), one per MAX_SEGMENTS
        segments, each over the rows from its first segment's begin (the first call: row 0) to the next call's (the last: n); the
        workspace is grown to the largest"""
        pieces = []
        for k in (range(0, len(seg), MAX_SEGMENTS) or [0]):
            part = seg[k:k + MAX_SEGMENTS]
            r0 = 0 if k == 0 else int(part[0, 0])
            r1 = n if k + MAX_SEGMENTS >= len(seg) else int(seg[k + MAX_SEGMENTS, 0])
            if r1 > r0:
                begin = (ctypes.c_int32 * max(len(part), 1))(*(part[:, 0] - r0).tolist())
                count = (ctypes.c_int32 * max(len(part), 1))(*part[:, 1].tolist())
                pieces.append((r0, r1 - r0, begin, count, len(part)))
                self._grow_work(dev, getattr(self._lib, self._abi[1] + "_seg"), r1 - r0, 1, len(part))
        return pieces


class HipA2cPolicyF32(_A2cPolicy):
    """one acting step of an _ActorCritic in float32 -- the two input layers (k_a2c_trunk_f32), dense 512 and the two CommNet steps
    (k_a2c_layer_f32, the column sums by k_a2c_colsum_part + k_a2c_colsum), the policy and value heads, the softmax and the draw
    (k_a2c_head_f32): magent_amd/csrc/policy_a2c_f32.hip.  The draw, the chunking and the CommNet rule: _A2cPolicy."""
    _abi, _struct = ("policy_a2c_f32_supported", "policy_a2c_f32_workspace_bytes", "f32"), _A2cWeights

    @torch.no_grad()
    def pack(self):
        self._pack_dense(fragment_order_f32, 8)

    @torch.no_grad()
    def infer(self, view, feature, u=None, want_policy=False, want_value=False, segments=None):
        """view float32 [n][H][W][C], feature float32 [n][F] (contiguous, on the policy's device); u float32 [n] uniform in [0, 1), or None:
        torch.rand from torch's generator; segments: None, or the (begin, count) table of a packed buffer (_A2cPolicy).  Enqueues the step
        on torch's current stream; returns int32 actions [n], followed by the probabilities [n][A] and / or the values [n] if asked for"""
        assert view.dtype == torch.float32 and tuple(view.shape[1:]) == (self.shape.view_h, self.shape.view_w, self.shape.view_c)
        return self._step("policy_a2c_infer_f32", view, feature, u, want_policy, want_value, segments)


class HipA2cPolicy(_A2cPolicy):
    """one acting step of an _ActorCritic with bf16 matrix operands -- the two input layers (k_a2c_trunk_bf16, from float32 views or from
    the engine's bf16 cells), dense 512 and the two CommNet steps (k_a2c_layer_bf16, the column sums by k_a2c_colsum_part +
    k_a2c_colsum), the heads, the softmax and the draw (k_a2c_head_bf16): magent_amd/csrc/policy_a2c_bf16.hip.  Accumulation, biases,
    relu / tanh, the column sums, the softmax and the draw are float32; the rounding points are listed in include/magent_policy.h.

    The draw, the chunking and the CommNet rule: _A2cPolicy.  `cells`: whether the shape has a cell entry (view_c <= 7 and 8 H W <= 4096)."""
    _abi, _struct = ("policy_a2c_supported", "policy_a2c_workspace_bytes", "bf16"), _A2cWeightsBf16

    def _pack_cells(self, t, wv):
        """dense_view in the cells' order: k = 8 cell + channel, zeros for the channels a cell pads with (and for its constant 1.0)"""
        s = self.shape
        if self.cells:
            hw = s.view_h * s.view_w
            wc = wv.new_zeros(256, hw, 8)
            wc[:, :, :s.view_c] = wv.reshape(256, hw, s.view_c)
            t["dense_view_cells"] = fragment_order(_pad_k(wc.reshape(256, 8 * hw), (hw + 1) // 2 * 16))

    @torch.no_grad()
    def pack(self):
        self._pack_dense(fragment_order, 16, self._pack_cells)

    @torch.no_grad()
    def infer(self, view, feature, u=None, want_policy=False, want_value=False, segments=None):
        """view float32 [n][H][W][C] -- or bfloat16 [n][H][W][8], the engine's cells (GridWorld.get_observation_device_bf16), where the
        shape has them --, feature float32 [n][F] (contiguous, on the policy's device); u float32 [n] uniform in [0, 1), or None:
        torch.rand from torch's generator; segments: None, or the (begin, count) table of a packed buffer (_A2cPolicy).  Enqueues the step
        on torch's current stream; returns int32 actions [n], followed by the probabilities [n][A] and / or the values [n] if asked for"""
        cells16, s = view.dtype == torch.bfloat16, self.shape
        if cells16:
            if not self.cells:
                raise ValueError("this view shape has no bf16 cell entry")
            assert tuple(view.shape[1:]) == (s.view_h, s.view_w, 8)
        else:
            assert view.dtype == torch.float32 and tuple(view.shape[1:]) == (s.view_h, s.view_w, s.view_c)
        return self._step("policy_a2c_infer_bf16" if cells16 else "policy_a2c_infer", view, feature, u, want_policy, want_value, segments)
