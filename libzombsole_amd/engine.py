"""Runtime binding of the HIP engine (libzombsole_mi355x.so) through its C ABI.

`Engine` owns one `zs_handle` (N envs on one GPU) plus the torch device
tensors the engine writes its outputs into.  There is no CPU fallback: if
the shared library or a HIP device is missing, construction raises.
"""
import ctypes as C
import os

import numpy as np

from . import _abi

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_build", "libzombsole_mi355x.so")
SYMBOLS = list(_abi.ABI)

_lib = None


class EngineUnavailable(RuntimeError):
    pass


def load_library(path=None):
    """Load the engine .so (no device call is made).  The product library unless `path` names
    another build of the same sources; use_library(path) makes such a build the process's engine
    (diagnostic tools: tools/stamps.py, A/B runs).  No environment variable selects the library."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise EngineUnavailable("HIP engine library not built: %s (run __graft_entry__.build())" % p)
    # torch ships its own libamdhip64.so.7 / libhsa-runtime64.so.1; load it first so the engine
    # binds to that same runtime (same SONAME) instead of pulling a second HIP runtime from
    # /opt/rocm into the process, which cannot open the device once torch's runtime owns it.
    import torch  # noqa: F401
    L = C.CDLL(p)
    for name, argtypes in _abi.ABI.items():
        f = getattr(L, name)
        f.argtypes = argtypes
        f.restype = C.c_char_p if name == "zs_last_error" else C.c_int
    if path is None:
        _lib = L
    return L


def use_library(path):
    """Tools only: make the build at `path` (e.g. a -DZS_STAMPS diagnostic build) the library every
    later Engine of this process binds."""
    global _lib
    _lib = load_library(path)
    return _lib


class EngineError(RuntimeError):
    pass


def _raise(L, rc, what):
    msg = (L.zs_last_error() or b"").decode(errors="replace")
    if rc == _abi.ZS_EINVAL:
        raise ValueError("%s: %s" % (what, msg))
    if rc == _abi.ZS_ENOSPACE:
        raise Exception(msg or "Not enough space to spawn")  # core.py:62-64 raises a bare Exception
    raise EngineError("%s failed (%d): %s" % (what, rc, msg))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _np_ptr(a):
    """A host buffer argument: None, bytes (e.g. struct-packed) or a numpy array."""
    if a is None or isinstance(a, bytes):
        return a
    return C.c_void_p(a.ctypes.data)


def _to_int32(torch, x, device):
    """An integer tensor as a contiguous int32 tensor on `device`; a value int32 does not hold becomes -1 (no env, no
    record, no count and no limit is -1: the device refuses or skips the entry) instead of wrapping into range.  No
    synchronisation."""
    x = x.to(device)
    if x.dtype != torch.int32:
        x = x.to(torch.int64)
        x = torch.where((x < -2 ** 31) | (x > 2 ** 31 - 1), torch.full_like(x, -1), x)
    return x.to(torch.int32).contiguous()


def as_index(torch, x, device, what):
    """`x` (a sequence or tensor of env / record numbers) as a contiguous int32 1-D tensor on `device`, by _to_int32's
    rule; ValueError for bool, float or other than 1-D input.  None (the call's default order) stays None."""
    if x is None:
        return None
    if not torch.is_tensor(x):
        x = torch.as_tensor(x)
        if x.numel() == 0:  # an empty sequence has no integer dtype of its own
            x = x.to(torch.int32)
    if x.dim() != 1 or x.dtype == torch.bool or x.is_floating_point() or x.is_complex():
        raise ValueError("%s: an index is a 1-D integer tensor or sequence" % what)
    return _to_int32(torch, x, device)


def check_tensor(t, what, dtype, device, rows, trailing, at_least=False, align=0):
    """ValueError unless `t` is a contiguous `dtype` tensor [rows, *trailing] on `device` (at_least: `rows` or more
    leading rows) at an address that is a multiple of `align` (0: any).  `what` names the call and the tensor."""
    shape = tuple(t.shape)
    if (t.dtype != dtype or t.device != device or not t.is_contiguous() or shape[1:] != tuple(trailing) or not shape or
            (shape[0] < rows if at_least else shape[0] != rows) or (align and t.data_ptr() % align)):
        raise ValueError("%s must be a contiguous%s %s tensor [%s%d%s] on %s"
                         % (what, ", %d-byte aligned" % align if align else "", dtype, "rows >= " if at_least else "",
                            rows, "".join(", %d" % w for w in trailing), device))


def decode_action_log(words, n, E):
    """(actions, raised) from zs_action_log's words and count (n < 0: a debug raise, -1 - n entries)."""
    raised = n < 0
    k = min(-1 - n if raised else n, E)
    w = words[:2 * k].tolist()
    return [(w[2 * j] & 0xff, (w[2 * j] >> 8) & 0xff, w[2 * j + 1]) for j in range(k)], raised


def decode_death_log(words, n, E):
    """[(slot, serial, x, y, life)] from zs_death_log's words and count."""
    k = max(0, min(n, E))
    w = words[:5 * k].tolist()
    return [tuple(w[5 * j:5 * j + 5]) for j in range(k)]


class Engine(object):
    """N lock-step envs on one MI355X."""

    def __init__(self, builder, device=None, grid_obs=True):
        """grid_obs=False: no grid observation is allocated or written (self.obs is None; every step, graphed step
        and reset passes a null obs_dev): the engine of a learner on entity observations (bind_entity_obs)."""
        import torch
        if not torch.cuda.is_available():
            raise EngineUnavailable("no HIP device visible: the zombsole engine runs only on the GPU")
        self.torch = torch
        self.L = load_library()
        self.builder = builder
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        # Initialise torch's HIP runtime on this device first: the engine .so binds to the same
        # libamdhip64 torch loaded (one runtime per process), and a bare is_available() leaves
        # that runtime without a device context (hipSetDevice then reports no device).
        torch.zeros(1, device=self.device)
        self.h = C.c_void_p()
        self._layouts = {}  # _layout's cache: (call, arguments) -> dict
        rc = self.L.zs_create(C.cast(builder.ptr(), C.c_void_p), self.device.index, C.byref(self.h))
        if rc:
            _raise(self.L, rc, "zs_create")
        shp = (C.c_int32 * 4)()
        self._call("zs_obs_shape", shp)
        self.obs_shape = tuple(int(v) for v in shp)
        self.N = builder.cfg.num_envs
        self.A = builder.num_agents
        c = builder.cfg
        self.E = self.A + builder.num_bots + max(c.initial_zombies, c.minimum_zombies)  # entity slots (zs_create)
        self.multi = builder.cfg.reward_mode == _abi.REWARD_MULTI
        dt = {_abi.DTYPE_I32: torch.int32, _abi.DTYPE_I64: torch.int64, _abi.DTYPE_I16: torch.int16}
        self.obs_dtype = dt[builder.cfg.obs_dtype]
        kw = dict(device=self.device)
        self.grid_obs = bool(grid_obs)
        self.out = self.outputs()
        self.obs, self.rewards, self.done, self.trunc = self.out.obs, self.out.rewards, self.out.done, self.out.trunc
        self.listed, self.was_reset = self.out.listed, self.out.was_reset
        self.actions = torch.zeros((self.N, self.A, 3), dtype=torch.int32, **kw)
        n = C.c_int32()
        self._call("zs_state_size", C.byref(n))
        self.state_words = int(n.value)
        self.n_discrete = 7 if self.multi else 6
        self.masks = None  # the bound action-mask tensor (bind_action_masks), uint8 [N, A, 8]
        self.entities = None  # the bound entity-observation tensor (bind_entity_obs), int16 [N, A, ROW]
        self.entity_k = None  # its (kz, kp)
        self.entity_act_ids = None  # the bound entity-action ids (bind_entity_act), int32 [N, A]
        self.entity_act_masks = None  # the bound entity-action masks, uint8 [N, A, row_bytes]
        self.entity_act_k = None  # their (kz, kp)
        self.nav = None  # the bound path-distance rows (nav_bind), int16 [N, A, F, 8]
        self.nav_args = None  # its (fields mask, max_dist)
        self.pilot = None  # the bound scripted triples (bind_autopilot), int32 [N, A, 3]; self.actions when bound into it
        self.pilot_policy = None  # the bound policy codes, uint8 [N, A]

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.zs_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name, *args):
        """The C ABI's `name` on this handle; a nonzero status is raised (_raise) under the call's name."""
        rc = getattr(self.L, name)(self.h, *args)
        if rc:
            _raise(self.L, rc, name)

    def _layout(self, name, *args):
        """The layout call `name` as a dict of its _abi.LAYOUT_KEYS (reserved words left out), read once per
        argument set."""
        if (name,) + args not in self._layouts:
            keys = _abi.LAYOUT_KEYS[name]
            out = (C.c_int32 * len(keys))()
            self._call(name, *args + (out,))
            self._layouts[(name,) + args] = {k: int(v) for k, v in zip(keys, out) if k is not None}
        return self._layouts[(name,) + args]

    def seed(self, seeds, env0=0):
        arr = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        self._call("zs_seed", env0, len(arr), arr.ctypes.data_as(C.POINTER(C.c_uint64)), self._stream())

    def reset(self, mask=None):
        """Reset envs (all, or where the uint8 device tensor `mask` is nonzero)."""
        self._call("zs_reset", _ptr(mask), _ptr(self.obs), self._stream())
        return self.obs

    def outputs(self, rows=None, obs=None, flat=None):
        """A set of step output buffers (StepOutputs) with `rows` >= N rows; the engine writes the
        first N.  Steps may alternate between sets (double-buffered outputs, vector.StepGather).  obs / flat,
        when given, are the storage to use (e.g. this rank's slice of a gather buffer)."""
        return StepOutputs(self, self.N if rows is None else max(int(rows), self.N), obs, flat)

    def step(self, actions=None, out=None):
        """One tick for all envs; `actions` int32 [N, A, 3] device tensor (default: self.actions);
        outputs into `out` (default: self.out)."""
        a = self.actions if actions is None else actions
        o = self.out if out is None else out
        self._call("zs_step", _ptr(a), _ptr(o.obs), _ptr(o.rewards), _ptr(o.done), _ptr(o.trunc), _ptr(o.listed),
                   _ptr(o.was_reset), self._stream())
        return self._obs_rows(o), o.rewards[:self.N], o.done[:self.N], o.trunc[:self.N]

    def _obs_rows(self, o):
        return None if o.obs is None else o.obs[:self.N]

    def step_graph(self, step0, n_discrete, out=None, steps=1, actions=None):
        """gen_actions(t, n_discrete) + step() as one replayed hipGraph (t = step0 on the call that captures the
        buffer set, then advancing by one per policy step on the device: a cached set ignores step0, and step(),
        step_graphed() and other n_discrete = 0 graphs do not move the counter).  steps > 1: that many steps per graph launch
        (zs_step_graph_n), the outputs holding the last one's.  n_discrete = 0: no policy, the graph
        replays step(actions) on the caller's action tensor (default self.actions), which the caller
        fills on the current stream before each call (see step_graphed)."""
        o = self.out if out is None else out
        a = self.actions if actions is None else actions
        bufs = (_ptr(a), _ptr(o.obs), _ptr(o.rewards), _ptr(o.done), _ptr(o.trunc), _ptr(o.listed), _ptr(o.was_reset),
                self._stream())
        if steps == 1:
            self._call("zs_step_graph", int(step0), int(n_discrete), *bufs)
        else:
            self._call("zs_step_graph_n", int(step0), int(n_discrete), int(steps), *bufs)
        return self._obs_rows(o), o.rewards[:self.N], o.done[:self.N], o.trunc[:self.N]

    def step_graphed(self, actions=None, out=None):
        """step(actions) as one replayed hipGraph launch (zs_step_graph with n_discrete = 0): the
        learner's per-step call (gym/multiagent_env.py:111-171) without the 3-5 host dispatches of an
        eager zs_step.  The graph is keyed on the action and output buffers, so a caller keeps them
        fixed (self.actions, an output set) and rewrites their contents each step."""
        return self.step_graph(0, 0, out=out, actions=actions)

    def observe(self, mask=None, out=None):
        """Re-encode observations from the current state (after pokes, or a viewer's after
        unpack_obs_state) into `out` (default: self.obs), a tensor of the observations' dtype with at least
        N rows of obs_shape."""
        o = self.obs if out is None else out
        if o is None:
            raise ValueError("observe: this engine keeps no grid observations (grid_obs=False); pass out=")
        if out is not None:
            check_tensor(o, "observe: out", self.obs_dtype, self.device, self.N, self.obs_shape, at_least=True)
        self._call("zs_observe", _ptr(mask), _ptr(o), self._stream())
        return o

    # -- action masks of the discrete tables (zs_action_mask*) ------------------------------------------------------
    def action_mask(self, mask=None, out=None):
        """The action masks of the current state, uint8 [N, A, 8] (zs_action_mask): entry k of agent a is 1 when
        the reference would carry out discrete action k for it; entries at k >= n_discrete are 0, absent agents
        all 0.  Envs where the uint8 device tensor `mask` is zero keep their bytes.  Into `out` when given, else
        into the bound tensor, else into a tensor this call allocates (zeroed)."""
        o = out if out is not None else self.masks
        if o is None:
            o = self.torch.zeros((self.N, self.A, 8), dtype=self.torch.uint8, device=self.device)
        check_tensor(o, "action_mask: masks", self.torch.uint8, self.device, self.N, (self.A, 8), align=8)
        self._call("zs_action_mask", _ptr(mask), _ptr(o), self._stream())
        return o

    def bind_action_masks(self, buf=True):
        """Bind `buf` (True: a new tensor; None / False: unbind) so that every step(), step_graph() and
        step_graphed() ends with a mask launch into it (zs_action_mask_bind); self.masks is the bound tensor."""
        if buf is True:
            buf = self.torch.zeros((self.N, self.A, 8), dtype=self.torch.uint8, device=self.device)
        elif buf is False:
            buf = None
        if buf is not None:
            check_tensor(buf, "bind_action_masks: masks", self.torch.uint8, self.device, self.N, (self.A, 8), align=8)
        self._call("zs_action_mask_bind", _ptr(buf))
        self.masks = buf
        return buf

    # -- entity observations (zs_entity_obs*): per agent its own values, the K nearest zombies and players, the nearest
    # objective and four rays, int16 [N, A, ROW] ------------------------------------------------------------------
    def entity_layout(self, kz=None, kp=None):
        """zs_entity_obs_layout as a dict: "row_words", the word offsets "self", "zombies", "players", "objective",
        "rays", "ray_cap" and "row_bytes", with "kz" and "kp" (default: the bound tensor's)."""
        kz, kp = self._entity_k(kz, kp)
        return dict(self._layout("zs_entity_obs_layout", kz, kp), kz=kz, kp=kp)

    def _entity_k(self, kz, kp):
        if kz is None and kp is None and self.entity_k is not None:
            return self.entity_k
        if kz is None or kp is None:
            raise ValueError("entity observations: kz and kp are needed (no tensor is bound)")
        return int(kz), int(kp)

    def _check_entities(self, t, kz, kp, what):
        row = _abi.entity_layout(kz, kp)["row_words"]  # ValueError on bad K values
        check_tensor(t, what + ": entity observations", self.torch.int16, self.device, self.N, (self.A, row), align=8)

    def entity_obs(self, mask=None, out=None, kz=None, kp=None):
        """The entity observations of the current state, int16 [N, A, 16 + 4 (kz + kp)] (zs_entity_obs; the layout:
        entity_layout, libzombsole_amd/entity_obs.py).  Envs where the uint8 device tensor `mask` is zero keep their
        bytes.  Into `out` when given, else into the bound tensor (with its kz, kp), else into a tensor this call
        allocates (zeroed)."""
        kz, kp = self._entity_k(kz, kp)
        o = out
        if o is None and self.entities is not None and (kz, kp) == self.entity_k:
            o = self.entities
        if o is None:
            o = self.torch.zeros((self.N, self.A, _abi.entity_layout(kz, kp)["row_words"]), dtype=self.torch.int16,
                                 device=self.device)
        self._check_entities(o, kz, kp, "entity_obs")
        self._call("zs_entity_obs", _ptr(mask), kz, kp, _ptr(o), self._stream())
        return o

    def bind_entity_obs(self, buf=True, kz=4, kp=1):
        """Bind `buf` (True: a new tensor; None / False: unbind) so that every step(), step_graph() and
        step_graphed() ends with an entity-observation launch into it (zs_entity_obs_bind); self.entities is the
        bound tensor and self.entity_k its (kz, kp)."""
        if buf is True:
            buf = self.torch.zeros((self.N, self.A, _abi.entity_layout(kz, kp)["row_words"]), dtype=self.torch.int16,
                                   device=self.device)
        elif buf is False:
            buf = None
        if buf is not None:
            self._check_entities(buf, kz, kp, "bind_entity_obs")
        self._call("zs_entity_obs_bind", _ptr(buf), int(kz) if buf is not None else 0, int(kp) if buf is not None else 0)
        self.entities = buf
        self.entity_k = (int(kz), int(kp)) if buf is not None else None
        return buf

    # -- entity-targeted actions (zs_entity_act*): a table of 15 + kz + kp ids per agent over the entity observation's
    # rows (libzombsole_amd/entity_act.py): ids int32 [N, A], masks uint8 [N, A, row_bytes], triples int32 [N, A, 3] ---
    def _entity_act_k(self, kz, kp):
        if kz is None and kp is None and self.entity_act_k is not None:
            return self.entity_act_k
        return self._entity_k(kz, kp)

    def entity_act_layout(self, kz=None, kp=None):
        """zs_entity_act_table as a dict: "nid", "row_bytes" (nid rounded up to 8) and the first id of the blocks
        "attack_dir", "heal_dir", "zombie_rows", "player_rows", "end", with "kz" and "kp" (default: the bound ones, else
        the bound entity observation's)."""
        kz, kp = self._entity_act_k(kz, kp)
        if ("zs_entity_act_table", kz, kp) not in self._layouts:
            out = (C.c_int32 * len(_abi.ENTITY_ACT_TABLE_KEYS))()
            self._call("zs_entity_act_table", kz, kp, out)
            self._layouts[("zs_entity_act_table", kz, kp)] = {k: int(v) for k, v in zip(_abi.ENTITY_ACT_TABLE_KEYS, out) if k}
        return dict(self._layouts[("zs_entity_act_table", kz, kp)], kz=kz, kp=kp)

    def entity_act_decode(self, ids, mask=None, out=None, kz=None, kp=None):
        """The triples of `ids` (int32 [N, A] on the device) on the current state, int32 [N, A, 3] (zs_entity_act_decode).
        Envs where the uint8 device tensor `mask` is zero keep their rows.  Into `out` when given, else a new tensor."""
        t = self.torch
        kz, kp = self._entity_act_k(kz, kp)
        self.entity_act_layout(kz, kp)  # ValueError on bad K values
        check_tensor(ids, "entity_act_decode: ids", t.int32, self.device, self.N, (self.A,))
        o = out if out is not None else t.zeros((self.N, self.A, 3), dtype=t.int32, device=self.device)
        check_tensor(o, "entity_act_decode: out", t.int32, self.device, self.N, (self.A, 3))
        self._call("zs_entity_act_decode", _ptr(mask), kz, kp, _ptr(ids), _ptr(o), self._stream())
        return o

    def entity_act_mask(self, mask=None, out=None, kz=None, kp=None):
        """The table's masks of the current state, uint8 [N, A, row_bytes] (zs_entity_act_mask); bytes past nid are 0.
        Envs where the uint8 device tensor `mask` is zero keep their bytes.  Into `out` when given, else into the bound
        tensor (same kz, kp), else into a tensor this call allocates (zeroed)."""
        t = self.torch
        kz, kp = self._entity_act_k(kz, kp)
        rb = self.entity_act_layout(kz, kp)["row_bytes"]
        o = out
        if o is None and self.entity_act_masks is not None and (kz, kp) == self.entity_act_k:
            o = self.entity_act_masks
        if o is None:
            o = t.zeros((self.N, self.A, rb), dtype=t.uint8, device=self.device)
        check_tensor(o, "entity_act_mask: masks", t.uint8, self.device, self.N, (self.A, rb), align=8)
        self._call("zs_entity_act_mask", _ptr(mask), kz, kp, _ptr(o), self._stream())
        return o

    def entity_act_encode(self, triples, mask=None, out=None, kz=None, kp=None):
        """The smallest id whose decoded triple equals each row of `triples` (int32 [N, A, 3]) on the current state, else
        -1; int32 [N, A] (zs_entity_act_encode).  Envs where `mask` is zero keep their values."""
        t = self.torch
        kz, kp = self._entity_act_k(kz, kp)
        self.entity_act_layout(kz, kp)
        check_tensor(triples, "entity_act_encode: triples", t.int32, self.device, self.N, (self.A, 3))
        o = out if out is not None else t.full((self.N, self.A), -1, dtype=t.int32, device=self.device)
        check_tensor(o, "entity_act_encode: out", t.int32, self.device, self.N, (self.A,))
        self._call("zs_entity_act_encode", _ptr(mask), kz, kp, _ptr(triples), _ptr(o), self._stream())
        return o

    def bind_entity_act(self, ids=None, masks=None, kz=4, kp=1):
        """Bind `ids` (True: a new int32 [N, A] tensor) so that every step(), step_graph() and step_graphed() begins
        with their decode into the step's actions, and `masks` (True: a new uint8 [N, A, row_bytes] tensor) so that every
        step launches the table's masks into it (zs_entity_act_bind).  None / False for both unbinds.  self.entity_act_ids,
        self.entity_act_masks and self.entity_act_k hold the binding.  Returns (ids, masks)."""
        t = self.torch
        ids = None if ids is False else ids
        masks = None if masks is False else masks
        if ids is None and masks is None:
            self._call("zs_entity_act_bind", None, None, 0, 0)
            self.entity_act_ids = self.entity_act_masks = self.entity_act_k = None
            return None, None
        kz, kp = int(kz), int(kp)
        rb = self.entity_act_layout(kz, kp)["row_bytes"]
        if ids is True:
            ids = t.zeros((self.N, self.A), dtype=t.int32, device=self.device)
        if masks is True:
            masks = t.zeros((self.N, self.A, rb), dtype=t.uint8, device=self.device)
        if ids is not None:
            check_tensor(ids, "bind_entity_act: ids", t.int32, self.device, self.N, (self.A,))
        if masks is not None:
            check_tensor(masks, "bind_entity_act: masks", t.uint8, self.device, self.N, (self.A, rb), align=8)
        self._call("zs_entity_act_bind", _ptr(ids), _ptr(masks), kz, kp)
        self.entity_act_ids, self.entity_act_masks, self.entity_act_k = ids, masks, (kz, kp)
        return ids, masks

    # -- path-distance fields (zs_nav*): walking distance to the objectives and to the zombies, int16 [N, A, F, 8] rows
    # and uint16 [n, H, W] frames (libzombsole_amd/nav.py) ---------------------------------------------------------
    def _nav_args(self, fields, max_dist):
        from . import nav
        if fields is None and max_dist is None and self.nav_args is not None:
            return self.nav_args
        if fields is None:
            raise ValueError("path distances: fields are needed (no tensor is bound)")
        return nav.fields_mask(fields), nav._check_max_dist(_abi.NAV_MAX_DIST if max_dist is None else max_dist)

    def nav_layout(self, fields=None):
        """zs_nav_plan as a dict of _abi.NAV_PLAN_KEYS: "F", "row_words" (8), the word offsets "field0" and "field1" of
        the fields' rows in an agent's block (-1: not emitted), and the launch plan "envs_per_wg", "block", "lds_bytes"
        (0 where the map is past the plan's limit) with "env_bytes", one env's search image; with "fields"."""
        fields = self._nav_args(fields, None)[0] if fields is not None or self.nav_args else _abi.NAV_OBJECTIVE | _abi.NAV_ZOMBIES
        if ("zs_nav_plan", fields) not in self._layouts:
            out = (C.c_int32 * len(_abi.NAV_PLAN_KEYS))()
            self._call("zs_nav_plan", fields, out)
            self._layouts[("zs_nav_plan", fields)] = dict(zip(_abi.NAV_PLAN_KEYS, (int(v) for v in out)), fields=fields)
        return dict(self._layouts[("zs_nav_plan", fields)])

    def _check_nav(self, t, fields, what):
        F = bin(fields).count("1")
        check_tensor(t, what + ": path distances", self.torch.int16, self.device, self.N, (self.A, F, _abi.NAV_ROW_WORDS), align=8)

    def nav_obs(self, mask=None, out=None, fields=None, max_dist=None):
        """The path-distance rows of the current state, int16 [N, A, F, 8] (zs_nav_obs; the row: libzombsole_amd/nav.py).
        `fields`: a bitmask, a name or names ("objective", "zombies"); default: the bound tensor's, with its max_dist.
        Envs where the uint8 device tensor `mask` is zero keep their bytes.  Into `out` when given, else into the bound
        tensor (same fields and cap), else into a tensor this call allocates (zeroed)."""
        fields, max_dist = self._nav_args(fields, max_dist)
        o = out
        if o is None and self.nav is not None and (fields, max_dist) == self.nav_args:
            o = self.nav
        if o is None:
            o = self.torch.zeros((self.N, self.A, bin(fields).count("1"), _abi.NAV_ROW_WORDS), dtype=self.torch.int16,
                                 device=self.device)
        self._check_nav(o, fields, "nav_obs")
        self._call("zs_nav_obs", _ptr(mask), fields, max_dist, _ptr(o), self._stream())
        return o

    def nav_field(self, which, envs=None, out=None, max_dist=None):
        """The full field `which` ("objective", "zombies" or its bit) of `envs` (an integer tensor or sequence, repeats
        allowed; default every env in order) as uint16 [n, H, W] on the device, 0xFFFF = unreachable or blocked
        (zs_nav_field: one launch, no synchronisation).  An index outside [0, N) leaves its frame as it is (0xFFFF in a
        tensor this call allocates)."""
        from . import nav
        t = self.torch
        which = nav.fields_mask(which)
        max_dist = nav._check_max_dist(_abi.NAV_MAX_DIST if max_dist is None else max_dist)
        envs = as_index(t, envs, self.device, "nav_field: envs")
        n = self.N if envs is None else int(envs.numel())
        W, H = self.builder.map.size
        if out is None:
            out = t.full((n, H, W), -1, dtype=t.int16, device=self.device).view(t.uint16)  # 0xFFFF
        check_tensor(out, "nav_field: out", t.uint16, self.device, n, (H, W), at_least=True)
        if n == 0:
            return out
        self._call("zs_nav_field", _ptr(envs), n, which, max_dist, _ptr(out), self._stream())
        return out

    def nav_bind(self, buf=True, fields=("objective", "zombies"), max_dist=None):
        """Bind `buf` (True: a new tensor; None / False: unbind) so that every step(), step_graph() and step_graphed()
        ends with a path-distance launch into it (zs_nav_bind); self.nav is the bound tensor and self.nav_args its
        (fields mask, max_dist)."""
        t = self.torch
        if buf is False:
            buf = None
        if buf is None:
            self._call("zs_nav_bind", None, 0, 0)
            self.nav = self.nav_args = None
            return None
        fields, max_dist = self._nav_args(fields, max_dist)
        if buf is True:
            buf = t.zeros((self.N, self.A, bin(fields).count("1"), _abi.NAV_ROW_WORDS), dtype=t.int16, device=self.device)
        self._check_nav(buf, fields, "nav_bind")
        self._call("zs_nav_bind", _ptr(buf), fields, max_dist)
        self.nav, self.nav_args = buf, (fields, max_dist)
        return buf

    # -- scripted policies for agent slots (zs_autopilot*): the bots' decisions as agent triples, int32 [N, A, 3] -------
    def policy_tensor(self, policy):
        """`policy` as the uint8 [N, A] device tensor of codes (libzombsole_amd/autopilot.py): a policy's name or code
        for every agent, or a tensor / array of codes that broadcasts to [N, A].  A uint8 [N, A] tensor on the device
        comes back as it is."""
        from . import autopilot
        t = self.torch
        if isinstance(policy, (str, int)):
            return t.full((self.N, self.A), autopilot.policy_code(policy), dtype=t.uint8, device=self.device)
        p = t.as_tensor(policy)
        if p.dtype == t.uint8 and p.device == self.device and tuple(p.shape) == (self.N, self.A) and p.is_contiguous():
            return p
        if p.dtype == t.bool or p.is_floating_point() or p.is_complex():
            raise ValueError("autopilot: policy codes are integers")
        return p.to(self.device).to(t.uint8).expand(self.N, self.A).contiguous()

    def autopilot(self, policy, mask=None, out=None):
        """The scripted triples of the current state under `policy` (policy_tensor's forms), int32 [N, A, 3]
        (zs_autopilot).  Rows of code 0 and envs where the uint8 device tensor `mask` is zero keep their values.  Into
        `out` when given, else into a tensor this call allocates (zeroed)."""
        t = self.torch
        pol = self.policy_tensor(policy)
        o = out if out is not None else t.zeros((self.N, self.A, 3), dtype=t.int32, device=self.device)
        check_tensor(o, "autopilot: out", t.int32, self.device, self.N, (self.A, 3))
        self._call("zs_autopilot", _ptr(mask), _ptr(pol), _ptr(o), self._stream())
        return o

    def bind_autopilot(self, policy, into_actions=False, out=None):
        """Bind `policy` (policy_tensor's forms; None / False: unbind) so that every step(), step_graph() and
        step_graphed() ends with an autopilot launch (zs_autopilot_bind) into self.pilot: a new tensor, `out`, or with
        into_actions=True self.actions, the closed loop in which a step's last launch writes the rows the next step
        reads.  self.pilot_policy is the bound uint8 [N, A] code tensor; writing into it changes the policy of the
        following steps, graph replays included.  Returns self.pilot."""
        t = self.torch
        if policy is None or policy is False:
            self._call("zs_autopilot_bind", None, None)
            self.pilot = self.pilot_policy = None
            return None
        pol = self.policy_tensor(policy)
        if into_actions:
            out = self.actions
        elif out is None:
            out = t.zeros((self.N, self.A, 3), dtype=t.int32, device=self.device)
        check_tensor(out, "bind_autopilot: out", t.int32, self.device, self.N, (self.A, 3))
        self._call("zs_autopilot_bind", _ptr(pol), _ptr(out))
        self.pilot, self.pilot_policy = out, pol
        return out

    # -- observation-state records (zs_obs_state_*): what the encoders read of an env, a fraction of its observation
    def obs_state_layout(self):
        """zs_obs_state_layout as a dict: the byte offset of every section of an env's record (the names of
        _abi.OBS_STATE_SECTIONS), "pad", "rec_bytes" and "hp_bytes"."""
        return self._layout("zs_obs_state_layout")

    def _check_records(self, rec, what, rows, layout):
        """`rec` holds at least `rows` records of `layout` (obs_state_layout() or snapshot_layout())."""
        check_tensor(rec, what + ": records", self.torch.uint8, self.device, rows, (layout["rec_bytes"],), at_least=True,
                     align=16)

    def pack_obs_state(self, out=None):
        """Every env's observation-state record into `out`, uint8 [rows >= N, rec_bytes] (default: a new
        tensor of N rows); the first N rows are written, every byte of them."""
        if out is None:
            out = self.torch.empty((self.N, self.obs_state_layout()["rec_bytes"]), dtype=self.torch.uint8,
                                   device=self.device)
        self._check_records(out, "pack_obs_state", self.N, self.obs_state_layout())
        self._call("zs_obs_state_pack", _ptr(out), self._stream())
        return out

    def unpack_obs_state(self, rec, env0=0, n=None):
        """Viewer engines only: records rec[:n] (default: all rows) into envs [env0, env0 + n); observe() then
        encodes them.  The records come from engines of the same map, entity counts and observation form."""
        n = rec.shape[0] if n is None else int(n)
        self._check_records(rec, "unpack_obs_state", n, self.obs_state_layout())
        self._call("zs_obs_state_unpack", _ptr(rec), int(rec.shape[1]), int(env0), n, self._stream())

    # -- snapshot records (zs_snapshot / zs_restore): complete envs, for checkpoints, rewinds and forks -------------
    def snapshot_layout(self):
        """zs_snapshot_layout as a dict: the byte offset of every section of an env's snapshot record (the names
        of _abi.SNAPSHOT_SECTIONS), "pad", "rec_bytes" and "fingerprint" (handles whose fingerprints agree can
        exchange records)."""
        L = dict(self._layout("zs_snapshot_layout"))
        lo, hi = L.pop("fingerprint_lo"), L.pop("fingerprint_hi")
        L["fingerprint"] = (lo & 0xffffffff) | ((hi & 0xffffffff) << 32)
        del L["nscal"], L["ring_words"]  # the record format's constants (_abi.SNAPSHOT_NSCAL, SNAPSHOT_RING)
        if not L["env_params"]:  # nonzero in a FLAG_ENV_PARAMS handle's record: the current triple, then the next one
            del L["env_params"]
        return L

    def snapshot(self, envs=None, out=None):
        """The snapshot records of `envs` (default: all N, in order; duplicates allowed) as uint8 [n, rec_bytes]
        (into the first n rows of `out` when given).  Asynchronous on the current stream."""
        idx = as_index(self.torch, envs, self.device, "snapshot")
        n = self.N if idx is None else int(idx.shape[0])
        L = self.snapshot_layout()
        if out is None:
            out = self.torch.empty((n, L["rec_bytes"]), dtype=self.torch.uint8, device=self.device)
        self._check_records(out, "snapshot", n, L)
        self._call("zs_snapshot", _ptr(idx), n, _ptr(out), self._stream())
        return out[:n]

    def restore(self, rec, src=None, dst=None, check=True):
        """Record src[k] of `rec` (default: k) into env dst[k] (default: k), then the pending-reset list rebuilt
        from the restored flags (zs_restore).  Sources may repeat, destinations must be distinct.  check=True
        validates the indices on the host (one small synchronisation; ValueError on a record or env out of range,
        a repeated destination, lengths that differ); check=False is the asynchronous path, on which the kernel
        skips out-of-range entries and distinct destinations are the caller's contract."""
        t = self.torch
        self._check_records(rec, "restore", 0, self.snapshot_layout())
        s, d = as_index(t, src, self.device, "restore"), as_index(t, dst, self.device, "restore")
        n = int(s.shape[0]) if s is not None else int(d.shape[0]) if d is not None else int(rec.shape[0])
        if s is not None and d is not None and s.shape[0] != d.shape[0]:
            raise ValueError("restore: src and dst differ in length")
        if check:
            sv = s if s is not None else t.arange(n, device=self.device)
            dv = d if d is not None else t.arange(n, device=self.device)
            bad = ((sv < 0) | (sv >= rec.shape[0])).any() | ((dv < 0) | (dv >= self.N)).any()
            dup = t.unique(dv).numel() != n if n else False
            if bool(bad):
                raise ValueError("restore: a record outside [0, %d) or an env outside [0, %d)" % (rec.shape[0], self.N))
            if dup:
                raise ValueError("restore: a destination env is repeated")
        self._call("zs_restore", _ptr(rec), int(rec.shape[1]), int(rec.shape[0]), _ptr(s), _ptr(d), n, self._stream())

    # -- per-env zombie counts and time limits (zs_env_params_*; a config with FLAG_ENV_PARAMS) -------------------
    def set_env_params(self, params, envs=None, check=True):
        """The triples (initial_zombies, minimum_zombies, max_episode_steps) that `envs` (an index tensor or
        sequence; default: envs 0..n-1) take up at their next reset (zs_env_params_set); a running episode keeps
        its own.  params: int32 [n, 3], or a dict of three [n] tensors under those names.  The config's counts are
        caps and max_episode_steps >= 0 (0: none); an entry outside them, or naming an env outside [0, N), is not
        applied.  When an env is named more than once, one of its triples wins whole.  check=True calls
        zs_env_params_check afterwards (one synchronisation: it reads OVF_PARAM_RANGE and clears that bit alone) and
        raises ValueError if an entry was refused; check=False never synchronises: the refusal stays in overflow() as OVF_PARAM_RANGE."""
        t = self.torch
        if isinstance(params, dict):
            params = t.stack([t.as_tensor(params[k]).to(self.device).reshape(-1) for k in _abi.ENV_PARAMS], dim=1)
        p = t.as_tensor(params)
        if p.dim() != 2 or p.shape[1] != 3 or p.dtype in (t.bool, t.float16, t.float32, t.float64):
            raise ValueError("set_env_params: params are an integer tensor [n, 3] or a dict of %s" % (_abi.ENV_PARAMS,))
        p = _to_int32(t, p, self.device)
        idx = as_index(t, envs, self.device, "set_env_params: envs")
        if idx is not None and idx.shape[0] != p.shape[0]:
            raise ValueError("set_env_params: %d envs for %d triples" % (idx.shape[0], p.shape[0]))
        self._call("zs_env_params_set", _ptr(idx), int(p.shape[0]), _ptr(p), self._stream())
        if not check:
            return
        refused = C.c_uint32(0)  # reads OVF_PARAM_RANGE and clears that bit alone (one synchronisation)
        self._call("zs_env_params_check", C.byref(refused), self._stream())
        if refused.value:
            raise ValueError("set_env_params: an env outside [0, %d) or a value outside its range (caps: the "
                             "config's counts; max_episode_steps >= 0); the other entries were applied" % self.N)

    def env_params(self, current=False, out=None):
        """int32 [N, 3]: every env's (initial_zombies, minimum_zombies, max_episode_steps), the triple its next
        reset takes up, or with current=True the triple of its running episode (zs_env_params_get)."""
        t = self.torch
        o = t.empty((self.N, 3), dtype=t.int32, device=self.device) if out is None else out
        check_tensor(o, "env_params: out", t.int32, self.device, self.N, (3,))
        self._call("zs_env_params_get", 1 if current else 0, _ptr(o), self._stream())
        return o

    # -- per-env episode statistics (zs_episode_stats_*; a config with FLAG_EPISODE_STATS) -------------------------
    def episode_stats_layout(self):
        """zs_episode_stats_layout as a dict: "R" (reward slots per env), "last_words", "tot_words" (8 each), and the
        byte offset "ep_run" and size "ep_bytes" of the running part's section of the handle's snapshot record."""
        return self._layout("zs_episode_stats_layout")

    def episode_stats(self, mask=None, out=None):
        """The episode statistics as a dict of five device tensors (zs_episode_stats_get, one launch, no
        synchronisation): "run_ret", "last_ret", "sum_ret" float64 [N, R], "last" int32 [N, 8] (_abi.EP_LAST) and "tot"
        (_abi.EP_TOT; uint32 counters in an int32 tensor, read with & 0xffffffff).  Envs where the uint8 device tensor
        `mask` is zero keep their rows: zero in the tensors this call allocates, untouched in `out` (a dict of the
        same five contiguous tensors, any of them None to skip it)."""
        t = self.torch
        R = self.episode_stats_layout()["R"]
        shapes = {"run_ret": (t.float64, R), "last_ret": (t.float64, R), "sum_ret": (t.float64, R), "last": (t.int32, 8),
                  "tot": (t.int32, 8)}
        if out is None:
            out = {k: t.zeros((self.N, w), dtype=dt, device=self.device) for k, (dt, w) in shapes.items()}
        for k, (dt, w) in shapes.items():
            if out.get(k) is not None:
                check_tensor(out[k], "episode_stats: " + k, dt, self.device, self.N, (w,))
        self._call("zs_episode_stats_get", _ptr(mask), *[_ptr(out.get(k)) for k in shapes], self._stream())
        return out

    def clear_episode_stats(self, mask=None):
        """Zero the last finished episode and the totals of every env (or where the uint8 device tensor `mask` is
        nonzero); the running returns stay (zs_episode_stats_clear)."""
        self._call("zs_episode_stats_clear", _ptr(mask), self._stream())

    # -- frames of the envs (zs_render*; a config with FLAG_RENDER) ------------------------------------------------
    def render_layout(self):
        """zs_render_layout as a dict: "height", "width", "frame_bytes", "cell", "mask", "palette", "body_bytes" (the
        body colours' bytes per env) and "body_col" (their offset in the handle's snapshot record)."""
        return self._layout("zs_render_layout")

    def render(self, envs=None, out=None):
        """Frames of the envs as a uint8 [n, 10 H, 10 W, 3] RGB device tensor (zs_render: one launch, no
        synchronisation), pixel-exact to the map area of the reference's OpencvRenderer.  `envs`: an integer
        tensor or sequence of env indices (as_index), repeats allowed, default every env in order; an index outside
        [0, N) leaves its frame as it is (zero in a tensor this call allocates).  `out`: a contiguous uint8 device tensor
        [m, 10 H, 10 W, 3] to draw into; with m < n only the first m entries are drawn.  Without `out` the frames are
        allocated zero-filled on every call (1.2 MB per bridge64 frame: a memset of the whole tensor ahead of the
        draw), so a caller that draws many envs or draws every step passes its own `out`."""
        t = self.torch
        L = self.render_layout()
        envs = as_index(t, envs, self.device, "render: envs")
        n = self.N if envs is None else int(envs.numel())
        if out is None:
            out = t.zeros((n, L["height"], L["width"], 3), dtype=t.uint8, device=self.device)
        check_tensor(out, "render: out", t.uint8, self.device, 0, (L["height"], L["width"], 3), at_least=True)
        self._call("zs_render", _ptr(envs), n, _ptr(out), int(out.shape[0]), self._stream())
        return out

    def set_render_atlas(self, masks, palette):
        """Replace the sprite atlas (zs_render_sprites; waits for the device): `masks` uint32 [5, 4], the 121-bit masks
        of render.SHAPES, `palette` uint8 [8, 3] RGB (render.default_atlas() gives the reference's)."""
        m = np.ascontiguousarray(np.asarray(masks, dtype=np.uint32).reshape(5, 4))
        pal = np.ascontiguousarray(np.asarray(palette, dtype=np.uint8).reshape(8, 3))
        self._call("zs_render_sprites", _np_ptr(m), _np_ptr(pal))

    def gen_actions(self, step, n_discrete, out=None):
        o = self.actions if out is None else out
        self._call("zs_gen_actions", int(step), int(n_discrete), _ptr(o), self._stream())
        return o

    def profile(self, enable=True):
        """Bracket every k_tick / k_obs launch with HIP events on its stream."""
        self._call("zs_profile", 1 if enable else 0)

    def profile_read(self):
        """Per-kernel totals: tick_ms/tick_n, obs_ms/obs_n, reset_ms/reset_n, respawn_ms/respawn_n."""
        out = (C.c_double * 8)()
        self._call("zs_profile_read", out)
        return {"tick_ms": out[0], "tick_n": int(out[1]), "obs_ms": out[2], "obs_n": int(out[3]),
                "reset_ms": out[4], "reset_n": int(out[5]), "respawn_ms": out[6], "respawn_n": int(out[7])}

    def describe(self):
        """The launch configuration the engine chose (zs_describe), as a dict."""
        import json
        buf = C.create_string_buffer(2048)
        self._call("zs_describe", buf, len(buf))
        return json.loads(buf.value.decode())

    def debug_stamps(self, n=5):
        """Per-phase k_tick cycle sums / maxima (diagnostic -DZS_STAMPS build only)."""
        ssum = np.zeros(n, dtype=np.uint64)
        smax = np.zeros(n, dtype=np.uint64)
        self._call("zs_debug_stamps", C.c_void_p(ssum.ctypes.data), C.c_void_p(smax.ctypes.data), n)
        return ssum, smax

    def debug_stamps_wg(self, n_wgs, n_phase):
        """Per-workgroup phase cycles of the step launches since the last stamps read, shape [n_wgs, n_phase]
        (diagnostic -DZS_STAMPS build only)."""
        out = np.zeros((n_wgs, n_phase), dtype=np.uint64)
        self._call("zs_debug_stamps_wg", C.c_void_p(out.ctypes.data), n_wgs, n_phase)
        return out

    def debug_timeline(self, n):
        """Start / end s_memrealtime (100 MHz) of the first n workgroups of the last fused step launch,
        shape [n, 2] (diagnostic -DZS_STAMPS build only)."""
        out = np.zeros((n, 2), dtype=np.uint64)
        self._call("zs_debug_timeline", C.c_void_p(out.ctypes.data), n)
        return out

    def debug_lists(self):
        """(pending-reset count of list 0, of list 1, deferred-respawn count, parity drained next)."""
        out = (C.c_int32 * 4)()
        self._call("zs_debug_lists", out, self._stream())
        return tuple(int(v) for v in out)

    def death_log(self, env):
        """The things env's last step removed in clean_dead_things (core.py:121-138), in removal order:
        a list of (slot, serial, x, y, life).  Needs a config with FLAG_DEATH_LOG."""
        out = (C.c_int32 * (5 * max(1, self.E)))()
        n = C.c_int32(0)
        self._call("zs_death_log", int(env), out, int(self.E), C.byref(n), self._stream())
        return decode_death_log(np.frombuffer(out, dtype=np.int32), n.value, self.E)

    def action_log(self, env):
        """The actions env's last step executed, in execution order (core.py:76,103-119): a list of
        (slot, kind, target), kind 1 move (target: destination x | y << 16), 2 attack, 3 heal (target: an
        entity slot, or -1 - obstacle index).  Needs a config with FLAG_DEATH_LOG.  Returns (actions, raised):
        raised when a debug raise stopped the step, the actions then being the decided actions of the actors
        before the raising one, in dict order."""
        out = (C.c_int32 * (2 * max(1, self.E)))()
        n = C.c_int32(0)
        self._call("zs_action_log", int(env), out, int(self.E), C.byref(n), self._stream())
        return decode_action_log(np.frombuffer(out, dtype=np.int32), n.value, self.E)

    # -- the drop-ins' per-call path (zs_host_*): one copy in, one copy out, one synchronisation ----------
    def host_layout(self):
        """Word offsets of a zs_host_* record's sections (zs_host_layout)."""
        return self._layout("zs_host_layout")

    def host_record(self):
        """A fresh record buffer for one zs_host_* call over all N envs (int32 [N][words])."""
        return np.empty((self.N, self.host_layout()["words"]), dtype=np.int32)

    def host_step(self, actions, rng, rec):
        """zs_host_step: actions int32 [N, A, 3] (host), rng [N][625] uint32 words (random.getstate() form;
        a numpy array or packed bytes) or None, rec from host_record() (filled)."""
        a = np.ascontiguousarray(actions, dtype=np.int32)
        self._call("zs_host_step", C.c_void_p(a.ctypes.data), _np_ptr(rng), C.c_void_p(rec.ctypes.data), self._stream())
        return rec

    def host_reset(self, rng, rec):
        """zs_host_reset: every env rebuilt (Game.__initialize_world__), record filled.  On ZS_ENOSPACE the
        record still holds the envs' streams (the caller moves them back before re-raising)."""
        self._call("zs_host_reset", _np_ptr(rng), C.c_void_p(rec.ctypes.data), self._stream())
        return rec

    def host_observe(self, rec):
        self._call("zs_host_observe", C.c_void_p(rec.ctypes.data), self._stream())
        return rec

    def get_state(self, env):
        buf = np.zeros(self.state_words, dtype=np.int32)
        self._call("zs_get_state", int(env), C.c_void_p(buf.ctypes.data), self._stream())
        return StateView(self, buf)

    def set_state(self, env, view):
        self._call("zs_set_state", int(env), C.c_void_p(view.buf.ctypes.data), self._stream())

    def overflow(self, clear=False):
        """Sticky range flags (_abi.OVF_INT16 | OVF_INT32 | OVF_PARAM_RANGE) of every env since creation / the last clear."""
        f = C.c_uint32(0)
        self._call("zs_overflow", C.byref(f), 1 if clear else 0, self._stream())
        return int(f.value)

    def check_lossless(self):
        """Raise OverflowError when an obstacle life left what this engine's outputs hold exactly: below
        the int16 range with int16 observations, or saturated at -2**31 + 1."""
        f = self.overflow()
        if f & _abi.OVF_INT32:
            raise OverflowError("an obstacle life fell below -2147483647 and saturated (reference: unbounded int)")
        if (f & _abi.OVF_INT16) and self.obs_dtype == self.torch.int16:
            raise OverflowError("an obstacle life fell below -32768: int16 observations saturated it")

    def get_rng(self, env):
        """(mt[624] uint32, index) of env's MT19937 stream, CPython getstate() form."""
        buf = np.zeros(625, dtype=np.uint32)
        self._call("zs_get_rng", int(env), C.c_void_p(buf.ctypes.data), self._stream())
        return buf

    def set_rng(self, env, state):
        buf = np.ascontiguousarray(np.asarray(state, dtype=np.uint32).reshape(625))
        self._call("zs_set_rng", int(env), C.c_void_p(buf.ctypes.data), self._stream())

    def load_python_random(self, env, rnd=None):
        """Move a `random.Random` (default: the module-global one) state into env."""
        import random as _random
        st = (rnd or _random).getstate()
        self.set_rng(env, np.asarray(st[1], dtype=np.uint64).astype(np.uint32))

    def store_python_random(self, env, rnd=None):
        """Write env's stream back into a `random.Random` (default: the module-global one)."""
        import random as _random
        buf = self.get_rng(env)
        r = rnd or _random
        r.setstate((3, tuple(int(v) for v in buf), None))


class StepOutputs(object):
    """One set of zs_step output buffers, `rows` >= N rows (rows past N are padding the engine never
    writes: equal-sized shards for a collective).  Everything but the observations lives in one flat byte
    tensor (`flat`), so a per-step exchange moves it in one collective (obs + reward +
    done/trunc/alive): float64 rewards [rows][R], then done [rows], truncated [rows], listed [rows][A] (the
    agents alive before the step: the keys of the reference's per-agent dicts, gym/multiagent_env.py:156-169)
    and was_reset [rows] (the observation is a reset's)."""

    @staticmethod
    def row_bytes(eng):
        R = eng.A if eng.multi else 1
        return 8 * R + 3 + eng.A

    def __init__(self, eng, rows, obs=None, flat=None):
        torch = eng.torch
        kw = dict(device=eng.device)
        R = eng.A if eng.multi else 1
        A = eng.A
        self.rows = rows
        nb = rows * self.row_bytes(eng)
        grid = getattr(eng, "grid_obs", True)
        if obs is not None:
            assert grid, "an engine built with grid_obs=False writes no observations"
            assert obs.shape == (rows,) + tuple(eng.obs_shape) and obs.dtype == eng.obs_dtype and obs.is_contiguous()
        if flat is not None:
            assert flat.dim() == 1 and flat.numel() >= nb and flat.dtype == torch.uint8
            assert flat.is_contiguous() and flat.storage_offset() % 8 == 0
        self.obs = obs if obs is not None or not grid else torch.zeros((rows,) + eng.obs_shape, dtype=eng.obs_dtype, **kw)
        self.flat = flat if flat is not None else torch.zeros(nb, dtype=torch.uint8, **kw)
        o = 8 * R * rows
        self.rewards = self.flat[:o].view(torch.float64).view(rows, R)
        self.done = self.flat[o:o + rows]
        self.trunc = self.flat[o + rows:o + 2 * rows]
        self.listed = self.flat[o + 2 * rows:o + (2 + A) * rows].view(rows, A)
        self.was_reset = self.flat[o + (2 + A) * rows:o + (3 + A) * rows]


class StateView(object):
    """Decoded zs_get_state record (layout: include/zombsole_mi355x.h)."""

    def __init__(self, eng, buf):
        self.buf = buf
        b = buf
        self.E, self.O, self.W, self.H = int(b[6]), int(b[7]), int(b[8]), int(b[9])
        self.A = eng.A
        self.P = eng.builder.num_bots
        o = _abi.STATE_HEADER
        self.ent = b[o:o + _abi.STATE_ENTITY_WORDS * self.E].reshape(self.E, _abi.STATE_ENTITY_WORDS)
        o += _abi.STATE_ENTITY_WORDS * self.E
        self.order = b[o:o + self.E]
        o += self.E
        self.obst_life = b[o:o + self.O]
        o += self.O
        self.obst_present = b[o:o + self.O]
        o += self.O
        self.prev_life = b[o:o + self.A]
        o += self.A
        self.listed = b[o:o + self.A]
        o += self.A
        dw = (self.W * self.H + 31) // 32
        self.dead_words = b[o:o + dw]

    t = property(lambda s: int(s.buf[0]))
    deaths = property(lambda s: int(s.buf[1]))
    zombie_deaths = property(lambda s: int(s.buf[2]))
    n_order = property(lambda s: int(s.buf[4]))

    def dead_cells(self):
        w = self.dead_words.astype(np.uint32)
        bits = np.unpackbits(w.view(np.uint8), bitorder="little")
        return [int(c) for c in np.nonzero(bits[:self.W * self.H])[0]]

    def canonical(self, obstacle_kinds):
        """The canonical state dict of tests/golden records."""
        dyn = []
        for s in self.order[:self.n_order]:
            r = self.ent[int(s)]
            dyn.append([int(r[0]), int(r[2]), int(r[3]), int(r[4]), int(r[5]), int(r[6])])
        obst = []
        for i in range(self.O):
            ml = 10 if obstacle_kinds[i] == _abi.THING_BOX else 200
            if int(self.obst_life[i]) != ml or not self.obst_present[i]:
                obst.append([i, int(self.obst_life[i]), int(self.obst_present[i])])
        agents = [[int(r[2]), int(r[3]), int(r[4]), int(r[5])] for r in self.ent[:self.A]]
        players = [[int(r[2]), int(r[3]), int(r[4]), int(r[5])] for r in self.ent[self.A:self.A + self.P]]
        return {"dyn": dyn, "obst": obst, "dead": self.dead_cells(), "ctr": [self.t, self.deaths, self.zombie_deaths],
                "agents": agents, "players": players}
