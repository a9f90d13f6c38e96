"""Batched device API: N lock-step envs of one surface on one GPU, env-sharded across ranks.

This is the throughput path (`bench.py`).  The drop-in classes in
`gym_env` / `gym.multiagent_env` drive one env each through the same engine; here the
caller hands whole-batch device tensors in and gets device tensors back:

    venv = BatchedZombsole("multi", 8192, rules_name="extermination", player_names=[],
                           map_name="bridge64", agent_ids=["0", "1"], initial_zombies=10,
                           max_episode_steps=1000, base_seed=0, env0=rank * 8192)
    obs = venv.reset()                                  # [N, A, 3, 21, 21] on the GPU
    obs, rew, done, trunc = venv.step(actions)          # actions int32 [N, A, 3] or ids [N, A]

Envs are independent: rank r of G owns global envs [r*N/G, (r+1)*N/G) and env i is seeded
`base_seed + i` (CPython random.seed semantics per env), so every env's trajectory is the
same whatever G is.  Done/truncated envs are reset by the next step (autoreset); the
`was_reset` tensor flags them.  The only collective is the optional observation gather
for a centralised learner (`gather_observations`, RCCL all-gather over xGMI).
"""
from . import _abi
from .actions import DISCRETE_TRIPLES
from .engine import Engine, as_index


def shard_range(total_envs, rank, world):
    """(first global env, count) of `rank`'s shard; contiguous, sizes differ by <= 1."""
    base, extra = divmod(int(total_envs), int(world))
    n = base + (1 if rank < extra else 0)
    env0 = rank * base + min(rank, extra)
    return env0, n


CHECKPOINT_KEYS = ("records", "fingerprint", "rec_bytes", "num_envs", "env0", "base_seed")


def write_checkpoint(path, records, fingerprint, num_envs, env0=0, base_seed=0):
    """torch.save of a checkpoint: `records` (uint8 [num_envs, rec_bytes], any device; stored on the CPU) with what
    load needs to refuse a file of another configuration.  Plain tensors in, no engine."""
    import torch
    if records.dim() != 2 or records.dtype != torch.uint8 or records.shape[0] != int(num_envs):
        raise ValueError("write_checkpoint: records must be uint8 [num_envs = %d, rec_bytes]" % int(num_envs))
    torch.save({"records": records.detach().cpu().contiguous(), "fingerprint": int(fingerprint),
                "rec_bytes": int(records.shape[1]), "num_envs": int(num_envs), "env0": int(env0),
                "base_seed": int(base_seed)}, path)


def read_checkpoint(path, fingerprint, rec_bytes, num_envs):
    """torch.load of a write_checkpoint file, on the CPU.  ValueError when its fingerprint, record size or env
    count is not the expected one (or the file is no checkpoint); returns the dict."""
    import torch
    ck = torch.load(path, map_location="cpu")
    if not isinstance(ck, dict) or any(k not in ck for k in CHECKPOINT_KEYS):
        raise ValueError("read_checkpoint: %s is not a checkpoint (keys %s)" % (path, ", ".join(CHECKPOINT_KEYS)))
    rec = ck["records"]
    if ck["fingerprint"] != int(fingerprint):
        raise ValueError("read_checkpoint: fingerprint %#x, expected %#x: the checkpoint is of another map, entity "
                         "counts, rules or static tables" % (ck["fingerprint"], int(fingerprint)))
    if ck["rec_bytes"] != int(rec_bytes) or rec.dim() != 2 or rec.shape[1] != int(rec_bytes) or rec.dtype != torch.uint8:
        raise ValueError("read_checkpoint: records of %d bytes, expected %d" % (ck["rec_bytes"], int(rec_bytes)))
    if ck["num_envs"] != int(num_envs) or rec.shape[0] != int(num_envs):
        raise ValueError("read_checkpoint: %d envs, expected %d" % (ck["num_envs"], int(num_envs)))
    return ck


class BatchedZombsole(object):
    def __init__(self, surface, num_envs, rules_name, player_names, map_name, agent_ids=None, agent_id=0,
                 initial_zombies=0, minimum_zombies=0, max_episode_steps=0, base_seed=0, env0=0,
                 observation_scope="world", observation_position_encoding="simple", agent_weapon="rifle",
                 observation_surroundings_width=21, observation_position_encoding_style="channels",
                 agent_weapons="rifle", obs_dtype=None, autoreset=True, device=None, lanes_per_env=0,
                 action_masks=False, env_params=False, episode_stats=False, render=False, entity_obs=None,
                 grid_obs=True, autopilot=None, autopilot_into_actions=False, nav=None, nav_max_dist=32766,
                 entity_actions=False):
        if entity_actions and entity_obs is None:
            raise ValueError("entity_actions=True needs entity_obs=(kz, kp): the table's rows are the entity observation's")
        if surface == "single":
            b = _abi.single_env_config(num_envs, rules_name, player_names, map_name, agent_id, initial_zombies,
                                       minimum_zombies, observation_scope, observation_position_encoding,
                                       agent_weapon, max_episode_steps,
                                       _abi.DTYPE_I32 if obs_dtype is None else obs_dtype, autoreset, lanes_per_env,
                                       env_params=env_params, episode_stats=episode_stats, render=render)
        elif surface == "multi":
            b = _abi.multi_env_config(num_envs, rules_name, player_names, map_name, agent_ids, initial_zombies,
                                      minimum_zombies, observation_surroundings_width,
                                      observation_position_encoding_style, agent_weapons, max_episode_steps,
                                      _abi.DTYPE_I64 if obs_dtype is None else obs_dtype, autoreset, lanes_per_env,
                                      env_params=env_params, episode_stats=episode_stats, render=render)
        else:
            raise ValueError("surface must be 'single' or 'multi'")
        self.surface = surface
        if not grid_obs and entity_obs is None:
            raise ValueError("grid_obs=False needs entity_obs=(kz, kp): the env would have no observation")
        self.engine = Engine(b, device=device, grid_obs=grid_obs)
        self.torch = self.engine.torch
        self.num_envs = int(num_envs)
        self.env0 = int(env0)
        self.base_seed = int(base_seed)
        self.engine.seed([self.base_seed + self.env0 + i for i in range(self.num_envs)])
        self._triples = self.torch.from_numpy(DISCRETE_TRIPLES).to(self.engine.device)
        self.n_discrete = 7 if surface == "multi" else 6
        # action_masks=True: a mask tensor bound to the engine, so every step ends with the mask launch; reset,
        # restore, clone and load_checkpoint launch it themselves
        if action_masks:
            self.engine.bind_action_masks()
        # entity_obs=(kz, kp): an entity-observation tensor bound the same way, refreshed at the same places.
        # grid_obs=False: no grid observation is allocated or written; the entity tensor is the observation
        if entity_obs is not None:
            self.engine.bind_entity_obs(True, int(entity_obs[0]), int(entity_obs[1]))
        # entity_actions=True: the entity action table over those rows (libzombsole_amd/entity_act.py): its masks bound
        # and refreshed the same way, and an id buffer that step(ids) binds, so the step's first launch decodes it
        self._eact_ids = None
        if entity_actions:
            kz, kp = int(entity_obs[0]), int(entity_obs[1])
            self._eact_ids = self.torch.zeros((self.num_envs, self.engine.A), dtype=self.torch.int32, device=self.engine.device)
            self.engine.bind_entity_act(None, True, kz, kp)
        # nav=("objective", "zombies") | "objective" | "zombies": path-distance rows (libzombsole_amd/nav.py) bound the
        # same way, refreshed at the same places
        if nav is not None:
            self.engine.nav_bind(True, nav, nav_max_dist)
        # autopilot="terminator" | "sniper" | "troll" | uint8 [N, A] codes: scripted triples bound the same way
        # (libzombsole_amd/autopilot.py), refreshed at the same places.  autopilot_into_actions=True binds the engine's
        # action buffer: a step's last launch writes the rows the next step reads
        if autopilot is not None:
            self.engine.bind_autopilot(autopilot, into_actions=bool(autopilot_into_actions))

    @property
    def scripted_actions(self):
        """int32 [N, A, 3]: the engine's bound scripted triples for the world self.obs shows, rows of policy code 0 left
        as they were.  Valid after every reset, step, restore / clone and load_checkpoint.  None without autopilot=."""
        return self.engine.pilot

    def set_autopilot(self, policy):
        """Write the bound policy tensor (a name, a code, or codes that broadcast to [N, A]); no synchronisation.  The
        next launch (the next step's last, or a reset / restore) decides with it."""
        eng = self.engine
        if eng.pilot_policy is None:
            raise ValueError("set_autopilot: no autopilot is bound (BatchedZombsole(autopilot=...))")
        if isinstance(policy, (str, int)):
            from .autopilot import policy_code
            eng.pilot_policy.fill_(policy_code(policy))
        else:
            eng.pilot_policy.copy_(self.torch.as_tensor(policy).to(eng.device).expand(eng.N, eng.A))

    def step_scripted(self, graph=True):
        """step(self.scripted_actions): every agent slot of nonzero code played by its scripted policy."""
        if self.engine.pilot is None:
            raise ValueError("step_scripted: no autopilot is bound (BatchedZombsole(autopilot=...))")
        return self.step(self.engine.pilot, graph=graph)

    def _refresh(self, mask=None):
        """The bound side tensors of the envs whose mask byte is nonzero (None: all), after a call that is no step."""
        eng = self.engine
        if eng.masks is not None:
            eng.action_mask(mask)
        if eng.entities is not None:
            eng.entity_obs(mask)
        if eng.entity_act_masks is not None:
            eng.entity_act_mask(mask)
        if eng.nav is not None:
            eng.nav_obs(mask)
        if eng.pilot is not None:
            eng.autopilot(eng.pilot_policy, mask, out=eng.pilot)

    @property
    def nav_obs(self):
        """int16 [N, A, F, 8]: the engine's bound path-distance rows (libzombsole_amd/nav.py) of the world self.obs shows.
        Valid after every reset, step, restore / clone and load_checkpoint.  None without nav=."""
        return self.engine.nav

    def nav_field(self, which, envs=None, out=None):
        """Engine.nav_field with the bound cap: the full field `which` of `envs` (default: all), uint16 [n, H, W] on the
        device, 0xFFFF = unreachable or blocked."""
        args = self.engine.nav_args
        return self.engine.nav_field(which, envs, out, max_dist=args[1] if args else None)

    @property
    def entity_obs(self):
        """int16 [N, A, 16 + 4 (kz + kp)]: the engine's bound entity observations (libzombsole_amd/entity_obs.py) of
        the world self.obs shows.  Valid after every reset, step, restore / clone and load_checkpoint.  None without
        entity_obs=(kz, kp)."""
        return self.engine.entities

    # -- entity-targeted actions (entity_actions=True): a table of 15 + kz + kp ids per agent -------------------------
    @property
    def n_entity_actions(self):
        """NID = 15 + kz + kp, the ids of the entity action table (libzombsole_amd/entity_act.py).  None without
        entity_actions=True."""
        return None if self._eact_ids is None else self.engine.entity_act_layout()["nid"]

    @property
    def entity_action_masks(self):
        """uint8 [N, A, NID] (a view of the engine's bound [N, A, row_bytes] tensor): entry i of agent a is 1 when the
        reference would carry out the table's action i for it on the world self.obs shows; all 0 for an agent not in the
        world.  Valid after every reset, step, restore / clone and load_checkpoint.  None without entity_actions=True."""
        m = self.engine.entity_act_masks
        return None if m is None else m[:, :, :self.n_entity_actions]

    def encode_actions(self, triples=None):
        """The table's ids of `triples` (int32 [N, A, 3]; default self.scripted_actions, the bound autopilot's: the
        teacher's labels over this table) on the current world, int32 [N, A], -1 where the table has no such entry."""
        if self._eact_ids is None:
            raise ValueError("encode_actions: no entity action table (BatchedZombsole(entity_actions=True))")
        if triples is None:
            triples = self.scripted_actions
            if triples is None:
                raise ValueError("encode_actions: no triples given and no autopilot is bound")
        t = self.torch
        return self.engine.entity_act_encode(triples.to(self.engine.device).to(t.int32).contiguous())

    def _bind_entity_ids(self, on):
        """The id buffer bound (the step begins with its decode) or not (the step takes the caller's triples); the
        masks stay bound.  A change of form drops the cached step graphs once."""
        eng = self.engine
        if (eng.entity_act_ids is not None) != on:
            eng.bind_entity_act(self._eact_ids if on else None, eng.entity_act_masks, *eng.entity_act_k)

    def _observation(self):
        return self.engine.obs if self.engine.grid_obs else self.engine.entities

    @property
    def action_masks(self):
        """uint8 [N, A, n_discrete] (a view of the engine's bound [N, A, 8] tensor): entry k of agent a is 1 when
        discrete action k would succeed for it on the world self.obs shows; all 0 for an agent not in the world.
        Valid after every reset, step, restore / clone and load_checkpoint.  None without action_masks=True."""
        m = self.engine.masks
        return None if m is None else m[:, :, :self.engine.n_discrete]

    # -- per-env difficulty (env_params=True): zombie counts and time limit per env, set on the device --------------
    def set_env_params(self, params, envs=None, check=True):
        """(initial_zombies, minimum_zombies, max_episode_steps) per env, taken up at each env's next reset
        (Engine.set_env_params): int32 [n, 3] or a dict of three [n] tensors, for `envs` (default 0..n-1).  The
        constructor's counts are the caps.  check=False never synchronises."""
        self.engine.set_env_params(params, envs, check)

    @property
    def env_params(self):
        """int32 [N, 3]: the triple every env takes up at its next reset."""
        return self.engine.env_params()

    @property
    def env_params_current(self):
        """int32 [N, 3]: the triple of every env's running episode."""
        return self.engine.env_params(current=True)

    # -- episode statistics (episode_stats=True): returns, lengths and outcomes per env, kept on the device ---------
    def episode_stats(self, mask=None):
        """Engine.episode_stats: a dict of "run_ret", "last_ret", "sum_ret" (float64 [N, R]), "last" and "tot" (int32
        [N, 8]; _abi.EP_LAST, _abi.EP_TOT) on the device.  Correct at any number of steps per launch."""
        return self.engine.episode_stats(mask)

    def clear_episode_stats(self, mask=None):
        """Zero the last finished episode and the totals of the masked envs (default: all); running returns stay."""
        self.engine.clear_episode_stats(mask)

    def episode_totals(self, groups=None, n_groups=1):
        """The totals summed over groups of envs (e.g. curriculum levels): `groups` int64 [N] with values in
        [0, n_groups) (default: one group).  Returns {"tot": int64 [n_groups, 8], "sum_ret": float64 [n_groups, R]}, a
        torch.index_add_ of the per-env tensors; no synchronisation."""
        t = self.torch
        st = self.engine.episode_stats()
        g = t.zeros(self.num_envs, dtype=t.int64, device=self.engine.device) if groups is None else \
            t.as_tensor(groups).to(device=self.engine.device, dtype=t.int64)
        tot = t.zeros((int(n_groups), 8), dtype=t.int64, device=self.engine.device)
        tot.index_add_(0, g, st["tot"].to(t.int64) & 0xffffffff)
        ret = t.zeros((int(n_groups), st["sum_ret"].shape[1]), dtype=t.float64, device=self.engine.device)
        ret.index_add_(0, g, st["sum_ret"])
        return {"tot": tot, "sum_ret": ret}

    # -- frames (render=True): the envs' picture, drawn on the device ------------------------------------------------
    def render(self, envs=None, out=None):
        """Engine.render: uint8 [n, 10 H, 10 W, 3] RGB frames of `envs` (default: all) on the device, pixel-exact to
        the map area of the reference's OpencvRenderer; no synchronisation."""
        return self.engine.render(envs, out)

    @property
    def obs(self):
        return self.engine.obs

    @property
    def was_reset(self):
        return self.engine.was_reset

    @property
    def listed(self):
        return self.engine.listed

    def reset(self, mask=None):
        self.engine.reset(mask)
        self._refresh(mask)
        return self._observation()

    def discrete_to_triples(self, ids):
        """Discrete(6)/(7) ids [N, A] (gym_env.py:328-351, gym/multiagent_env.py:259-285) -> [N, A, 3]."""
        return self._triples[ids.long()]

    @property
    def actions(self):
        """The engine's action buffer, int32 [N, A, 3]: a caller that writes its actions here (e.g.
        `torch.index_select(..., out=venv.actions.view(-1, 3))`) saves step()'s copy."""
        return self.engine.actions

    def step(self, actions, graph=True):
        """One tick of every env on the caller's actions (int32 [N, A, 3] triples, or Discrete ids
        [N, A]), as MultiagentZombsoleEnv.step / ZombsoleGymEnv.step do per env
        (gym/multiagent_env.py:111-171, gym_env.py:99-145).  graph=True replays the step as one hipGraph
        launch reading the engine's action buffer (Engine.step_graphed); graph=False dispatches its
        kernels one by one (zs_step).  With entity_actions=True an integer [N, A] tensor holds ids of the entity
        action table (0..6 are the Discrete(7) ids), written into the bound id buffer and decoded by the step's first
        launch against each env's current world; an [N, A, 3] tensor is still taken as triples."""
        t = self.torch
        if self._eact_ids is not None:
            self._bind_entity_ids(actions.dim() == 2)
            if actions.dim() == 2:  # the table's ids: the step's first launch decodes them into the action buffer
                self._eact_ids.copy_(actions)
                eng = self.engine
                return self._stepped(eng.step_graphed(eng.actions) if graph else eng.step(eng.actions))
        if actions.dim() == 2:
            actions = self.discrete_to_triples(actions)
        if not graph:
            if actions.dtype != t.int32 or not actions.is_contiguous():
                actions = actions.to(t.int32).contiguous()
            return self._stepped(self.engine.step(actions))
        buf = self.engine.actions
        if actions.data_ptr() != buf.data_ptr():
            buf.copy_(actions)
        return self._stepped(self.engine.step_graphed(buf))

    def _stepped(self, res):
        # grid_obs=False: the step's observation is the bound entity tensor
        return res if self.engine.grid_obs else (self.engine.entities,) + tuple(res[1:])

    def sample_actions(self, step):
        """The bench/parity uniform policy, generated on device (zs_gen_actions)."""
        return self.engine.gen_actions(step, self.n_discrete)

    # -- snapshot, restore, clone, checkpoints (Engine.snapshot / restore: complete envs as device records) -----
    def snapshot(self, envs=None):
        """The snapshot records of `envs` (default: all), uint8 [n, rec_bytes] on the device."""
        return self.engine.snapshot(envs)

    def restore(self, snap, src=None, dst=None, observe=True, check=True):
        """Record src[k] of `snap` (default: k) into env dst[k] (default: k); see Engine.restore.  observe=True
        re-encodes the written envs (a masked observe) and returns self.obs, whose other rows are untouched (with
        grid_obs=False: the entity tensor, which is refreshed whenever one is bound)."""
        eng, t = self.engine, self.torch
        eng.restore(snap, src, dst, check=check)
        if (not observe and self.engine.masks is None and self.engine.entities is None and self.engine.pilot is None and
                self.engine.nav is None):
            return None
        mask = t.zeros(eng.N, dtype=t.uint8, device=eng.device)
        if dst is None:
            n = snap.shape[0] if src is None else len(src)
            mask[:min(int(n), eng.N)] = 1
        else:
            d = as_index(t, dst, eng.device, "restore").long()
            mask[d[(d >= 0) & (d < eng.N)]] = 1
        self._refresh(mask)  # the written envs' action masks, entity rows and scripted triples, beside their observations
        if not observe:
            return None
        return eng.observe(mask) if eng.grid_obs else eng.entities

    def clone(self, src, dst, observe=True):
        """Env dst[k] becomes a copy of env src[k] (fork; sources may repeat).  The copy goes through records in a
        scratch tensor, so overlapping src / dst sets are safe: every destination gets its source's state as it
        was before the call."""
        return self.restore(self.engine.snapshot(src), None, dst, observe=observe)

    def save_checkpoint(self, path):
        """Every env's snapshot record and what identifies the run (write_checkpoint) into `path`."""
        L = self.engine.snapshot_layout()
        write_checkpoint(path, self.engine.snapshot(), L["fingerprint"], self.num_envs, self.env0, self.base_seed)

    def load_checkpoint(self, path, observe=True):
        """Restore every env from a save_checkpoint file of the same configuration and env count (ValueError
        otherwise, before the engine is touched).  The action-stream seeds are not part of a checkpoint: they are
        this object's own (base_seed, env0)."""
        L = self.engine.snapshot_layout()
        ck = read_checkpoint(path, L["fingerprint"], L["rec_bytes"], self.num_envs)
        return self.restore(ck["records"].to(self.engine.device), observe=observe)

    def close(self):
        self.engine.close()


def _gather_sizes(n_local, device, group):
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    t = torch.tensor([int(n_local)], dtype=torch.int64, device=device)
    parts = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(parts, t, group=group)
    return [int(p.item()) for p in parts]


def _all_gather_rows(out, x, group):
    """out[r*m:(r+1)*m] = rank r's x (every rank's x has m rows).

    RCCL has no int16 type (the compact C5 observations): such tensors travel as their bytes."""
    import torch
    import torch.distributed as dist
    if dist.get_backend(group) == "gloo":
        dist.all_gather(list(out.chunk(dist.get_world_size(group), dim=0)), x, group=group)
        return
    if x.dtype in (torch.int16, torch.uint16, torch.bool):
        out, x = out.view(torch.uint8), x.view(torch.uint8)
    dist.all_gather_into_tensor(out, x, group=group)


def gather_observations(obs, group=None, sizes=None):
    """All-gather every rank's observation shard into one [sum(N_r), ...] tensor in global env
    order.

    Shards from `shard_range` differ by at most one env: short shards are padded to the longest, so
    every rank issues one equal-sized collective.  `sizes` (every rank's shard size, e.g. from
    shard_range) saves a size exchange and its host sync per call; per-step callers should use
    StepGather, which also overlaps the exchange with the next step.  Over RCCL on MI355X it is one
    all_gather_into_tensor; with gloo (CPU tests) the same call on host tensors."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    if sizes is None:
        sizes = _gather_sizes(obs.shape[0], obs.device, group)
    sizes = [int(v) for v in sizes]
    m = max(sizes)
    x = obs.contiguous()
    if x.shape[0] < m:
        x = torch.cat([x, x.new_zeros((m - x.shape[0],) + tuple(x.shape[1:]))], dim=0)
    out = torch.empty((world * m,) + tuple(obs.shape[1:]), dtype=obs.dtype, device=obs.device)
    _all_gather_rows(out, x, group)
    if all(n == m for n in sizes):
        return out
    return torch.cat([out[r * m:r * m + n] for r, n in enumerate(sizes)], dim=0)


class StepGather(object):
    """C5's per-step exchange for a centralised learner, overlapped with the next
    step's compute.

    Every rank's observation shard plus its rewards / done / truncated / listed / was_reset are
    all-gathered into node-wide tensors (obs + reward + done/trunc/alive; `listed` says
    which agents' rewards and observations are valid — the agents alive before the step, whose keys the
    reference's dicts carry, gym/multiagent_env.py:156-169 — and `was_reset` which observations are a reset's).
    The engine writes each step into one of `depth` output sets (Engine.outputs) whose storage
    is this rank's slice of that set's gather buffers, padded to the longest shard, so the exchange copies
    nothing: the collectives run in place (a rank receives the other ranks' slices only), the observations
    one collective and the rest (one flat byte tensor per set, engine.StepOutputs) a second.  Step t
    writes set t % depth on the caller's stream; its collectives are issued on a communication stream
    that waits for that step only, so they run while step t + 1 computes into the next set; before a
    set is written again the caller's stream waits for the collectives that read it.  With gloo (CPU
    tensors) everything is synchronous.

        g = StepGather(eng)
        g.step(lambda out: eng.step_graph(t, 7, out=out))   # per step
        g.obs(), g.rewards(), g.done(), g.truncated()      # the last step's node-wide tensors
        g.listed(), g.was_reset()

    The tensors obs() returns are the exchange buffers themselves when every shard has the same size
    (no copy): they hold step t's values until the exchange of step t + depth overwrites them, and are
    ordered on the current stream only (obs(copy=True) returns a copy).  A consumer that reads a step's
    gathered values on the communication stream instead (a learner overlapping with the next step)
    passes after=fn to step(): fn(k) runs there right after the collectives that fill set k.

    mode="state" exchanges observation-state records instead of observations (Engine.pack_obs_state: what the
    encoders read of an env, 1 584 B against 10 584 B of observations at C5).  After run(out) the rank packs
    its envs into its slice of g_state[k] (uint8 [world * m, rec_bytes], out.state) on the caller's stream; the
    communication stream all-gathers g_state[k] and the flat buffer, unpacks all world * m records into
    `viewer` (an Engine built with viewer=True and world * m envs; default: one built from the engine's
    config) and re-encodes them into g_obs[k] (viewer.observe) before after(k).  obs(), rewards(), ... and
    the pending-event protocol mean what they mean in mode="obs", and the values are the same.  The step
    still writes the rank's own observations (into its slice of g_obs[k], which the viewer then rewrites
    with the same values).  Padding rows carry zero records; _rows drops what they decode to.  At world size
    1 the collectives are skipped as in mode="obs"; pack, unpack and re-encode still run.
    """

    def __init__(self, engine, group=None, depth=2, self_exchange=False, mode="obs", viewer=None):
        import torch
        import torch.distributed as dist
        self.torch = torch
        self.eng = engine
        self.group = group
        self.world = dist.get_world_size(group)
        self.n = engine.N
        self.sizes = _gather_sizes(self.n, engine.device, group)  # once: shards keep their size
        self.m = max(self.sizes)
        self.R = engine.A if engine.multi else 1
        self.depth = int(depth)
        dev = engine.device
        rank = dist.get_rank(group)
        shape = tuple(engine.obs_shape)
        self.A = engine.A
        # a rank's segment of the flat exchange buffer (engine.StepOutputs); the float64 rewards 8-B aligned
        nflat = (self.m * (8 * self.R + 3 + self.A) + 15) // 16 * 16
        self.g_obs = [torch.zeros((self.world * self.m,) + shape, dtype=engine.obs_dtype, device=dev)
                      for _ in range(self.depth)]
        self.g_flat = [torch.zeros(self.world * nflat, dtype=torch.uint8, device=dev) for _ in range(self.depth)]
        # the engine's output sets are this rank's slices of the gather buffers (in-place collectives)
        self.sets = [engine.outputs(rows=self.m, obs=self.g_obs[k][rank * self.m:(rank + 1) * self.m],
                                    flat=self.g_flat[k][rank * nflat:(rank + 1) * nflat]) for k in range(self.depth)]
        cuda = dev.type == "cuda"
        self.comm = torch.cuda.Stream(device=dev) if cuda else None
        self.pending = [None] * self.depth  # per set: event after the collectives that read it
        # world size 1: the output sets are the whole gather buffers, so the gathered tensors are already
        # complete and the collectives are skipped (self_exchange=True issues them anyway: diagnostics of
        # the exchange's fixed cost)
        self.skip = self.world == 1 and not self_exchange
        self.t = 0
        self.last = None
        if mode not in ("obs", "state"):
            raise ValueError("mode must be 'obs' or 'state'")
        self.mode = mode
        self.viewer = self.g_state = None
        if mode == "state":
            nb = engine.obs_state_layout()["rec_bytes"]
            rows = self.world * self.m
            self.g_state = [torch.zeros((rows, nb), dtype=torch.uint8, device=dev) for _ in range(self.depth)]
            for k, out in enumerate(self.sets):  # the rank's records: its slice of the exchanged tensor
                out.state = self.g_state[k][rank * self.m:(rank + 1) * self.m]
            self._own_viewer = viewer is None
            if viewer is None:
                viewer = type(engine)(engine.builder.viewer(rows), device=dev.index)
            if viewer.N != rows or viewer.obs_state_layout()["rec_bytes"] != nb:
                raise ValueError("viewer must hold world * m = %d envs of the engine's record (%d bytes)" % (rows, nb))
            self.viewer = viewer

    def close(self):
        """Free the viewer this object built (mode="state" without a viewer argument)."""
        if self.viewer is not None and self._own_viewer:
            self.viewer.close()
        self.viewer = None

    def _exchange(self, k, out):
        """Set k's collectives (unless skipped) and, in mode="state", the viewer's unpack and re-encode, on
        the current stream."""
        if self.mode == "obs":
            if not self.skip:
                _all_gather_rows(self.g_obs[k], out.obs, self.group)
                _all_gather_rows(self.g_flat[k], out.flat, self.group)
            return
        if not self.skip:
            _all_gather_rows(self.g_state[k], out.state, self.group)
            _all_gather_rows(self.g_flat[k], out.flat, self.group)
        self.viewer.unpack_obs_state(self.g_state[k])
        self.viewer.observe(out=self.g_obs[k])

    def step(self, run, after=None):
        """run(out) issues one engine step into output set `out` on the current stream; the step's
        exchange follows on the communication stream, then after(k) (if given) on that stream, with
        g_obs[k] / g_flat[k] holding the step's gathered values.  Returns the set used."""
        torch = self.torch
        k = self.t % self.depth
        out = self.sets[k]
        if self.pending[k] is not None:
            torch.cuda.current_stream(self.eng.device).wait_event(self.pending[k])
        run(out)
        if self.mode == "state":
            self.eng.pack_obs_state(out=out.state)
        if self.skip:
            self._exchange(k, out)
            if after is not None:
                after(k)
        elif self.comm is not None:
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self.eng.device))
            self.comm.wait_event(done)
            with torch.cuda.stream(self.comm):
                self._exchange(k, out)
                if after is not None:
                    after(k)
                ev = torch.cuda.Event()
                ev.record(self.comm)
            self.pending[k] = ev
        else:
            self._exchange(k, out)
            if after is not None:
                after(k)
        self.last = k
        self.t += 1
        return out

    def wait(self):
        """Make the current stream wait for the last step's exchange (before reading its results)."""
        if self.last is not None and self.pending[self.last] is not None:
            self.torch.cuda.current_stream(self.eng.device).wait_event(self.pending[self.last])

    def _rows(self, t):
        if all(s == self.m for s in self.sizes):
            return t
        return self.torch.cat([t[r * self.m:r * self.m + s] for r, s in enumerate(self.sizes)], dim=0)

    def _flat(self, lo, hi):
        """Rows [lo, hi) of every rank's flat buffer segment (units: bytes per row), ranks in order."""
        self.wait()
        f = self.g_flat[self.last].view(self.world, -1)
        m = self.m
        return self.torch.cat([f[r, lo * m:hi * m].view(m, hi - lo)[:s] for r, s in enumerate(self.sizes)], dim=0)

    def obs(self, copy=False):
        """The last step's node-wide observations (see the class note on their lifetime)."""
        self.wait()
        o = self._rows(self.g_obs[self.last])
        return o.clone() if copy and o is self.g_obs[self.last] else o

    def rewards(self):
        R = self.R
        return self._flat(0, 8 * R).contiguous().view(self.torch.float64).view(-1, R)

    def done(self):
        return self._flat(8 * self.R, 8 * self.R + 1).view(-1)

    def truncated(self):
        return self._flat(8 * self.R + 1, 8 * self.R + 2).view(-1)

    def listed(self):
        """[N, A] uint8: agent a of env e was alive before the step (its reward and observation are valid)."""
        o = 8 * self.R + 2
        return self._flat(o, o + self.A)

    def was_reset(self):
        """[N] uint8: env e's observation is the one its autoreset produced this step."""
        o = 8 * self.R + 2 + self.A
        return self._flat(o, o + 1).view(-1)
