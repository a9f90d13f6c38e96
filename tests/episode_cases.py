"""The table of the episode-statistics tests (ZS_FLAG_EPISODE_STATS): nine configs of terminal_outcomes.CONFIGS (by
import: every way an episode can end), each run both fused (k_step) and unfused (k_tick) because the launch sequences
differ, at 13, 37, 67 and 300 envs (k_episode_stats runs one lane per env in 256-thread workgroups: 300 is two
workgroups, the last one partial), 24 steps.

trace(row, steps) is the reference: the oracle alone (OracleEnv per env: rewards, done, truncated, states) run through
episode_model.EnvModel, computed once per (row, steps) and shared by the tests, which leave it unchanged.
test_episode_stats_plan.py shows on the CPU that the rows meet every outcome code; test_episode_stats.py compares the
engine with the trace on the GPU."""
import functools

import episode_model as EM
import outcomes as O
import step_instantiations as S
import terminal_outcomes as TO

CONFIGS = ("evac_tiny", "evac_bot", "evac_crowd", "surv_melee", "multi_troll", "single_troll", "single_duel", "ext_min",
           "safe_crowd")
ENVS = (13, 37, 67, 300)
LANES = {13: 64, 37: 8, 67: 1, 300: 16}  # lanes per env of a row, by its env count
STEPS = 24
KERNELS = ("k_step", "k_tick6")
# rows whose first seed is moved so that every outcome code shows in three envs or more between the rows
SEED0 = {}


class Row(S.Row):
    def __init__(self, config, ci, kernel):
        self.config, self.kernel = config, kernel
        self.n = ENVS[ci % len(ENVS)]
        self.G = LANES[self.n]
        self.make, self.stream, self.respawn, extra, _ = TO.CONFIGS[config]
        launch, self.step_kernel, self.tick_waves = S.KERNEL_LAUNCH[kernel]
        self.launch = dict(launch, fobs=-1, **extra)
        self.fused = kernel == "k_step"
        self.id = "%s-%s@%d" % (config, self.step_kernel, self.n)
        self.seed0 = SEED0.get(config, 41000 + 1000 * ci)

    def builder(self, n=None, par_exec=1, **flags):
        """The engine's config: the row's lanes per env and overrides, episode_stats on; flags: env_params,
        autoreset (False: ZS_FLAG_AUTORESET off)."""
        from libzombsole_amd import _abi
        b = S.Row.builder(self, n, par_exec)
        b.cfg.flags |= _abi.FLAG_EPISODE_STATS
        if flags.get("env_params"):
            b.cfg.flags |= _abi.FLAG_ENV_PARAMS
        if flags.get("autoreset") is False:
            b.cfg.flags &= ~_abi.FLAG_AUTORESET
        return b

    def plain_builder(self):
        """The same config without the flag."""
        return S.Row.builder(self)

    def info(self):
        return O.info_for(self.make(1))

    @property
    def R(self):
        c = self.make(1).cfg
        return c.num_agents if self.info()["surface"] == "multi" else 1

    def triple(self):
        c = self.make(1).cfg
        return (int(c.initial_zombies), int(c.minimum_zombies), int(c.max_episode_steps))


ROWS = [Row(cfg, ci, k) for ci, cfg in enumerate(CONFIGS) for k in KERNELS]
BY_ID = {r.id: r for r in ROWS}
MULTI_STEP = ("evac_tiny", "single_duel")  # TimeLimit 6 and 8: envs end twice within one 16-step launch


class Track(object):
    """One env: its oracle and its model, stepped with autoreset as the engine's envs are."""

    def __init__(self, row, seed, autoreset=True):
        from oracle.oracle import OracleEnv
        self.row, self.seed, self.autoreset = row, seed, autoreset
        self.o = OracleEnv(row.make(1))
        self.o.seed(seed)
        self.m = EM.EnvModel(row.R, int(row.make(1).cfg.rules))
        self.info = row.info()
        self.need, self.terminal, self.classes = False, None, set()
        self.reset()

    def reset(self):
        self.o.reset()
        self.m.reset()
        self.need = False
        self.prev = self.o.state()

    def step(self, t, actions=None):
        """Step t of the row's action stream (or `actions`); returns (done, trunc, was_reset)."""
        self.terminal = None
        if self.need and self.autoreset:
            self.reset()
            return False, False, True
        a = self.row.actions([self.seed], t, self.o.A)[0] if actions is None else actions
        _, rew, d, tr, _ = self.o.step(a)
        cur = self.o.state()
        closed = self.m.closed
        self.m.step(rew, d, tr, cur, self.row.triple())
        if (d or tr) and not closed:
            self.terminal = (EM.outcome_code(self.m.rules, cur, d, tr), O.classify(self.info, self.prev, cur, d, tr))
        self.prev = cur
        self.need = d or tr
        return d, tr, False


@functools.lru_cache(maxsize=None)
def trace(row_id, steps=STEPS):
    """The reference of a row: [snapshot after the reset, after step 1, ...] (episode_model.snapshot), and the list of
    (env, step, code, outcomes.classify's set) of every terminal step.  Shared: callers do not modify it."""
    row = BY_ID[row_id]
    tracks = [Track(row, s) for s in row.seeds()]
    snaps, ends = [EM.snapshot([k.m for k in tracks])], []
    for t in range(1, steps + 1):
        for e, k in enumerate(tracks):
            k.step(t)
            if k.terminal:
                ends.append((e, t) + k.terminal)
        snaps.append(EM.snapshot([k.m for k in tracks]))
    return snaps, ends
