"""The ways an episode can end, read off two consecutive canonical states (the dict of tests/golden records,
OracleEnv.state(), StateView.canonical()) and the step's done / truncated flags.  Shared by the fixture census
(test_golden_outcomes.py: what the reference's recorded runs contain) and the terminal-outcome table
(terminal_outcomes.py: what the oracle alone shows for every row before the GPU test compares the engine with it).

Outcomes of a step:

  ext_won, ext_lost       extermination ended without a minimum of zombies / with no player alive
  ext_min_won             extermination with minimum_zombies > 0 ended won: the last zombie died and no spawn cell
                          was free for the respawn
  ext_min_goes_on         ... every zombie of the previous state died, the respawn placed one, the episode goes on
  safe_won, safe_lost     safehouse ended with / without a player alive; safe_won_death: a player died on that step
  evac_won                evacuation ended with half the team alive and 4-connected; evac_won_bot_first: a bot is
                          alive (the walk starts from the first alive bot), evac_won_agents_only: a team without
                          bots, evac_won_dead_member: a member of the team is dead
  evac_lost               evacuation ended with fewer than half the team alive
  evac_apart              evacuation goes on with half the team alive; evac_apart_diag: two alive players of
                          different 4-connected groups touch diagonally
  surv_lost               survival ended (every player dead)
  agents_dead_bot_alive   not ended, truncated: no agent alive, a bot alive (end reward -10)
  done_and_timelimit      ended on the step the TimeLimit truncated
  single_won, single_lost the single-agent surface (ZS_REWARD_SINGLE) ended won / lost
  late_zombie, late_player, late_off
                          the step's decisive thing sat in an entity slot >= G (info["G"]): the only zombie left
                          while the episode goes on, the only player alive, the only alive player off the
                          objectives (safehouse, not ended)
"""

from libzombsole_amd import _abi

LIFE = 2  # [x, y, life, weapon]

RULE_NAMES = {_abi.RULES_EXTERMINATION: "extermination", _abi.RULES_SURVIVAL: "survival",
              _abi.RULES_EVACUATION: "evacuation", _abi.RULES_SAFEHOUSE: "safehouse"}


def info_for(builder, G=0):
    """What classify() needs to know of a config (an _abi.ConfigBuilder); G: the lanes per env, for the late_*
    outcomes (0: none)."""
    c = builder.cfg
    return {"rule": RULE_NAMES[int(c.rules)], "surface": "multi" if c.reward_mode == _abi.REWARD_MULTI else "single",
            "min_z": int(c.minimum_zombies), "objectives": {tuple(p) for p in builder.map.objectives}, "G": G}


def groups(cells):
    """The 4-connected groups of a list of (x, y): a list of sets."""
    left, out = set(cells), []
    while left:
        todo = [left.pop()]
        g = set(todo)
        while todo:
            x, y = todo.pop()
            for q in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
                if q in left:
                    left.discard(q)
                    g.add(q)
                    todo.append(q)
        out.append(g)
    return out


def diagonal_contact(gs):
    for i, g in enumerate(gs):
        for h in gs[i + 1:]:
            for (x, y) in g:
                if any((x + dx, y + dy) in h for dx in (-1, 1) for dy in (-1, 1)):
                    return True
    return False


def classify(info, prev, cur, done, trunc):
    """The set of outcomes of the step that led from state `prev` to `cur`."""
    out = set()
    rule, G = info["rule"], info.get("G", 0)
    agents, bots = cur["agents"], cur["players"]
    team = bots + agents  # Game.get_all_players(): the bots first
    slots = list(range(len(agents), len(agents) + len(bots))) + list(range(len(agents)))
    alive = [p for p in team if p[LIFE] > 0]
    alive_slots = [s for s, p in zip(slots, team) if p[LIFE] > 0]
    bot_alive = any(p[LIFE] > 0 for p in bots)
    agent_alive = any(p[LIFE] > 0 for p in agents)
    before = prev["players"] + prev["agents"]
    died_now = any(q[LIFE] > 0 and p[LIFE] <= 0 for q, p in zip(before, team))
    nz = sum(1 for d in cur["dyn"] if d[0] == 5)
    nz_prev = sum(1 for d in prev["dyn"] if d[0] == 5)
    half = 2 * len(alive) >= len(team)
    won = half if rule == "evacuation" else bool(alive)
    if done and trunc:
        out.add("done_and_timelimit")
    if not done and trunc and not agent_alive and bot_alive:
        out.add("agents_dead_bot_alive")
    if done and info["surface"] == "single":
        out.add("single_won" if won else "single_lost")
    if G and len(alive_slots) == 1 and alive_slots[0] >= G:
        out.add("late_player")
    if G and not done and nz == 1 and len(team) >= G and rule == "extermination":
        out.add("late_zombie")
    if rule == "extermination":
        if done and not alive:
            out.add("ext_lost")
        elif done:
            out.add("ext_min_won" if info["min_z"] > 0 else "ext_won")
        elif info["min_z"] > 0 and nz_prev > 0 and nz > 0 and cur["ctr"][2] - prev["ctr"][2] == nz_prev:
            out.add("ext_min_goes_on")
    elif rule == "safehouse":
        if done:
            out.add("safe_won" if alive else "safe_lost")
            if alive and died_now:
                out.add("safe_won_death")
        else:
            off = [s for s, p in zip(slots, team) if p[LIFE] > 0 and (p[0], p[1]) not in info["objectives"]]
            if G and len(off) == 1 and off[0] >= G:
                out.add("late_off")
    elif rule == "evacuation":
        if done and half:
            out.add("evac_won")
            out.add("evac_won_bot_first" if bot_alive else "evac_won_agent_first")
            if not bots:
                out.add("evac_won_agents_only")
            if len(alive) < len(team):
                out.add("evac_won_dead_member")
        elif done:
            out.add("evac_lost")
        elif half:
            out.add("evac_apart")
            if diagonal_contact(groups([(p[0], p[1]) for p in alive])):
                out.add("evac_apart_diag")
    elif rule == "survival":
        if done:
            out.add("surv_lost")
    return out
