// zs_episode.hpp — per-env episode statistics (ZS_FLAG_EPISODE_STATS): the update rule, written once.
//
// Per env (R = 1 on the single surface, A on the multi surface):
//   running        run_ret f64 [R], run_flags i32 (bit 0: closed)           -- the env's own, travels in snapshot records
//   last episode   last_ret f64 [R], last i32 [8] = {length, outcome, zombie_deaths, deaths, initial_zombies,
//                  minimum_zombies, max_episode_steps, serial}; serial = tot[0] after the episode is counted
//   totals         tot u32 [8] = {episodes, won, lost, truncated_agents_dead, truncated_timelimit, sum length,
//                  sum zombie_deaths, sum deaths} (sums mod 2^32), sum_ret f64 [R]
//
// The rule, per env and step, in this order:
//   1. the step was the env's reset:      run_ret = 0, closed = 0;
//   2. else, if not closed:               run_ret[r] = run_ret[r] + rewards[r]   (one float64 add, in step order);
//   3. if additionally done | truncated:  last_ret = run_ret, last filled, tot bumped, sum_ret[r] += run_ret[r],
//                                         closed = 1;
//   4. a closed env is neither accumulated nor counted again until its next reset (without ZS_FLAG_AUTORESET an
//      ended env keeps ticking and keeps reporting done).
//
// episode_update() is the rule over a store S, which says where the data lives: the kernel's store reads and writes
// the engine's [k][N] columns (k_episode.hip), a host program's plain vectors (tests/episode_plan_host.cpp).  A store
// provides, for the env it stands for:
//   double rew(int r)                 the step's reward r
//   double run(int r), void set_run(int r, double v)
//   int32_t flags(), void set_flags(int32_t v)
//   void set_last_ret(int r, double v), void add_sum_ret(int r, double v)
//   void set_last(int k, int32_t v)
//   uint32_t tot(int k), void set_tot(int k, uint32_t v)
//   EpisodeEnd end()                  what a terminal step leaves in the env's world (read only when it ended)
// Nothing here needs HIP.
#pragma once
#include <stdint.h>

#include "zs_obs_plan.hpp"  // ZS_HD, the public header (ZS_RULES_*)

#define ZS_EP_CLOSED 1  // run_flags bit 0: the episode ended, the env has not been reset since

#define ZS_EP_LAST 8  // words of `last`
#define ZS_EP_TOT 8   // words of `tot`
enum { EP_LAST_LENGTH = 0, EP_LAST_OUTCOME, EP_LAST_ZD, EP_LAST_DEATHS, EP_LAST_INITIAL, EP_LAST_MINIMUM, EP_LAST_MAXSTEPS, EP_LAST_SERIAL };
enum { EP_TOT_EPISODES = 0, EP_TOT_WON, EP_TOT_LOST, EP_TOT_AGENTS_DEAD, EP_TOT_TIMELIMIT, EP_TOT_LENGTH, EP_TOT_ZD, EP_TOT_DEATHS };

// outcome codes (last[EP_LAST_OUTCOME]); ZS_EP_DONE_AND_TIMELIMIT is OR-ed in when done and truncated are both set
#define ZS_EP_WON 1           // done and won
#define ZS_EP_LOST 2          // done and not won
#define ZS_EP_AGENTS_DEAD 3   // not done, truncated, no agent alive (the -10 truncation)
#define ZS_EP_TIMELIMIT 4     // not done, truncated, some agent alive
#define ZS_EP_DONE_AND_TIMELIMIT 256

// a terminal step's world: the scalar rows, the players (slots [0, A + P)) and agents (slots [0, A)) with life > 0,
// and the triple of the episode that ended
struct EpisodeEnd {
    int32_t length, zombie_deaths, deaths;  // S_EPSTEPS, S_ZD, S_DEATHS
    int32_t alive_players, alive_agents;
    int32_t initial_zombies, minimum_zombies, max_episode_steps;
};

// rules_check's `won` (zs_tick.hpp): half the team alive for evacuation, else any player alive
ZS_HD inline bool episode_won(int rules, int alive_players, int n_players) {
    return rules == ZS_RULES_EVACUATION ? 2 * alive_players >= n_players : alive_players > 0;
}

ZS_HD inline int32_t episode_outcome(bool done, bool trunc, bool won, bool agent_alive) {
    const int32_t code = done ? (won ? ZS_EP_WON : ZS_EP_LOST) : (agent_alive ? ZS_EP_TIMELIMIT : ZS_EP_AGENTS_DEAD);
    return code | (done && trunc ? ZS_EP_DONE_AND_TIMELIMIT : 0);
}

// the totals' counter an outcome code bumps
ZS_HD inline int episode_tot_slot(int32_t outcome) { return EP_TOT_WON + (outcome & 255) - ZS_EP_WON; }

template <class S>
ZS_HD inline void episode_update(S& s, int R, int rules, int n_players, bool was_reset, bool done, bool trunc) {
    if (was_reset) {
        for (int r = 0; r < R; r++) s.set_run(r, 0.0);
        s.set_flags(0);
        return;
    }
    const int32_t flags = s.flags();
    if (flags & ZS_EP_CLOSED) return;
    const bool ended = done || trunc;
    for (int r = 0; r < R; r++) {
        const double v = s.run(r) + s.rew(r);
        s.set_run(r, v);
        if (ended) {
            s.set_last_ret(r, v);
            s.add_sum_ret(r, v);
        }
    }
    if (!ended) return;
    const EpisodeEnd w = s.end();
    const int32_t outcome = episode_outcome(done, trunc, episode_won(rules, w.alive_players, n_players), w.alive_agents > 0);
    const uint32_t serial = s.tot(EP_TOT_EPISODES) + 1u;
    s.set_tot(EP_TOT_EPISODES, serial);
    const int slot = episode_tot_slot(outcome);
    s.set_tot(slot, s.tot(slot) + 1u);
    s.set_tot(EP_TOT_LENGTH, s.tot(EP_TOT_LENGTH) + (uint32_t)w.length);
    s.set_tot(EP_TOT_ZD, s.tot(EP_TOT_ZD) + (uint32_t)w.zombie_deaths);
    s.set_tot(EP_TOT_DEATHS, s.tot(EP_TOT_DEATHS) + (uint32_t)w.deaths);
    s.set_last(EP_LAST_LENGTH, w.length);
    s.set_last(EP_LAST_OUTCOME, outcome);
    s.set_last(EP_LAST_ZD, w.zombie_deaths);
    s.set_last(EP_LAST_DEATHS, w.deaths);
    s.set_last(EP_LAST_INITIAL, w.initial_zombies);
    s.set_last(EP_LAST_MINIMUM, w.minimum_zombies);
    s.set_last(EP_LAST_MAXSTEPS, w.max_episode_steps);
    s.set_last(EP_LAST_SERIAL, (int32_t)serial);
    s.set_flags(flags | ZS_EP_CLOSED);
}

// The engine's running part, [ZS_EP_RUN_COLS(R)][N] dword columns in one allocation, so that a snapshot record takes
// it as one column section (zs_snapshot.hpp ep_run): column 0 stays zero (the record's alignment gap, when it has
// one), then run_ret[r] as its low and high dwords, run_flags, and a column that stays zero (the record's 4 zero bytes).
#define ZS_EP_RUN_COLS(R) (2 * (R) + 3)
#define ZS_EP_COL_RET(r) (1 + 2 * (r))
#define ZS_EP_COL_FLAGS(R) (1 + 2 * (R))
