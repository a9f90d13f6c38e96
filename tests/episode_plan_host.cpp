// Host program of tests/test_episode_stats_plan.py: the episode-statistics update rule (libzombsole_amd/csrc/
// zs_episode.hpp) over a store of plain vectors, and the snapshot record's ep_run section (zs_snapshot.hpp,
// zs_record.hpp), compiled with the host compiler.  One JSON line per input line:
//   "E R rules n_players"   a new env of R reward slots -> {"ok": true}
//   "S reset done trunc length zd deaths alive_players alive_agents initial minimum max_steps rew..."
//                           one step through episode_update(); the R rewards are C99 hex floats
//                           -> {"run": [...], "last_ret": [...], "sum_ret": [...], "last": [...], "tot": [...], "closed": c}
//   "C"                     the last episode and the totals zeroed (what k_episode_clear does) -> the same row
//   "L E O DW OW A envp R"  snapshot_layout(E, O, DW, OW, A, envp, R) -> every section's offset, "env_params", "ep_run",
//                           "ep_bytes", "ep_gap", "pad", "rec_bytes"
//   "W E O DW OW A envp R N" the record walker over the flagged table: every env packed and unpacked; the bytes at
//                           ep_run must be the env's run_ret, run_flags and 4 zero bytes, the gap zero
//                           -> {"ok": true, "nsec": n, "rec_bytes": b}
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "zs_episode.hpp"
#include "zs_record.hpp"
#include "zs_snapshot.hpp"

static const char* names[SNAP_NSEC] = {"ring", "dead", "obst_hp", "obst_present", "obst_nonpos", "pos", "life", "serial", "scal",
                                       "hp_dirty", "dead_dirty", "rngst", "prev_life", "weapon", "present", "order", "listed"};

struct HostStore {
    std::vector<double> run_, last_ret_, sum_ret_, rew_;
    int32_t flags_ = 0, last_[ZS_EP_LAST] = {0};
    uint32_t tot_[ZS_EP_TOT] = {0};
    EpisodeEnd end_{};
    double rew(int r) const { return rew_[r]; }
    double run(int r) const { return run_[r]; }
    void set_run(int r, double v) { run_[r] = v; }
    int32_t flags() const { return flags_; }
    void set_flags(int32_t v) { flags_ = v; }
    void set_last_ret(int r, double v) { last_ret_[r] = v; }
    void add_sum_ret(int r, double v) { sum_ret_[r] = sum_ret_[r] + v; }
    void set_last(int k, int32_t v) { last_[k] = v; }
    uint32_t tot(int k) const { return tot_[k]; }
    void set_tot(int k, uint32_t v) { tot_[k] = v; }
    EpisodeEnd end() const { return end_; }
};

static void print_doubles(const char* name, const std::vector<double>& v) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? ", " : "", v[i]);
    printf("], ");
}

static void print_store(const HostStore& s) {
    printf("{");
    print_doubles("run", s.run_);
    print_doubles("last_ret", s.last_ret_);
    print_doubles("sum_ret", s.sum_ret_);
    printf("\"last\": [");
    for (int k = 0; k < ZS_EP_LAST; k++) printf("%s%d", k ? ", " : "", s.last_[k]);
    printf("], \"tot\": [");
    for (int k = 0; k < ZS_EP_TOT; k++) printf("%s%u", k ? ", " : "", s.tot_[k]);
    printf("], \"closed\": %d}\n", s.flags_ & ZS_EP_CLOSED);
}

static std::string walk(int E, int O, int DW, int OW, int A, int envp, int R, int N, int* nsec, int* rec_bytes) {
    const size_t words[SNAP_NSEC] = {(size_t)ZS_SNAP_RING * N, (size_t)DW * N, (size_t)O * N, (size_t)OW * N, (size_t)OW * N,
                                     (size_t)E * N, (size_t)E * N, (size_t)E * N, (size_t)ZS_SNAP_NSCAL * N, (size_t)N,
                                     (size_t)N, (size_t)N, (size_t)A * N,
                                     ((size_t)E * N + 3) / 4, ((size_t)E * N + 3) / 4, ((size_t)E * N + 3) / 4, ((size_t)A * N + 3) / 4};
    std::vector<std::vector<uint32_t>> src(SNAP_NSEC), dst(SNAP_NSEC);
    void *sb[SNAP_NSEC], *db[SNAP_NSEC];
    for (int s = 0; s < SNAP_NSEC; s++) {
        src[s].assign(words[s] + 4, 0u), dst[s].assign(words[s] + 4, 0u);
        for (size_t k = 0; k < words[s]; k++) src[s][k] = (uint32_t)(s + 1) * 0x9E3779B1u ^ (uint32_t)(k + 1) * 0x85EBCA77u;
        sb[s] = src[s].data(), db[s] = dst[s].data();
    }
    std::vector<uint32_t> ep((size_t)ZS_EP_RUN_COLS(R) * N, 0u), ep2(ep.size(), 0u), envs((size_t)ZS_SNAP_ENVP * N + 4, 7u),
        envd(envs.size(), 0u);
    for (int c = 1; c <= 2 * R + 1; c++)  // the zero columns stay zero
        for (int e = 0; e < N; e++) ep[(size_t)c * N + e] = 0xA0000000u + (uint32_t)c * 1000u + (uint32_t)e;
    const RecTable T = snapshot_rec_table(sb, E, O, DW, OW, A, (size_t)N, envp ? envs.data() : nullptr, ep.data(), R);
    const RecTable D = snapshot_rec_table(db, E, O, DW, OW, A, (size_t)N, envp ? envd.data() : nullptr, ep2.data(), R);
    const RecTable U = snapshot_rec_table(sb, E, O, DW, OW, A, (size_t)N, envp ? envs.data() : nullptr);
    const SnapshotLayout L = snapshot_layout(E, O, DW, OW, A, envp != 0, R), L0 = snapshot_layout(E, O, DW, OW, A, envp != 0);
    *nsec = T.nsec, *rec_bytes = T.rec_bytes;
    if (T.rec_bytes != L.rec_bytes) return "table and layout differ in rec_bytes";
    std::vector<uint32_t> rec((size_t)T.rec_bytes / 4 + 4, 0xCCCCCCCCu), rec0((size_t)U.rec_bytes / 4 + 4, 0xCCCCCCCCu);
    uint8_t *r = (uint8_t*)rec.data(), *r0 = (uint8_t*)rec0.data();
    while ((uintptr_t)r & 15) r++;
    while ((uintptr_t)r0 & 15) r0++;
    for (int e = 0; e < N; e++) {
        for (int c = 0; c < T.rec_bytes / 16; c++) rec_copy_chunk<true>(T, (RecChunk*)r, (size_t)e, c);
        for (int c = 0; c < U.rec_bytes / 16; c++) rec_copy_chunk<true>(U, (RecChunk*)r0, (size_t)e, c);
        for (int k = 0; k < 2 * R + 2; k++) {
            uint32_t v;
            memcpy(&v, r + L.ep_run + 4 * k, 4);
            if (v != ep[(size_t)(k + 1) * N + e]) return "ep_run dword " + std::to_string(k) + " of env " + std::to_string(e);
        }
        const int head = L.ep_run - L.ep_gap;  // where the unflagged record's byte rows start
        if (head != L0.off[SNAP_NWORD]) return "ep_run is not right behind the 4-byte sections";
        if (memcmp(r, r0, head) != 0) return "the sections before ep_run differ from the unflagged record";
        for (int b = head; b < L.ep_run; b++)
            if (r[b]) return "the alignment gap is not zero";
        if (memcmp(r + L.ep_run + L.ep_bytes, r0 + head, L0.off[SNAP_NSEC] - head) != 0)
            return "the byte rows differ from the unflagged record";
        for (int b = L.off[SNAP_NSEC]; b < T.rec_bytes; b++)
            if (r[b]) return "padding is not zero";
        for (int c = 0; c < D.rec_bytes / 16; c++) rec_copy_chunk<false>(D, (RecChunk*)r, (size_t)e, c);
    }
    if (ep2 != ep) return "unpack: ep_run differs";
    if (envp && memcmp(envd.data(), envs.data(), (size_t)4 * ZS_SNAP_ENVP * N) != 0) return "unpack: env_params differs";
    for (int s = 0; s < SNAP_NSEC; s++)
        if (memcmp(dst[s].data(), src[s].data(), (s < SNAP_NWORD ? 4 : 1) * (s < SNAP_NWORD ? words[s] : (s == SNAP_LISTED ? (size_t)A * N : (size_t)E * N))) != 0)
            return std::string("unpack: ") + names[s] + " differs";
    return "";
}

int main(void) {
    char kind;
    HostStore st;
    int R = 0, rules = 0, n_players = 0;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'E') {
            if (scanf("%d %d %d", &R, &rules, &n_players) != 3 || R < 1) return 1;
            st = HostStore();
            st.run_.assign(R, 0.0), st.last_ret_.assign(R, 0.0), st.sum_ret_.assign(R, 0.0), st.rew_.assign(R, 0.0);
            printf("{\"ok\": true}\n");
        } else if (kind == 'S') {
            int reset, done, trunc;
            EpisodeEnd& w = st.end_;
            if (scanf("%d %d %d %d %d %d %d %d %d %d %d", &reset, &done, &trunc, &w.length, &w.zombie_deaths, &w.deaths,
                      &w.alive_players, &w.alive_agents, &w.initial_zombies, &w.minimum_zombies, &w.max_episode_steps) != 11)
                return 1;
            for (int r = 0; r < R; r++) {
                char buf[64];
                if (scanf("%63s", buf) != 1) return 1;
                st.rew_[r] = strtod(buf, nullptr);
            }
            episode_update(st, R, rules, n_players, reset != 0, done != 0, trunc != 0);
            print_store(st);
        } else if (kind == 'C') {
            for (int r = 0; r < R; r++) st.last_ret_[r] = st.sum_ret_[r] = 0.0;
            memset(st.last_, 0, sizeof(st.last_));
            memset(st.tot_, 0, sizeof(st.tot_));
            print_store(st);
        } else if (kind == 'L' || kind == 'W') {
            int E, O, DW, OW, A, envp, ep, N = 0;
            if (scanf("%d %d %d %d %d %d %d", &E, &O, &DW, &OW, &A, &envp, &ep) != 7) return 1;
            if (kind == 'W' && scanf("%d", &N) != 1) return 1;
            if (kind == 'L') {
                const SnapshotLayout L = snapshot_layout(E, O, DW, OW, A, envp != 0, ep);
                printf("{");
                for (int s = 0; s < SNAP_NSEC; s++) printf("\"%s\": %d, ", names[s], L.off[s]);
                printf("\"env_params\": %d, \"ep_run\": %d, \"ep_bytes\": %d, \"ep_gap\": %d, \"pad\": %d, \"rec_bytes\": %d}\n", L.envp,
                       L.ep_run, L.ep_bytes, L.ep_gap, L.off[SNAP_NSEC], L.rec_bytes);
            } else {
                int nsec = 0, rec_bytes = 0;
                const std::string err = walk(E, O, DW, OW, A, envp, ep, N, &nsec, &rec_bytes);
                if (err.empty()) printf("{\"ok\": true, \"nsec\": %d, \"rec_bytes\": %d}\n", nsec, rec_bytes);
                else printf("{\"ok\": false, \"error\": \"%s\"}\n", err.c_str());
            }
        } else {
            return 1;
        }
    }
    return 0;
}
