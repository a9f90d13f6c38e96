// render_plan_host.cpp — csrc/zs_render.hpp on the host (tests/test_render_plan.py builds this with AddressSanitizer and
// UBSan and reads its JSON): the default atlas, the launch plans of a list of map sizes, the per-pixel rule over one
// crowded world, and the tracker's rule over a death log with entries to skip.
#include <cstdio>
#include <vector>

#include "zs_render.hpp"

struct HostAtlas {
    const RenderAtlas& a;
    bool bit(int shape, int ox, int oy) const { return ZS_RENDER_BIT(a.mask[shape - 1], ox, oy); }
    uint32_t rgb(int i) const { return a.rgb[i]; }
};
struct HostCodes {
    const std::vector<uint8_t>& c;
    int W;
    int operator()(int x, int y) const { return x < 0 || y < 0 ? 0 : c[(size_t)y * W + x]; }
};

int main() {
    const RenderAtlas at = render_default_atlas();
    printf("{\"masks\": [");
    for (int s = 0; s < RS_NSHAPE - 1; s++)
        printf("%s[%u, %u, %u, %u]", s ? ", " : "", at.mask[s][0], at.mask[s][1], at.mask[s][2], at.mask[s][3]);
    printf("], \"rgb\": [");
    for (int i = 0; i < ZS_RENDER_PALETTE; i++) printf("%s%u", i ? ", " : "", at.rgb[i]);
    printf("], \"plans\": [");
    const int sizes[][2] = {{9, 7}, {8, 5}, {1, 70}, {70, 1}, {5, 4}, {64, 64}, {16000, 1}, {1, 16000}, {218, 3}, {219, 3}, {4096, 1700}};
    bool first = true;
    for (const auto& wh : sizes) {
        const RenderPlan p = render_plan(wh[0], wh[1]);
        printf("%s[%d, %d, %d, %d, %d, %d]", first ? "" : ", ", wh[0], wh[1], p.rows, p.bands, p.lds, p.body_bytes);
        first = false;
    }
    // a 5 x 4 world: things side by side in every direction, in the first and last row and column
    const int W = 5, H = 4;
    const int32_t bots[1] = {ZS_BOT_SNIPER};
    const int ents[][3] = {{0, 0, 0}, {1, 0, 1}, {1, 1, 2}, {4, 3, 3}, {3, 2, 4}};          // x, y, slot (A = 1, P = 1)
    const int obst[][3] = {{2, 0, ZS_THING_WALL}, {2, 1, ZS_THING_BOX}, {0, 3, ZS_THING_WALL}, {4, 0, ZS_THING_BOX}};
    const int bodies[][3] = {{0, 1, RC_BLUE}, {1, 2, RC_GREEN}, {3, 3, RC_YELLOW}, {1, 0, RC_RED}};  // the last under an entity
    const int objs[][2] = {{0, 2}, {1, 2}, {4, 2}, {2, 0}};  // one under a body, one under a wall
    std::vector<uint8_t> code((size_t)W * H, 0);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int ob = 0, col = 0;
            bool dead = false, obj = false;
            for (const auto& o : obst) if (o[0] == x && o[1] == y) ob = o[2];
            for (const auto& b : bodies) if (b[0] == x && b[1] == y) dead = true, col = b[2];
            for (const auto& o : objs) if (o[0] == x && o[1] == y) obj = true;
            code[(size_t)y * W + x] = render_cell_code(ob, dead, col, obj);
        }
    printf("], \"world\": {\"W\": %d, \"H\": %d, \"entities\": [", W, H);
    for (size_t i = 0; i < sizeof(ents) / sizeof(ents[0]); i++) {
        const int col = render_slot_col(ents[i][2], 1, 1, bots);
        code[(size_t)ents[i][1] * W + ents[i][0]] = render_entity_code(col);
        printf("%s[%d, %d, %d]", i ? ", " : "", ents[i][0], ents[i][1], col);
    }
    printf("], \"obstacles\": [");
    for (size_t i = 0; i < 4; i++) printf("%s[%d, %d, %d]", i ? ", " : "", obst[i][0], obst[i][1], obst[i][2]);
    printf("], \"bodies\": [");
    for (size_t i = 0; i < 4; i++) printf("%s[%d, %d, %d]", i ? ", " : "", bodies[i][0], bodies[i][1], bodies[i][2]);
    printf("], \"objectives\": [");
    for (size_t i = 0; i < 4; i++) printf("%s[%d, %d]", i ? ", " : "", objs[i][0], objs[i][1]);
    printf("], \"frame\": [");
    const HostAtlas ha = {at};
    const HostCodes hc = {code, W};
    for (int py = 0; py < ZS_RENDER_CELL * H; py++)
        for (int px = 0; px < ZS_RENDER_CELL * W; px++) printf("%s%u", py || px ? ", " : "", render_pixel(hc, ha, px, py));
    // the tracker: slot colours {blue, yellow, green, green}; two deaths on cell (2, 1), the later one counts; entries
    // with a slot or a cell out of range are skipped
    const uint8_t slot_col[4] = {RC_BLUE, RC_YELLOW, RC_GREEN, RC_GREEN};
    const int32_t dlog[][5] = {{2, 7, 2, 1, 0}, {1, 1, 2, 1, -3}, {0, 0, 4, 3, 0}, {9, 0, 0, 0, 0}, {0, 0, 5, 0, 0},
                               {0, 0, 0, -1, 0}, {3, 2, 0, 0, 0}};
    std::vector<uint8_t> row((size_t)W * H, 0);
    row[3] = RC_RED;  // an earlier step's body stays
    render_track_env(row.data(), W, H, &dlog[0][0], 7, 4, slot_col);
    printf("], \"track_expected\": [");
    std::vector<int> exp((size_t)W * H, 0);
    exp[3] = RC_RED, exp[1 * W + 2] = RC_YELLOW, exp[3 * W + 4] = RC_BLUE, exp[0] = RC_GREEN;
    for (int i = 0; i < W * H; i++) printf("%s%d", i ? ", " : "", exp[i]);
    printf("]}, \"track\": [");
    for (int i = 0; i < W * H; i++) printf("%s%d", i ? ", " : "", (int)row[i]);
    printf("]}\n");
    return 0;
}
