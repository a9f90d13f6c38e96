// zs_render.hpp — the rules of a ZS_FLAG_RENDER handle's picture, written once for k_render.hip and for a host
// compiler (tests/render_plan_host.cpp): the frame's geometry and the launch plan, the sprite atlas, the per-cell rule,
// the per-pixel rule and the body-colour tracker's rule.  Nothing here needs HIP.
//
// The frame is the map area of the reference's OpencvRenderer.render (renderer.py:235-277): uint8 [10 H][10 W][3], RGB.
// Every drawn cell paints a one-colour ZS_RENDER_MASK x ZS_RENDER_MASK mask at (10 x, 10 y); the reference paints the
// cells with x as the outer loop and y as the inner one, so on the border row or column two neighbouring masks share,
// the later cell wins, and a pixel's colour comes from at most four cells.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "zs_step_plan.hpp"  // ZS_HD

#define ZS_RENDER_CELL 10   // pixels per cell, both ways (build_renderer's cellwidth / cellheight)
#define ZS_RENDER_MASK 11   // a sprite's mask: the cell and the first pixel row and column of its neighbours
#define ZS_RENDER_PALETTE 8 // palette entries (RGB)
#define ZS_RENDER_MASK_WORDS 4  // 121 bits, bit oy * 11 + ox

// sprite shapes: a cell's code is shape << 4 | palette index, 0 = nothing drawn
enum { RS_NONE = 0, RS_SOLID, RS_BOX, RS_DISC, RS_FRAME, RS_BODY, RS_NSHAPE };
// the default palette's entries; a body colour of 0 ("none recorded") is drawn green, which is the zombies' own
enum { RC_GREEN = 0, RC_BLUE, RC_CYAN, RC_YELLOW, RC_WHITE, RC_RED };

struct RenderAtlas {
    uint32_t mask[RS_NSHAPE - 1][ZS_RENDER_MASK_WORDS];  // solid, box, disc, frame, body
    uint32_t rgb[ZS_RENDER_PALETTE];                     // r | g << 8 | b << 16
};

// ---------------------------------------------------------------------------
// the default atlas: the project's own rasteriser of the five shapes on the 11 x 11 grid
// ---------------------------------------------------------------------------
inline bool render_disc_px(int x, int y) {
    if (x < 0 || y < 0 || x > 10 || y > 10) return false;
    return (x - 5) * (x - 5) + (y - 5) * (y - 5) <= 30;  // radius 5.5 around the cell's centre pixel
}
inline bool render_shape_px(int shape, int x, int y) {
    const bool frame = x < 2 || x > 8 || y < 2 || y > 8, diag = x == y || x + y == 10;
    switch (shape) {
        case RS_SOLID: return true;
        case RS_FRAME: return frame;
        case RS_BOX: return frame || diag;
        case RS_DISC: return render_disc_px(x, y);
        case RS_BODY:  // the disc's outline (its pixels with a 4-neighbour outside it) and both diagonals
            return diag || (render_disc_px(x, y) && !(render_disc_px(x - 1, y) && render_disc_px(x + 1, y) &&
                                                      render_disc_px(x, y - 1) && render_disc_px(x, y + 1)));
    }
    return false;
}
inline RenderAtlas render_default_atlas() {
    RenderAtlas a = {};
    for (int s = RS_SOLID; s < RS_NSHAPE; s++)
        for (int y = 0; y < ZS_RENDER_MASK; y++)
            for (int x = 0; x < ZS_RENDER_MASK; x++)
                if (render_shape_px(s, x, y)) a.mask[s - 1][(y * ZS_RENDER_MASK + x) >> 5] |= 1u << ((y * ZS_RENDER_MASK + x) & 31);
    // the CSS values of green, blue, cyan, yellow, white, red
    const uint32_t rgb[6] = {0x008000u, 0xff0000u, 0xffff00u, 0x00ffffu, 0xffffffu, 0x0000ffu};
    for (int i = 0; i < 6; i++) a.rgb[i] = rgb[i];
    return a;
}

// ---------------------------------------------------------------------------
// the launch plan: one workgroup per (frame, band of cell rows)
// ---------------------------------------------------------------------------
#define ZS_RENDER_BLOCK 256
#define ZS_RENDER_BAND_BYTES (64 * 1024)  // a band's pixel bytes, about: enough 16-B stores per lane to hide the setup

struct RenderPlan {
    int rows;        // cell rows per band
    int bands;       // bands per frame
    int lds;         // bytes of a workgroup's LDS image: the atlas, then the band's cell codes
    int frame_h, frame_w, frame_bytes;
    int body_bytes;  // body_col bytes per env: W * H rounded up to 16
};
#define ZS_RENDER_LDS_ATLAS ((int)sizeof(RenderAtlas))
// the code rows of a band: the row above it, then its own; each row has one zero cell ahead of column 0
ZS_HD inline int render_code_stride(int W) { return W + 1; }

ZS_HD inline RenderPlan render_plan(int W, int H) {
    RenderPlan p;
    const int row_bytes = 3 * ZS_RENDER_CELL * ZS_RENDER_CELL * W;  // the pixel bytes of one cell row
    int rows = (ZS_RENDER_BAND_BYTES + row_bytes - 1) / row_bytes;
    rows = rows < 1 ? 1 : rows > H ? H : rows;
    p.rows = rows;
    p.bands = (H + rows - 1) / rows;
    p.lds = ZS_RENDER_LDS_ATLAS + ((render_code_stride(W) * (rows + 1) + 15) & ~15);
    p.frame_h = ZS_RENDER_CELL * H, p.frame_w = ZS_RENDER_CELL * W;
    p.frame_bytes = 3 * p.frame_h * p.frame_w;
    p.body_bytes = (W * H + 15) & ~15;
    return p;
}

// ---------------------------------------------------------------------------
// the per-cell rule: what the reference's `world.things.get(p) or world.decoration.get(p)` draws
// ---------------------------------------------------------------------------
// obstacle: the cell's present obstacle kind (ZS_THING_WALL / ZS_THING_BOX, whatever its life) or 0; dead: the cell's
// body bit; body_col: its recorded colour; objective: the cell is an objective.  An entity on the cell replaces the
// code with render_entity_code.
ZS_HD inline uint8_t render_cell_code(int obstacle, bool dead, int body_col, bool objective) {
    if (obstacle) return obstacle == ZS_THING_BOX ? (RS_BOX << 4 | RC_YELLOW) : (RS_SOLID << 4 | RC_WHITE);
    if (dead) return (uint8_t)(RS_BODY << 4 | (body_col & (ZS_RENDER_PALETTE - 1)));  // a body replaces an objective
    if (objective) return RS_FRAME << 4 | RC_BLUE;
    return 0;
}
ZS_HD inline uint8_t render_entity_code(int slot_col) { return (uint8_t)(RS_DISC << 4 | (slot_col & (ZS_RENDER_PALETTE - 1))); }

// the colour of a slot's thing, and of the body it leaves: agents blue, zombies green, bots by type (players/*.py)
inline uint8_t render_slot_col(int slot, int A, int P, const int32_t* bot_types) {
    if (slot < A) return RC_BLUE;
    if (slot >= A + P) return RC_GREEN;
    switch (bot_types[slot - A]) {
        case ZS_BOT_TERMINATOR: return RC_CYAN;
        case ZS_BOT_SNIPER: return RC_YELLOW;
        case ZS_BOT_HAMSTER: return RC_WHITE;
        case ZS_BOT_RANDOMAN: return RC_RED;
        default: return RC_BLUE;  // the troll
    }
}

// ---------------------------------------------------------------------------
// the per-pixel rule.  code(x, y): the cell's code, 0 for x < 0 or y < 0 (the caller never asks beyond W - 1, H - 1).
// Candidates in priority order: the pixel's own cell; the cell above on a cell's first pixel row; the cell to the
// left on its first pixel column; the cell above-left on both.  The first whose mask has the pixel's bit colours it.
// at.bit(shape, ox, oy): bit oy * 11 + ox of the shape's mask; at.rgb(i): palette entry i.
// ---------------------------------------------------------------------------
#define ZS_RENDER_BIT(words, ox, oy) (((words)[((oy) * ZS_RENDER_MASK + (ox)) >> 5] >> (((oy) * ZS_RENDER_MASK + (ox)) & 31)) & 1u)

template <typename Code, typename Atlas>
ZS_HD inline uint32_t render_pixel(const Code& code, const Atlas& at, int px, int py) {
    const int x0 = px / ZS_RENDER_CELL, y0 = py / ZS_RENDER_CELL;
    const int ox = px - ZS_RENDER_CELL * x0, oy = py - ZS_RENDER_CELL * y0;
    const int n = 1 + (oy == 0) + (ox == 0) + (oy == 0 && ox == 0);
    for (int k = 0; k < n; k++) {
        // k = 0 own; then up (oy == 0), left (ox == 0), up-left (both), skipping the ones that do not apply
        const int which = k == 0 ? 0 : (oy == 0 && ox == 0) ? k : oy == 0 ? 1 : 2;
        const int dx = which >> 1, dy = which & 1;  // 0: own, 1: up, 2: left, 3: up-left
        const int c = code(x0 - dx, y0 - dy);
        if (c >> 4 && at.bit(c >> 4, ox + ZS_RENDER_CELL * dx, oy + ZS_RENDER_CELL * dy))
            return at.rgb(c & (ZS_RENDER_PALETTE - 1));
    }
    return 0u;
}

// ---------------------------------------------------------------------------
// the tracker's rule (k_render_track): env e's body_col row after a step.  was_reset: the step rebuilt the env (its
// death log is empty); else every entry {slot, serial, x, y, life} of the step's death log, in removal order, writes
// its slot's colour at its cell, so the last body of a cell gives the colour, as World.decoration keeps the last.
// ---------------------------------------------------------------------------
ZS_HD inline void render_track_env(uint8_t* row, int W, int H, const int32_t* dlog, int n, int E, const uint8_t* slot_col) {
    for (int i = 0; i < n; i++) {
        const int32_t* en = dlog + 5 * i;
        const int s = en[0], x = en[2], y = en[3];
        if (s < 0 || s >= E || x < 0 || y < 0 || x >= W || y >= H) continue;
        row[y * W + x] = slot_col[s];
    }
}
