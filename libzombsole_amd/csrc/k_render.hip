// k_render.hip — the picture of a ZS_FLAG_RENDER handle's envs (the rules: zs_render.hpp).  k_render_track is the last
// launch of a flagged handle's step: it keeps body_col, the colour of every cell's last body, from the step's death
// log (zs_reset clears the rows of the envs it resets through the same kernel).  k_render draws frames, uint8
// [10 H][10 W][3] each, pixel-exact to the map area of the reference's OpencvRenderer.
//
// k_render: one 256-thread workgroup per (frame, band of cell rows).  The band's cell codes (shape << 4 | colour), with
// the row above and a zero column to the left, are built in LDS: the decoration from the static cell word, the env's
// obstacle-present and body bitmaps and body_col, then the env's entities scattered over it.  A band's pixel rows are
// one contiguous byte range of the frame, so the lanes stream it as 16-B stores between a head and a tail of byte
// stores, whatever the alignment of the caller's buffer.  No atomics; nothing but the frame is written.
#include "zs_launch.hpp"
#include "zs_render.hpp"

// the band's codes and the atlas in LDS
struct LdsCodes {
    const lu8* codes;
    int stride, y_first;  // y_first: the cell row of code row 0 (the band's first row - 1)
    __device__ __forceinline__ int operator()(int x, int y) const { return codes[(y - y_first) * stride + x + 1]; }
};
struct LdsAtlas {
    const lu32* w;  // RenderAtlas's words
    __device__ __forceinline__ bool bit(int shape, int ox, int oy) const {
        return ZS_RENDER_BIT(w + (shape - 1) * ZS_RENDER_MASK_WORDS, ox, oy);
    }
    __device__ __forceinline__ uint32_t rgb(int i) const { return w[(RS_NSHAPE - 1) * ZS_RENDER_MASK_WORDS + i]; }
};

// the frame's bytes [o, o + n), n <= 16, o + n within the band: byte k of the result is frame byte o + k
struct Px16 {
    uint32_t w[4];
};
__device__ __forceinline__ Px16 render_bytes(const LdsCodes& code, const LdsAtlas& at, uint32_t o, int n, uint32_t row_bytes,
                                             int frame_w) {
    Px16 r = {{0u, 0u, 0u, 0u}};
    int py = (int)(o / row_bytes);
    const uint32_t bx = o - (uint32_t)py * row_bytes;
    int px = (int)(bx / 3u), ch = (int)(bx - 3u * (uint32_t)px);
    uint32_t rgb = render_pixel(code, at, px, py);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if (k < n) r.w[k >> 2] |= ((rgb >> (8 * ch)) & 0xffu) << (8 * (k & 3));
        if (++ch == 3 && k + 1 < n) {
            ch = 0;
            if (++px == frame_w) px = 0, py++;
            rgb = render_pixel(code, at, px, py);
        }
    }
    return r;
}

__global__ void __launch_bounds__(ZS_RENDER_BLOCK) k_render(RenderArgs a, const int32_t* envs, uint8_t* out, int n_frames) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    lu32* atlas = (lu32*)(ZS_LDS uint8_t*)lds_raw;
    lu8* codes = (lu8*)(ZS_LDS uint8_t*)lds_raw + ZS_RENDER_LDS_ATLAS;
    const int tid = threadIdx.x;
    const int k = blockIdx.x / a.plan.bands, band = blockIdx.x - k * a.plan.bands;
    if (k >= n_frames) return;  // a frame the caller's buffer has no room for
    const int env = envs ? envs[k] : k;
    if (env < 0 || env >= a.N) return;  // not an env: the frame keeps its bytes
    const int W = a.W, H = a.H, stride = render_code_stride(W);
    const int r0 = band * a.plan.rows, r1 = min(H, r0 + a.plan.rows), nr = r1 - r0 + 1;  // code rows: r0 - 1 .. r1 - 1

    if (tid == 0) {
#pragma unroll
        for (int s = 0; s < RS_NSHAPE - 1; s++)
#pragma unroll
            for (int w = 0; w < ZS_RENDER_MASK_WORDS; w++) atlas[s * ZS_RENDER_MASK_WORDS + w] = a.atlas.mask[s][w];
#pragma unroll
        for (int i = 0; i < ZS_RENDER_PALETTE; i++) atlas[(RS_NSHAPE - 1) * ZS_RENDER_MASK_WORDS + i] = a.atlas.rgb[i];
    }
    // 1) the decoration and the obstacles
    const uint32_t* opres = a.obst_present + (size_t)env * a.OW;
    const uint32_t* dead = a.dead + (size_t)env * a.DW;
    const uint8_t* body = a.body_col + (size_t)env * a.plan.body_bytes;
    for (int i = tid; i < nr * stride; i += ZS_RENDER_BLOCK) {
        const int j = i / stride, x = i - j * stride - 1, y = r0 - 1 + j;
        uint8_t c = 0;
        if (x >= 0 && y >= 0) {
            const int cell = y * W + x;
            const uint32_t sc = (uint32_t)a.scell[cell];
            const int oi = (int)(sc & SC_OBST_MASK) - 1;
            const int obstacle = oi >= 0 && oi < a.O && ((opres[oi >> 5] >> (oi & 31)) & 1u) ? (int)((sc >> SC_KIND_SHIFT) & 7u) : 0;
            const bool d = (dead[cell >> 5] >> (cell & 31)) & 1u;
            c = render_cell_code(obstacle, d, d ? body[cell] : 0, (sc & SC_OBJ_BIT) != 0);
        }
        codes[i] = c;
    }
    __syncthreads();
    // 2) the entities over it
    for (int s = tid; s < a.E; s += ZS_RENDER_BLOCK) {
        if (!a.present[(size_t)env * a.E + s]) continue;
        const int32_t p = a.pos[(size_t)env * a.E + s];
        const int x = unpack_x(p), y = unpack_y(p);
        if (x < 0 || x >= W || y < r0 - 1 || y >= r1 || y < 0) continue;
        codes[(y - (r0 - 1)) * stride + x + 1] = render_entity_code(a.slot_col[s]);
    }
    __syncthreads();
    // 3) the band's bytes: a head up to the first 16-B boundary, 16-B stores, a tail
    const LdsCodes code = {codes, stride, r0 - 1};
    const LdsAtlas at = {atlas};
    const uint32_t row_bytes = 3u * (uint32_t)a.plan.frame_w;
    const uint32_t b0 = (uint32_t)r0 * ZS_RENDER_CELL * row_bytes, b1 = (uint32_t)r1 * ZS_RENDER_CELL * row_bytes;
    uint8_t* dst = out + (size_t)k * (size_t)a.plan.frame_bytes;
    const uint32_t head = min((uint32_t)((0 - (uintptr_t)(dst + b0)) & 15u), b1 - b0);
    const uint32_t nchunk = (b1 - b0 - head) >> 4, t0 = b0 + head + (nchunk << 4);
    if (tid < 32) {  // lanes 0..15: the head's bytes, 16..31: the tail's
        const uint32_t o = tid < 16 ? b0 + tid : t0 + (tid - 16);
        const uint32_t end = tid < 16 ? b0 + head : b1;
        if (o < end) dst[o] = (uint8_t)render_bytes(code, at, o, 1, row_bytes, a.plan.frame_w).w[0];
    }
    for (uint32_t c = tid; c < nchunk; c += ZS_RENDER_BLOCK) {
        const uint32_t o = b0 + head + (c << 4);
        const Px16 v = render_bytes(code, at, o, 16, row_bytes, a.plan.frame_w);
        *(uint4*)(dst + o) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    }
}

// mode 0, the step's tracker: flags = the step's reset flags (never null); a reset env's row is cleared, every other
// env's death log is applied.  mode 1, zs_reset: the rows of the envs whose flag is nonzero (null: all) are cleared.
__global__ void __launch_bounds__(ZS_RENDER_BLOCK) k_render_track(RenderArgs a, const uint8_t* flags, int mode) {
    const int e = blockIdx.x * ZS_RENDER_BLOCK + threadIdx.x;
    const bool in = e < a.N;
    const bool clear = in && (flags ? flags[e] != 0 : true);
    const int lane = threadIdx.x & 63, e_wave = e - lane;
    const int nq = a.plan.body_bytes >> 4;  // a row is a multiple of 16 bytes, 16-B aligned
    unsigned long long m = __ballot(clear);
    while (m) {  // the wave clears its envs' rows together, one env at a time
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1;
        uint4* row = (uint4*)(a.body_col + (size_t)(e_wave + b) * a.plan.body_bytes);
        for (int q = lane; q < nq; q += 64) row[q] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (!in || clear || mode) return;
    const int n = max(0, min(a.dlog_n[e], a.E));
    render_track_env(a.body_col + (size_t)e * a.plan.body_bytes, a.W, a.H, a.dlog + (size_t)e * a.E * 5, n, a.E, a.slot_col);
}

hipError_t launch_render_track(hipStream_t s, const RenderArgs& a, const uint8_t* flags, int mode) {
    hipLaunchKernelGGL(k_render_track, dim3(zs_render_track_grid(a.N)), dim3(ZS_RENDER_BLOCK), 0, s, a, flags, mode);
    return hipGetLastError();
}

// frames k < min(n, n_frames) of envs[k] (null: env k) into out + k * frame_bytes
hipError_t launch_render(hipStream_t s, const RenderArgs& a, const int32_t* envs, int n, uint8_t* out, int n_frames) {
    const long frames = n < n_frames ? n : n_frames;
    if (frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_render, dim3((unsigned)(frames * a.plan.bands)), dim3(ZS_RENDER_BLOCK), (size_t)a.plan.lds, s, a, envs, out,
                       n_frames);
    return hipGetLastError();
}
