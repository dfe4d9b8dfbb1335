// The appearance model of the simulator's frames: per-vertex colours, a glTF 2.0 metallic-roughness material (Khronos glTF 2.0
// specification, appendix B) under an ambient term and up to 8 point lights, pasted over a background through the reference's
// grey-level mask.  Reference: src/HandSimulator/utils.py:225-230 (MetallicRoughnessMaterial: base colour factor 0.5, metallic 0.5,
// roughness 0.7), :286-313 (generate_train_lights, re-drawn for every frame), :264-284 (augment_background), :323 (ambient 0.1).
//
// The rule is the project's OWN -- pyrender's shader and its output encoding are not reproduced, parity unpinned, as the rasteriser's
// is; include/ev2hands_hip.h (ev2h_esim_shade) and tests/ref_shade.py (float64) state it.  This file runs after render.hip on the same
// chunk and reads what it left: face_id, depth and the per-vertex records of the render scratch.  It rasterises nothing: the edge
// functions of the ONE face a pixel holds are evaluated again, with the rasteriser's own expressions, to get the weights.
//
// One lane per pixel in the rasteriser's 16 x 16 tiles, so the lanes of a tile read the records of a few neighbouring faces (they
// stay in the vector cache; no LDS).  A frame's lights are indexed by blockIdx.y alone: scalar loads, uniform over the wave.  A wave
// without a covered lane only copies background.  No atomics; a pixel depends on its own frame only, so any split of a sequence into
// chunks gives the same bytes.
#include "common.hpp"
#include "ev2hands_hip.h"
#include "random.hpp"
#include "render_layout.hpp"
#include "shade_brdf.hpp"

#include <math.h>

namespace {

constexpr int SHD_MAX_LIGHTS = 8;
constexpr int SHD_DRAW_LIGHTS = 5;            // generate_train_lights
constexpr int SHD_MAX_FRAMES = 4096;          // esim.hip: ES_MAX_FRAMES, ES_MAX_PIXELS
constexpr int SHD_MAX_PIXELS = 1 << 22;

struct ShadeArgs {
    const int32_t* face_id;                   // [F][H][W]
    const float* depth;                       // [F][H][W] mm
    const float* scratch;                     // render.hip's, window stride scratch_stride floats
    size_t scratch_stride;
    const int32_t* faces;
    const uint8_t* colors;                    // [2 nv][3] RGB
    const float* lights;                      // [F or 1][L][6]
    size_t light_stride;                      // floats per frame, 0: one table for every frame
    const uint8_t* background;                // [H][W][3] or null
    uint8_t* rgb;                             // [F][H][W][3]
    int nfaces, nvt, width, height, n_lights, mask_rule;
    float f, cx, cy, factor, metallic, alpha2, kd;      // kd = 0.96 (1 - metallic)
    float ambient[3];
};

// generate_train_lights as a pure function of (seed, global frame): random.hpp, stream 5.  One lane per (frame, light).
__global__ __launch_bounds__(64) void shade_lights_kernel(uint64_t seed, const int64_t* __restrict__ frame_counter, int n_frames,
                                                          float* __restrict__ table) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_frames * SHD_DRAW_LIGHTS) return;
    const int fr = t / SHD_DRAW_LIGHTS, k = t % SHD_DRAW_LIGHTS;
    const uint32_t g = (uint32_t)((uint64_t)frame_counter[0] + (uint64_t)fr);
    const ev2h_random::u32x4 a = ev2h_random::window_block(seed, g, ev2h_random::STREAM_LIGHTS, 2u * (uint32_t)k);
    const float inten = (float)(1u + (a.v[0] >> 30));
    float x = k == 2 ? 1.f : 0.f, y = k == 0 ? -1.f : 1.f, z = k == 2 ? 2.f : 1.f;       // utils.py:293,297,301
    if (k >= 3) {                                                                         // utils.py:305,309
        const ev2h_random::u32x4 b = ev2h_random::window_block(seed, g, ev2h_random::STREAM_LIGHTS, 2u * (uint32_t)k + 1u);
        x = __fmul_rn(__fsub_rn(__fmul_rn(2.f, ev2h_random::unit_float(b.v[0])), 1.f), 2.f);
        y = __fmul_rn(__fsub_rn(__fmul_rn(2.f, ev2h_random::unit_float(b.v[1])), 1.f), 2.f);
        z = __fmul_rn(__fsub_rn(__fmul_rn(2.f, ev2h_random::unit_float(b.v[2])), 1.f), 2.f);
    }
    x = __fadd_rn(x, __fdiv_rn(ev2h_random::unit_float(a.v[1]), 10.f));
    y = __fadd_rn(y, __fdiv_rn(ev2h_random::unit_float(a.v[2]), 10.f));
    z = __fadd_rn(z, __fdiv_rn(ev2h_random::unit_float(a.v[3]), 10.f));
    float* o = table + (size_t)t * 6;
    o[0] = x; o[1] = -y; o[2] = -z;                                                       // utils.py:181-183: half a turn about x
    o[3] = inten; o[4] = inten; o[5] = inten;
}

using ev2h_shade::to_byte;

__global__ __launch_bounds__(RND_THREADS) void shade_kernel(ShadeArgs a, int tiles_x) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int c = tx * RND_TILE_W + (tid % RND_TILE_W), r = ty * RND_TILE_H + (tid / RND_TILE_W);
    const bool live = c < a.width && r < a.height;
    const size_t pix = ((size_t)b * a.height + (live ? r : 0)) * a.width + (live ? c : 0);
    int fid = live ? a.face_id[pix] : -1;
    int ia = 0, ib = 0, ic = 0;
    if (fid >= 0) {
        if (fid < a.nfaces) { ia = a.faces[3 * fid]; ib = a.faces[3 * fid + 1]; ic = a.faces[3 * fid + 2]; }
        if (fid >= a.nfaces || (unsigned)ia >= (unsigned)a.nvt || (unsigned)ib >= (unsigned)a.nvt || (unsigned)ic >= (unsigned)a.nvt)
            fid = -1;                                                            // not the rasteriser's output: background
    }
    const bool covered = fid >= 0;
    float val[3] = {0.f, 0.f, 0.f};
    if (__ballot(covered) != 0ull && covered) {
        const float* rec = a.scratch + (size_t)b * a.scratch_stride + RND_HEADER_FLOATS;
        const float4 A = *reinterpret_cast<const float4*>(rec + (size_t)ia * RND_RECORD_FLOATS);
        const float4 Bv = *reinterpret_cast<const float4*>(rec + (size_t)ib * RND_RECORD_FLOATS);
        const float4 Cv = *reinterpret_cast<const float4*>(rec + (size_t)ic * RND_RECORD_FLOATS);
        const float4 na = *reinterpret_cast<const float4*>(rec + (size_t)ia * RND_RECORD_FLOATS + 4);
        const float4 nb = *reinterpret_cast<const float4*>(rec + (size_t)ib * RND_RECORD_FLOATS + 4);
        const float4 nc = *reinterpret_cast<const float4*>(rec + (size_t)ic * RND_RECORD_FLOATS + 4);
        const float px = (float)c + 0.5f, py = (float)r + 0.5f;
        // render.hip's edge functions, relative to a vertex of the triangle
        const float e_ab = __fsub_rn(__fmul_rn(Bv.x - A.x, py - A.y), __fmul_rn(Bv.y - A.y, px - A.x));
        const float e_bc = __fsub_rn(__fmul_rn(Cv.x - Bv.x, py - Bv.y), __fmul_rn(Cv.y - Bv.y, px - Bv.x));
        const float e_ca = __fsub_rn(__fmul_rn(A.x - Cv.x, py - Cv.y), __fmul_rn(A.y - Cv.y, px - Cv.x));
        const float wa = e_bc * A.z, wb = e_ca * Bv.z, wc = e_ab * Cv.z;
        float nx = wa * na.x + wb * nb.x + wc * nc.x;
        float ny = wa * na.y + wb * nb.y + wc * nc.y;
        float nz = wa * na.z + wb * nb.z + wc * nc.z;
        // albedo
        const uint8_t* ca = a.colors + (size_t)ia * 3;
        const uint8_t* cb = a.colors + (size_t)ib * 3;
        const uint8_t* cc = a.colors + (size_t)ic * 3;
        const float wsum = wa + wb + wc;
        float base[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float col = wsum != 0.f ? (wa * (float)ca[k] + wb * (float)cb[k] + wc * (float)cc[k]) / wsum : (float)ca[k];
            base[k] = a.factor * col / 255.f;
            val[k] = base[k] * a.ambient[k];
        }
        const float l2 = nx * nx + ny * ny + nz * nz;
        if (l2 >= 1e-30f && a.n_lights > 0) {
            const float inv = 1.f / sqrtf(l2);
            nx *= inv; ny *= inv; nz *= inv;
            const float z = a.depth[pix] / 1000.f;
            const float Px = (px - a.cx) * z / a.f, Py = (py - a.cy) * z / a.f, Pz = z;
            const float* lt = a.lights + (size_t)b * a.light_stride;             // uniform over the workgroup
            ev2h_shade::add_lights(nx, ny, nz, Px, Py, Pz, base, a.metallic, a.alpha2, a.kd, lt, a.n_lights, val);
        }
    }
    if (!live) return;
    uint8_t o0 = 0, o1 = 0, o2 = 0;
    if (covered) { o0 = to_byte(val[0]); o1 = to_byte(val[1]); o2 = to_byte(val[2]); }
    if (a.background) {
        bool keep = covered;
        if (a.mask_rule) keep = ev2h_shade::grey_keeps(o0, o1, o2);                  // an uncovered pixel is black: grey 0
        if (!keep) {
            const uint8_t* g = a.background + ((size_t)r * a.width + c) * 3;
            o0 = g[0]; o1 = g[1]; o2 = g[2];
        }
    }
    uint8_t* o = a.rgb + pix * 3;
    o[0] = o0; o[1] = o1; o[2] = o2;
}

}  // namespace

extern "C" int ev2h_esim_shade(const int32_t* face_id, const float* depth, const void* render_scratch, size_t scratch_bytes,
                               const int32_t* faces, int nfaces, const uint8_t* vertex_colors, int n_frames, int nv, int width, int height,
                               float f, float cx, float cy, float base_color_factor, float metallic, float roughness, float ambient_r,
                               float ambient_g, float ambient_b, const float* lights, int n_lights, int lights_per_frame, uint64_t seed,
                               const int64_t* frame_counter, float* light_table, const uint8_t* background, int mask_rule, uint8_t* rgb,
                               ev2h_stream_t stream) {
    EV2H_CHECK_ARG(face_id && depth && render_scratch && faces && vertex_colors && rgb);
    EV2H_CHECK_ARG(lights || (frame_counter && light_table));
    EV2H_CHECK_ARG(n_frames >= 1 && n_frames <= SHD_MAX_FRAMES && width >= 1 && height >= 1 && width <= 4096 && height <= 4096);
    EV2H_CHECK_ARG((long long)width * height <= SHD_MAX_PIXELS);
    EV2H_CHECK_ARG(nv >= 1 && 2 * nv <= RND_MAX_VERTS && nfaces >= 1);
    EV2H_CHECK_ARG(lights ? (n_lights >= 0 && n_lights <= SHD_MAX_LIGHTS) : n_lights == SHD_DRAW_LIGHTS);
    EV2H_CHECK_ARG(lights_per_frame == 0 || lights_per_frame == 1);
    EV2H_CHECK_ARG(mask_rule == 0 || mask_rule == 1);
    EV2H_CHECK_ARG(f > 0.f && isfinite(f) && isfinite(cx) && isfinite(cy));
    EV2H_CHECK_ARG(base_color_factor >= 0.f && base_color_factor <= 1.f && metallic >= 0.f && metallic <= 1.f);
    EV2H_CHECK_ARG(roughness > 0.f && roughness <= 1.f);
    EV2H_CHECK_ARG(ambient_r >= 0.f && ambient_g >= 0.f && ambient_b >= 0.f && isfinite(ambient_r) && isfinite(ambient_g) && isfinite(ambient_b));
    EV2H_CHECK_ARG(((uintptr_t)render_scratch & 15) == 0);
    EV2H_CHECK_ARG(scratch_bytes == ev2h_render_scratch_bytes(n_frames, nv));
    ShadeArgs a{};
    a.face_id = face_id; a.depth = depth;
    a.scratch = static_cast<const float*>(render_scratch);
    a.scratch_stride = RND_HEADER_FLOATS + (size_t)2 * nv * RND_RECORD_FLOATS;
    a.faces = faces; a.colors = vertex_colors;
    a.background = background; a.rgb = rgb;
    a.nfaces = nfaces; a.nvt = 2 * nv; a.width = width; a.height = height; a.n_lights = n_lights; a.mask_rule = mask_rule;
    a.f = f; a.cx = cx; a.cy = cy; a.factor = base_color_factor; a.metallic = metallic;
    const float alpha = roughness * roughness;
    a.alpha2 = alpha * alpha;
    a.kd = 0.96f * (1.f - metallic);
    a.ambient[0] = ambient_r; a.ambient[1] = ambient_g; a.ambient[2] = ambient_b;
    if (lights) {
        a.lights = lights;
        a.light_stride = lights_per_frame ? (size_t)n_lights * 6 : 0;
    } else {
        shade_lights_kernel<<<ceil_div(n_frames * SHD_DRAW_LIGHTS, 64), 64, 0, (hipStream_t)stream>>>(seed, frame_counter, n_frames, light_table);
        EV2H_CHECK_LAUNCH();
        a.lights = light_table;
        a.light_stride = (size_t)SHD_DRAW_LIGHTS * 6;
    }
    const int tiles_x = ceil_div(width, RND_TILE_W), tiles_y = ceil_div(height, RND_TILE_H);
    shade_kernel<<<dim3(tiles_x * tiles_y, n_frames), RND_THREADS, 0, (hipStream_t)stream>>>(a, tiles_x);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
