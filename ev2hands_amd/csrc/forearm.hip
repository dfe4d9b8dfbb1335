// The forearm cylinders and the per-frame jitter of the simulator's frames.  Reference: src/HandSimulator/twohands.py:67-73 (5 mm of
// uniform jitter on `trans`, drawn again for every hand and frame, on the rendered mesh only) and :83-86 with manotosmplx.py:277-374
// (Forearms: the convex hull of two 18-gon rings of radius 0.0275 m around the wrist and 1.8 m further along `dir`).
//
// The rule is the project's OWN -- include/ev2hands_hip.h (ev2h_esim_forearms) and tests/ref_forearm.py (float64) state it.  The hull
// is not rasterised: the capped cylinder it approximates is intersected analytically with the ray of every pixel centre.  The
// intersection runs in float64 (a few dozen operations per pixel and cylinder): in float32 the discriminant of a 27.5 mm cylinder
// half a metre away loses the digits that decide the silhouette and the depth next to it.  The shading is float32 and is shade.hip's
// own, from shade_brdf.hpp.
//
// The pass runs after render.hip and after shade.hip (or esim.hip's compose) on the same chunk and overwrites, in place, the pixels a
// forearm owns: depth, face_id (-2 left, -3 right: negative, so esim.hip labels them 0) and rgb.  One lane per pixel in the
// rasteriser's 16 x 16 tiles; a frame's two records and its lights are indexed by blockIdx.y alone (scalar loads, uniform over the
// wave); a wave without a hit stops after the intersection.  No LDS, no atomics, nothing read back.
#include "common.hpp"
#include "ev2hands_hip.h"
#include "random.hpp"
#include "render_layout.hpp"
#include "shade_brdf.hpp"

#include <math.h>

namespace {

constexpr int FA_MAX_FRAMES = 4096;           // shade.hip: SHD_MAX_FRAMES, SHD_MAX_PIXELS
constexpr int FA_MAX_PIXELS = 1 << 22;
constexpr int FA_MAX_LIGHTS = 8;
constexpr int FA_REC = EV2H_FOREARM_RECORD;   // a[3] d[3] radius length colour[3] valid
constexpr int FA_JOINT_FLOATS = 21 * 3;

// ---- the jitter ---------------------------------------------------------------------------------------------------------------------
// One lane per (frame, hand, axis): lane k copies the columns k, k + 3, ... of its row; the three last columns (transl) get the draw.
__global__ __launch_bounds__(64) void jitter_rows_kernel(const float* __restrict__ rows_l, const float* __restrict__ rows_r, int n_frames,
                                                         int width, float amplitude_mm, uint64_t seed,
                                                         const int64_t* __restrict__ frame_counter, float* __restrict__ out_l,
                                                         float* __restrict__ out_r) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_frames * 6) return;
    const int fr = t / 6, h = (t % 6) / 3, k = t % 3;
    const float* src = (h ? rows_r : rows_l) + (size_t)fr * width;
    float* dst = (h ? out_r : out_l) + (size_t)fr * width;
    const uint32_t g = (uint32_t)((uint64_t)frame_counter[0] + (uint64_t)fr);
    const ev2h_random::u32x4 blk = ev2h_random::window_block(seed, g, ev2h_random::STREAM_JITTER, (uint32_t)h);
    for (int j = k; j < width; j += 3) {
        float v = src[j];
        if (j >= width - 3) {
            const float u = ev2h_random::unit_float(ev2h_random::block_word(blk, (uint32_t)(j - (width - 3))));
            v = __fadd_rn(v, __fdiv_rn(__fmul_rn(amplitude_mm, u), 1000.f));
        }
        dst[j] = v;
    }
}

// ---- the axes -----------------------------------------------------------------------------------------------------------------------
struct AxesArgs {
    float R[9], t[3], e[6];                   // row-major rotation, translation in METRES, the elbow offsets of left and right
    float radius, length, colour[6];
    int reference_rule;
};

// One lane per (frame, hand).
__global__ __launch_bounds__(64) void forearm_axes_kernel(const float* __restrict__ joints_l, const float* __restrict__ joints_r,
                                                          const uint8_t* __restrict__ present, int n_frames, AxesArgs a,
                                                          float* __restrict__ records) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_frames * 2) return;
    const int fr = t / 2, h = t % 2;
    const float* w = (h ? joints_r : joints_l) + (size_t)fr * FA_JOINT_FLOATS;      // joint 0: the wrist, metres
    const float wx = w[0], wy = w[1], wz = w[2];
    const float px = wx - a.t[0], py = wy - a.t[1], pz = wz - a.t[2];
    float s[3];                                                                   // R^T (root_c - t), then the rule
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float rw = a.R[i] * px + a.R[3 + i] * py + a.R[6 + i] * pz;
        s[i] = a.reference_rule ? rw + a.e[3 * h + i] : a.e[3 * h + i] - rw;
    }
    float v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = a.R[3 * i] * s[0] + a.R[3 * i + 1] * s[1] + a.R[3 * i + 2] * s[2];
    const float n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    const bool there = present ? present[t] != 0 : true;
    const bool valid = there && isfinite(wx) && isfinite(wy) && isfinite(wz) && n2 > 0.f && isfinite(n2);
    const float inv = valid ? 1.f / sqrtf(n2) : 0.f;
    float* o = records + (size_t)t * FA_REC;
    o[0] = wx; o[1] = wy; o[2] = wz;
    o[3] = valid ? v[0] * inv : 0.f; o[4] = valid ? v[1] * inv : 0.f; o[5] = valid ? v[2] * inv : 0.f;
    o[6] = a.radius; o[7] = a.length;
    o[8] = a.colour[3 * h]; o[9] = a.colour[3 * h + 1]; o[10] = a.colour[3 * h + 2];
    o[11] = valid ? 1.f : 0.f;
}

// ---- the pass -----------------------------------------------------------------------------------------------------------------------
struct ForearmArgs {
    const float* records;                     // [F][2][FA_REC]
    float* depth;                             // [F][H][W] mm
    int32_t* face_id;                         // [F][H][W]
    uint8_t* rgb;                             // [F][H][W][3]
    const float* lights;                      // [F or 1][L][6]
    size_t light_stride;
    const uint8_t* background;                // [H][W][3] or null
    int width, height, n_lights, mask_rule, lit;
    float f, cx, cy, znear, factor, metallic, alpha2, kd;
    float ambient[3];
};

struct Hit {
    float depth;                              // mm, 0: no hit
    float nx, ny, nz;                         // unit, outward
};

// the nearest point of one capped cylinder on the ray t * (qx, qy, 1), t in metres, with t * 1000 > znear; rec is uniform
__device__ __forceinline__ Hit cylinder_hit(const float* __restrict__ rec, double qx, double qy, double znear) {
    Hit out{0.f, 0.f, 0.f, 0.f};
    const double ax = rec[0], ay = rec[1], az = rec[2];
    double dx = rec[3], dy = rec[4], dz = rec[5];
    const double dl = sqrt(dx * dx + dy * dy + dz * dz);
    dx /= dl; dy /= dl; dz /= dl;
    const double rad = rec[6], len = rec[7];
    const double qd = qx * dx + qy * dy + dz, ad = ax * dx + ay * dy + az * dz;
    const double ux = qx - qd * dx, uy = qy - qd * dy, uz = 1.0 - qd * dz;      // the ray and the camera across the axis
    const double mx = ad * dx - ax, my = ad * dy - ay, mz = ad * dz - az;
    const double A = ux * ux + uy * uy + uz * uz, B = ux * mx + uy * my + uz * mz;
    const double hh = qx * (ay * dz - az * dy) + qy * (az * dx - ax * dz) + (ax * dy - ay * dx);     // q . (a x d)
    const double disc = A * (rad * rad) - hh * hh;
    double best = INFINITY, nx = 0.0, ny = 0.0, nz = 0.0;
    if (A > 0.0 && disc >= 0.0) {                                               // the side: both roots
        const double sq = sqrt(disc);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double t = (k ? -B + sq : -B - sq) / A;
            const double s = t * qd - ad;
            if (t * 1000.0 > znear && s >= 0.0 && s <= len && t < best) {
                best = t;
                nx = t * qx - ax - s * dx; ny = t * qy - ay - s * dy; nz = t - az - s * dz;
            }
        }
    }
    if (qd != 0.0) {                                                            // the caps: at the wrist (-d), at the far end (+d)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double off = k ? len : 0.0;
            const double t = (ad + off) / qd;
            const double wx = t * qx - ax - off * dx, wy = t * qy - ay - off * dy, wz = t - az - off * dz;
            if (t * 1000.0 > znear && wx * wx + wy * wy + wz * wz <= rad * rad && t < best) {
                best = t;
                nx = k ? dx : -dx; ny = k ? dy : -dy; nz = k ? dz : -dz;
            }
        }
    }
    if (best < INFINITY) {
        const double nl = sqrt(nx * nx + ny * ny + nz * nz);
        out.depth = (float)(best * 1000.0);
        if (nl > 0.0) { out.nx = (float)(nx / nl); out.ny = (float)(ny / nl); out.nz = (float)(nz / nl); }
    }
    return out;
}

__global__ __launch_bounds__(RND_THREADS) void forearm_kernel(ForearmArgs a, int tiles_x) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int c = tx * RND_TILE_W + (tid % RND_TILE_W), r = ty * RND_TILE_H + (tid / RND_TILE_W);
    const bool live = c < a.width && r < a.height;
    const size_t pix = ((size_t)b * a.height + (live ? r : 0)) * a.width + (live ? c : 0);
    const float* rec = a.records + (size_t)b * 2 * FA_REC;                      // uniform over the workgroup
    const bool valid_l = rec[FA_REC - 1] != 0.f, valid_r = rec[2 * FA_REC - 1] != 0.f;
    if (!valid_l && !valid_r) return;
    const float px = (float)c + 0.5f, py = (float)r + 0.5f;
    const double qx = ((double)px - (double)a.cx) / (double)a.f, qy = ((double)py - (double)a.cy) / (double)a.f;
    Hit hit{0.f, 0.f, 0.f, 0.f};
    bool right = false;
    if (valid_l) hit = cylinder_hit(rec, qx, qy, (double)a.znear);
    if (valid_r) {
        const Hit hr = cylinder_hit(rec + FA_REC, qx, qy, (double)a.znear);
        if (hr.depth > 0.f && (hit.depth == 0.f || hr.depth < hit.depth)) { hit = hr; right = true; }      // an equal depth keeps the left
    }
    bool own = false;
    if (live && hit.depth > 0.f) {
        const float hd = a.depth[pix];
        own = hd == 0.f || a.face_id[pix] < 0 || hit.depth < hd;                // an equal depth keeps the hand
    }
    if (__ballot(own) == 0ull || !own) return;
    const float* col = rec + (right ? FA_REC : 0) + 8;
    uint8_t o0, o1, o2;
    if (a.lit) {
        float base[3], val[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            base[k] = a.factor * col[k] / 255.f;
            val[k] = base[k] * a.ambient[k];
        }
        if (a.n_lights > 0) {
            const float z = hit.depth / 1000.f;
            const float Px = (px - a.cx) * z / a.f, Py = (py - a.cy) * z / a.f, Pz = z;
            const float* lt = a.lights + (size_t)b * a.light_stride;             // uniform over the workgroup
            ev2h_shade::add_lights(hit.nx, hit.ny, hit.nz, Px, Py, Pz, base, a.metallic, a.alpha2, a.kd, lt, a.n_lights, val);
        }
        o0 = ev2h_shade::to_byte(val[0]); o1 = ev2h_shade::to_byte(val[1]); o2 = ev2h_shade::to_byte(val[2]);
        if (a.background && a.mask_rule && !ev2h_shade::grey_keeps(o0, o1, o2)) {   // a dark forearm pixel shows the background
            const uint8_t* g = a.background + ((size_t)r * a.width + c) * 3;
            o0 = g[0]; o1 = g[1]; o2 = g[2];
        }
    } else {                                                                     // the demo's head-light, coloured as esim.hip's compose
        const float I = fminf(1.f, 0.3f + 0.7f * fabsf(hit.nz));
        const float s = (float)(int)(I * 255.f + 0.5f) / 255.0f;
        o0 = (uint8_t)(int)(s * col[0] + 0.5f); o1 = (uint8_t)(int)(s * col[1] + 0.5f); o2 = (uint8_t)(int)(s * col[2] + 0.5f);
    }
    a.depth[pix] = hit.depth;
    a.face_id[pix] = right ? EV2H_FOREARM_RIGHT : EV2H_FOREARM_LEFT;
    uint8_t* o = a.rgb + pix * 3;
    o[0] = o0; o[1] = o1; o[2] = o2;
}

bool finite3(const float* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!isfinite(v[i])) return false;
    return true;
}

}  // namespace

extern "C" int ev2h_esim_jitter_rows(const float* rows_left, const float* rows_right, int n_frames, int row_width, float amplitude_mm,
                                     uint64_t seed, const int64_t* frame_counter, float* out_left, float* out_right,
                                     ev2h_stream_t stream) {
    EV2H_CHECK_ARG(rows_left && rows_right && frame_counter && out_left && out_right);
    EV2H_CHECK_ARG(out_left != rows_left && out_right != rows_right && out_left != out_right);
    EV2H_CHECK_ARG(n_frames >= 1 && n_frames <= FA_MAX_FRAMES && row_width >= 3 && row_width <= 4096);
    EV2H_CHECK_ARG(amplitude_mm >= 0.f && isfinite(amplitude_mm));
    jitter_rows_kernel<<<ceil_div(n_frames * 6, 64), 64, 0, (hipStream_t)stream>>>(rows_left, rows_right, n_frames, row_width, amplitude_mm,
                                                                                   seed, frame_counter, out_left, out_right);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_esim_forearm_axes(const float* joints_left, const float* joints_right, const uint8_t* present, int n_frames,
                                      const float* rotation, const float* translation_mm, const float* elbow_offset, int reference_rule,
                                      float radius, float length, const uint8_t* colors, float* records, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(joints_left && joints_right && elbow_offset && colors && records);
    EV2H_CHECK_ARG(n_frames >= 1 && n_frames <= FA_MAX_FRAMES);
    EV2H_CHECK_ARG(reference_rule == 0 || reference_rule == 1);
    EV2H_CHECK_ARG(radius > 0.f && length > 0.f && isfinite(radius) && isfinite(length));
    EV2H_CHECK_ARG(finite3(elbow_offset, 6) && (!rotation || finite3(rotation, 9)) && (!translation_mm || finite3(translation_mm, 3)));
    AxesArgs a{};
    for (int i = 0; i < 9; ++i) a.R[i] = rotation ? rotation[i] : (i % 4 == 0 ? 1.f : 0.f);
    for (int i = 0; i < 3; ++i) a.t[i] = translation_mm ? translation_mm[i] / 1000.f : 0.f;
    for (int i = 0; i < 6; ++i) { a.e[i] = elbow_offset[i]; a.colour[i] = (float)colors[i]; }
    a.radius = radius; a.length = length; a.reference_rule = reference_rule;
    forearm_axes_kernel<<<ceil_div(n_frames * 2, 64), 64, 0, (hipStream_t)stream>>>(joints_left, joints_right, present, n_frames, a, records);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_esim_forearms(const float* records, int n_frames, int width, int height, float f, float cx, float cy, float znear,
                                  int lit, float base_color_factor, float metallic, float roughness, float ambient_r, float ambient_g,
                                  float ambient_b, const float* lights, int n_lights, int lights_per_frame, const uint8_t* background,
                                  int mask_rule, float* depth, int32_t* face_id, uint8_t* rgb, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(records && depth && face_id && rgb);
    EV2H_CHECK_ARG(n_frames >= 1 && n_frames <= FA_MAX_FRAMES && width >= 1 && height >= 1 && width <= 4096 && height <= 4096);
    EV2H_CHECK_ARG((long long)width * height <= FA_MAX_PIXELS);
    EV2H_CHECK_ARG(f > 0.f && isfinite(f) && isfinite(cx) && isfinite(cy) && znear >= 0.f && isfinite(znear));
    EV2H_CHECK_ARG(lit == 0 || lit == 1);
    EV2H_CHECK_ARG(mask_rule == 0 || mask_rule == 1);
    ForearmArgs a{};
    if (lit) {
        EV2H_CHECK_ARG(n_lights >= 0 && n_lights <= FA_MAX_LIGHTS && (lights || n_lights == 0));
        EV2H_CHECK_ARG(lights_per_frame == 0 || lights_per_frame == 1);
        EV2H_CHECK_ARG(base_color_factor >= 0.f && base_color_factor <= 1.f && metallic >= 0.f && metallic <= 1.f);
        EV2H_CHECK_ARG(roughness > 0.f && roughness <= 1.f);
        EV2H_CHECK_ARG(ambient_r >= 0.f && ambient_g >= 0.f && ambient_b >= 0.f && isfinite(ambient_r) && isfinite(ambient_g) && isfinite(ambient_b));
        a.lights = lights; a.n_lights = n_lights;
        a.light_stride = lights_per_frame ? (size_t)n_lights * 6 : 0;
        a.factor = base_color_factor; a.metallic = metallic;
        const float alpha = roughness * roughness;                               // ev2h_esim_shade's own expressions
        a.alpha2 = alpha * alpha;
        a.kd = 0.96f * (1.f - metallic);
        a.ambient[0] = ambient_r; a.ambient[1] = ambient_g; a.ambient[2] = ambient_b;
        a.background = background; a.mask_rule = mask_rule;
    }
    a.records = records; a.depth = depth; a.face_id = face_id; a.rgb = rgb;
    a.width = width; a.height = height; a.lit = lit;
    a.f = f; a.cx = cx; a.cy = cy; a.znear = znear;
    const int tiles_x = ceil_div(width, RND_TILE_W), tiles_y = ceil_div(height, RND_TILE_H);
    forearm_kernel<<<dim3(tiles_x * tiles_y, n_frames), RND_THREADS, 0, (hipStream_t)stream>>>(a, tiles_x);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
