// The demo's three panels on the GPU: event pixels coloured by polarity share, the same pixels coloured by predicted class,
// and the two predicted hand meshes rendered through the data set's camera, composed into one [B][H][3W][3] BGR frame.
// Reference: src/Ev2Hands/demo.py:35,53-62 (seg_mask), :120-145 (pyrender render + np.hstack),
// dataset/ev2hands_r.py:148-156 (event_frame, coordinates), settings.py:42 (MAIN_CAMERA).
//
// Panels 1 and 2 restate the reference's Python loops bit for bit (one float32 rounding per operation, conversion by
// truncation; every byte a point writes depends on that point's pixel record or is 255, so plain byte stores from many threads
// give the loop's result whatever their order).  Panel 3 is this project's OWN renderer -- pyrender's shader is not
// reproduced, parity unpinned; tests/ref_render.py is its float64 statement: pinhole f = (H/2)/tan(15 deg) looking down +z,
// sample at the pixel centre, inside = three edge functions of one sign or zero, 1/z linear in the image, nearest depth then
// lowest face index, smooth area-weighted vertex normals, I = min(1, 0.3 + 0.7 |n_z|).
//
// Why tiles and not a depth atomic: a 64-bit atomicMin of (depth, face) per covered sample would need a cleared depth image, a
// second pass to shade, and float atomics' traffic on 90 000 pixels x the depth complexity; with one workgroup per 16x16 tile
// every pixel is owned by one thread, the winner is kept in registers, and the image is written once.  Nearest-depth-then-
// lowest-index does not depend on the order the faces are visited in, so the image does not depend on tile shape or batch size.
#include "common.hpp"
#include "ev2hands_hip.h"
#include "render_layout.hpp"

namespace {

struct RenderArgs {
    const float* verts[2];                               // [B][nv][3] metres, window stride vstride[h] floats
    size_t vstride[2];
    const int32_t* faces;                                // [nfaces][3] into the concatenated 2 nv vertices
    const int32_t* vf_offsets;                           // [2 nv + 1] CSR: incident faces of every vertex, ascending
    const int32_t* vf_faces;
    int nv, nfaces, vf_len;
    int width, height;
    float f, cx, cy, znear;
    float* scratch;
    size_t scratch_stride;                               // floats per window
    uint8_t* frame;                                      // [B][height][frame_width][3]
    int frame_width, render_x0, clear_x0, clear_width;   // pixel columns: where panel 3 goes, which columns are zero-filled
    float* depth;                                        // [B][height][width] or null
    int32_t* face_id;
};

__device__ __forceinline__ void load_vertex(const RenderArgs& a, int b, int i, float& x, float& y, float& z) {
    const int h = i >= a.nv ? 1 : 0;
    const float* p = a.verts[h] + (size_t)b * a.vstride[h] + (size_t)(i - h * a.nv) * 3;
    x = p[0]; y = p[1]; z = p[2];
}

// One workgroup per window: project the 2 nv vertices, gather their normals in fixed (ascending face) order -- no float atomics,
// results independent of scheduling -- and reduce the screen bounding box of the vertices in front of znear.
__global__ __launch_bounds__(RND_THREADS) void render_setup_kernel(RenderArgs a) {
    __shared__ float s_box[4][RND_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nvt = 2 * a.nv;
    float* win = a.scratch + (size_t)b * a.scratch_stride;
    float* rec = win + RND_HEADER_FLOATS;
    float x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
    for (int i = tid; i < nvt; i += RND_THREADS) {
        float x, y, z;
        load_vertex(a, b, i, x, y, z);
        const float zmm = __fmul_rn(z, 1000.f);
        const bool front = zmm > a.znear;
        float u = 0.f, v = 0.f, w = 0.f;
        if (front) {
            u = __fadd_rn(__fmul_rn(a.f, __fdiv_rn(x, z)), a.cx);
            v = __fadd_rn(__fmul_rn(a.f, __fdiv_rn(y, z)), a.cy);
            w = __fdiv_rn(1.f, zmm);
            x0 = fminf(x0, u); x1 = fmaxf(x1, u);
            y0 = fminf(y0, v); y1 = fmaxf(y1, v);
        }
        float nx = 0.f, ny = 0.f, nz = 0.f;
        const int q0 = a.vf_offsets[i], q1 = a.vf_offsets[i + 1];
        if (q0 >= 0 && q1 <= a.vf_len) {
            for (int q = q0; q < q1; ++q) {
                const int k = a.vf_faces[q];
                if ((unsigned)k >= (unsigned)a.nfaces) continue;
                const int ia = a.faces[3 * k], ib = a.faces[3 * k + 1], ic = a.faces[3 * k + 2];
                if ((unsigned)ia >= (unsigned)nvt || (unsigned)ib >= (unsigned)nvt || (unsigned)ic >= (unsigned)nvt) continue;
                float ax, ay, az, bx, by, bz, cx, cy, cz;
                load_vertex(a, b, ia, ax, ay, az);
                load_vertex(a, b, ib, bx, by, bz);
                load_vertex(a, b, ic, cx, cy, cz);
                const float e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
                nx += e1y * e2z - e1z * e2y;
                ny += e1z * e2x - e1x * e2z;
                nz += e1x * e2y - e1y * e2x;
            }
        }
        const float l2 = nx * nx + ny * ny + nz * nz;
        if (l2 >= 1e-30f) {
            const float inv = 1.f / sqrtf(l2);
            nx *= inv; ny *= inv; nz *= inv;
        } else {
            nx = ny = nz = 0.f;
        }
        float4* o = reinterpret_cast<float4*>(rec + (size_t)i * RND_RECORD_FLOATS);
        o[0] = make_float4(u, v, w, 0.f);
        o[1] = make_float4(nx, ny, nz, 0.f);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        x0 = fminf(x0, __shfl_xor(x0, o, 64)); y0 = fminf(y0, __shfl_xor(y0, o, 64));
        x1 = fmaxf(x1, __shfl_xor(x1, o, 64)); y1 = fmaxf(y1, __shfl_xor(y1, o, 64));
    }
    if ((tid & 63) == 0) { s_box[0][tid >> 6] = x0; s_box[1][tid >> 6] = y0; s_box[2][tid >> 6] = x1; s_box[3][tid >> 6] = y1; }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < RND_THREADS / 64; ++wv) {
            x0 = fminf(x0, s_box[0][wv]); y0 = fminf(y0, s_box[1][wv]);
            x1 = fmaxf(x1, s_box[2][wv]); y1 = fmaxf(y1, s_box[3][wv]);
        }
        reinterpret_cast<float4*>(win)[0] = make_float4(x0, y0, x1, y1);      // +inf / -inf: nothing in front of the camera
        reinterpret_cast<float4*>(win)[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

__device__ __forceinline__ void store_bgr(uint8_t* p, uint8_t b, uint8_t g, uint8_t r) { p[0] = b; p[1] = g; p[2] = r; }

// One workgroup per (tile, window), one pixel per thread.  The workgroup owns every byte of its pixels' frame rows: it zero-fills
// the point panels' columns and writes panel 3 straight into the frame (and depth / face id when asked).
__global__ __launch_bounds__(RND_THREADS) void render_raster_kernel(RenderArgs a, int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float4* s_vert = reinterpret_cast<float4*>(smem_raw);                       // [2 nv] (u, v, w, -)
    __shared__ int4 s_list[RND_THREADS];                                        // kept faces of a batch: (ia, ib, ic, face)
    __shared__ int s_wave_cnt[RND_THREADS / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int c = tx * RND_TILE_W + (tid % RND_TILE_W), r = ty * RND_TILE_H + (tid / RND_TILE_W);
    const bool live = c < a.width && r < a.height;
    const int nvt = 2 * a.nv;
    const float* win = a.scratch + (size_t)b * a.scratch_stride;
    const float* rec = win + RND_HEADER_FLOATS;
    uint8_t* row = a.frame + ((size_t)b * a.height + (live ? r : 0)) * (size_t)a.frame_width * 3;

    if (live) {                                                                  // the point panels' background
        for (int x = a.clear_x0 + c; x < a.clear_x0 + a.clear_width; x += a.width) store_bgr(row + (size_t)x * 3, 0, 0, 0);
    }

    // tile against the window's bounding box: pixel centres of the tile span [tx0 + 0.5, tx1 - 0.5]
    const float4 box = reinterpret_cast<const float4*>(win)[0];
    const float tx0 = (float)(tx * RND_TILE_W) + 0.5f, tx1 = (float)min((tx + 1) * RND_TILE_W, a.width) - 0.5f;
    const float ty0 = (float)(ty * RND_TILE_H) + 0.5f, ty1 = (float)min((ty + 1) * RND_TILE_H, a.height) - 0.5f;
    const bool hit = box.x <= tx1 && box.z >= tx0 && box.y <= ty1 && box.w >= ty0;       // uniform over the workgroup

    float best_w = 0.f, best_ea = 0.f, best_eb = 0.f, best_ec = 0.f;
    int best = -1;
    if (hit) {
        for (int i = tid; i < nvt; i += RND_THREADS) s_vert[i] = *reinterpret_cast<const float4*>(rec + (size_t)i * RND_RECORD_FLOATS);
        __syncthreads();
        const float px = (float)c + 0.5f, py = (float)r + 0.5f;
        for (int k0 = 0; k0 < a.nfaces; k0 += RND_THREADS) {
            // keep the faces whose bounding box meets the tile, in ascending order
            const int k = k0 + tid;
            bool keep = false;
            int ia = 0, ib = 0, ic = 0;
            if (k < a.nfaces) {
                ia = a.faces[3 * k]; ib = a.faces[3 * k + 1]; ic = a.faces[3 * k + 2];
                if ((unsigned)ia < (unsigned)nvt && (unsigned)ib < (unsigned)nvt && (unsigned)ic < (unsigned)nvt) {
                    const float4 A = s_vert[ia], Bv = s_vert[ib], Cv = s_vert[ic];
                    keep = A.z > 0.f && Bv.z > 0.f && Cv.z > 0.f &&
                           fminf(A.x, fminf(Bv.x, Cv.x)) <= tx1 && fmaxf(A.x, fmaxf(Bv.x, Cv.x)) >= tx0 &&
                           fminf(A.y, fminf(Bv.y, Cv.y)) <= ty1 && fmaxf(A.y, fmaxf(Bv.y, Cv.y)) >= ty0;
                }
            }
            const unsigned long long m = __ballot(keep);
            const int lane = tid & 63, wv = tid >> 6;
            if (lane == 0) s_wave_cnt[wv] = __popcll(m);
            __syncthreads();
            int base = 0, total = 0;
#pragma unroll
            for (int q = 0; q < RND_THREADS / 64; ++q) {
                const int n = s_wave_cnt[q];
                base += (q < wv) ? n : 0;
                total += n;
            }
            if (keep) s_list[base + __popcll(m & ((1ull << lane) - 1ull))] = make_int4(ia, ib, ic, k);
            __syncthreads();
            for (int j = 0; j < total; ++j) {
                const int4 fk = s_list[j];
                const float4 A = s_vert[fk.x], Bv = s_vert[fk.y], Cv = s_vert[fk.z];
                // edge functions relative to a vertex of the triangle: differences of the size of the triangle, not of the image
                const float e_ab = __fsub_rn(__fmul_rn(Bv.x - A.x, py - A.y), __fmul_rn(Bv.y - A.y, px - A.x));
                const float e_bc = __fsub_rn(__fmul_rn(Cv.x - Bv.x, py - Bv.y), __fmul_rn(Cv.y - Bv.y, px - Bv.x));
                const float e_ca = __fsub_rn(__fmul_rn(A.x - Cv.x, py - Cv.y), __fmul_rn(A.y - Cv.y, px - Cv.x));
                const bool in = (e_ab >= 0.f && e_bc >= 0.f && e_ca >= 0.f) || (e_ab <= 0.f && e_bc <= 0.f && e_ca <= 0.f);
                const float tot = e_ab + e_bc + e_ca;
                if (in && tot != 0.f) {
                    const float w = __fdiv_rn(e_bc * A.z + e_ca * Bv.z + e_ab * Cv.z, tot);
                    if (w > best_w) {                                            // ascending faces: an equal depth keeps the lower index
                        best_w = w; best = fk.w;
                        best_ea = e_bc * A.z; best_eb = e_ca * Bv.z; best_ec = e_ab * Cv.z;
                    }
                }
            }
            __syncthreads();                                                     // s_list is rewritten by the next batch
        }
    }
    if (!live) return;
    uint8_t red = 0;
    float depth = 0.f;
    if (best >= 0) {
        depth = __fdiv_rn(1.f, best_w);
        const int ia = a.faces[3 * best], ib = a.faces[3 * best + 1], ic = a.faces[3 * best + 2];
        const float4 na = *reinterpret_cast<const float4*>(rec + (size_t)ia * RND_RECORD_FLOATS + 4);
        const float4 nb = *reinterpret_cast<const float4*>(rec + (size_t)ib * RND_RECORD_FLOATS + 4);
        const float4 nc = *reinterpret_cast<const float4*>(rec + (size_t)ic * RND_RECORD_FLOATS + 4);
        const float nx = best_ea * na.x + best_eb * nb.x + best_ec * nc.x;
        const float ny = best_ea * na.y + best_eb * nb.y + best_ec * nc.y;
        const float nz = best_ea * na.z + best_eb * nb.z + best_ec * nc.z;
        const float l2 = nx * nx + ny * ny + nz * nz;
        const float inten = l2 >= 1e-30f ? fminf(1.f, 0.3f + 0.7f * fabsf(nz) / sqrtf(l2)) : 0.3f;
        red = (uint8_t)(int)(inten * 255.f + 0.5f);
    }
    store_bgr(row + (size_t)(a.render_x0 + c) * 3, 0, 0, red);
    const size_t pix = ((size_t)b * a.height + r) * a.width + c;
    if (a.depth) a.depth[pix] = depth;
    if (a.face_id) a.face_id[pix] = best;
}

// Panels 1 and 2: one thread per sampled point.
__global__ __launch_bounds__(256) void demo_point_panels_kernel(const int32_t* __restrict__ yx, const float* __restrict__ pos, const float* __restrict__ neg,
                                                                const float* __restrict__ logits, size_t logits_stride, int B, int N, int width,
                                                                int height, uint8_t* __restrict__ frame, int frame_width, int event_x0, int seg_x0) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)B * N) return;
    const int b = (int)(t / N), n = (int)(t % N);
    const int y = yx[2 * t], x = yx[2 * t + 1];
    if ((unsigned)y >= (unsigned)height || (unsigned)x >= (unsigned)width) return;
    uint8_t* row = frame + ((size_t)b * height + y) * (size_t)frame_width * 3;
    if (event_x0 >= 0) {
        // ev2hands_r.py:155-156: (p / (p + n)) * 255 in float32, truncated into a uint8 array
        const float p = pos[t], q = neg[t], tot = __fadd_rn(p, q);
        uint8_t* o = row + (size_t)(event_x0 + x) * 3;
        o[0] = (uint8_t)(int)__fmul_rn(__fdiv_rn(p, tot), 255.f);
        o[2] = (uint8_t)(int)__fmul_rn(__fdiv_rn(q, tot), 255.f);
    }
    if (seg_x0 >= 0 && logits) {
        // demo.py:35: softmax(1).argmax(1), the first maximum on ties; :59-62
        const float* l = logits + (size_t)b * logits_stride + n;
        int cid = 0;
        float best = l[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float v = l[(size_t)k * N];
            if (v > best) { best = v; cid = k; }
        }
        uint8_t* o = row + (size_t)(seg_x0 + x) * 3;
        if (cid == 3) { o[0] = 255; o[1] = 255; o[2] = 255; }
        else o[cid] = 255;
    }
}

// What the reference's demo item calls 'coordinates' (ev2hands_r.py:149-154) plus the two counts, gathered from the builder's
// per-pixel table with the index clamping of event_window_sample_kernel.
__global__ __launch_bounds__(256) void event_window_pixels_kernel(const float* __restrict__ uniq, const int32_t* __restrict__ uniq_count, int cap,
                                                                  const int32_t* __restrict__ sample_idx, int B, int N, int32_t* __restrict__ yx,
                                                                  float* __restrict__ pos, float* __restrict__ neg) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)B * N) return;
    const int b = (int)(t / N);
    const int M = uniq_count[b];
    int i = sample_idx[t];
    i = (i < 0 || i >= M || i >= cap) ? 0 : i;
    const float* rec = uniq + ((size_t)b * cap + i) * 8;
    const float4 r0 = *reinterpret_cast<const float4*>(rec);
    yx[2 * t] = (int32_t)r0.y;
    yx[2 * t + 1] = (int32_t)r0.x;
    pos[t] = r0.w;
    neg[t] = rec[4];
}

}  // namespace

extern "C" int ev2h_event_window_pixels(const float* uniq, const int32_t* uniq_count, int cap, const int32_t* sample_idx, int B, int N,
                                        int32_t* yx, float* pos, float* neg, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(uniq && uniq_count && sample_idx && yx && pos && neg);
    EV2H_CHECK_ARG(B > 0 && N > 0 && cap > 0);
    const size_t total = (size_t)B * N;
    EV2H_CHECK_ARG(total <= (size_t)1 << 30);
    event_window_pixels_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(uniq, uniq_count, cap, sample_idx, B, N, yx, pos, neg);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" size_t ev2h_render_scratch_bytes(int B, int nv) {
    if (B <= 0 || nv <= 0 || 2 * nv > RND_MAX_VERTS) return 0;
    return (size_t)B * (RND_HEADER_FLOATS + (size_t)2 * nv * RND_RECORD_FLOATS) * sizeof(float);
}

extern "C" int ev2h_render_hands(const float* verts_left, const float* verts_right, size_t stride_left, size_t stride_right,
                                 const int32_t* faces, int nfaces, const int32_t* vf_offsets, const int32_t* vf_faces, int vf_len,
                                 int B, int nv, int width, int height, float f, float cx, float cy, float znear,
                                 uint8_t* frame, int frame_width, int render_x0, int clear_x0, int clear_width,
                                 float* depth, int32_t* face_id, void* scratch, size_t scratch_bytes, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(verts_left && verts_right && faces && vf_offsets && vf_faces && frame && scratch);
    EV2H_CHECK_ARG(B > 0 && B <= 65535 && nv > 0 && 2 * nv <= RND_MAX_VERTS && nfaces > 0 && vf_len >= 0);
    EV2H_CHECK_ARG(stride_left >= (size_t)nv * 3 && stride_right >= (size_t)nv * 3);
    EV2H_CHECK_ARG(width > 0 && height > 0 && width <= 4096 && height <= 4096 && f > 0.f && znear >= 0.f);
    EV2H_CHECK_ARG(frame_width >= width && render_x0 >= 0 && render_x0 + width <= frame_width);
    EV2H_CHECK_ARG(clear_width >= 0 && clear_x0 >= 0 && clear_x0 + clear_width <= frame_width && clear_width % width == 0);
    EV2H_CHECK_ARG(clear_width == 0 || clear_x0 + clear_width <= render_x0 || clear_x0 >= render_x0 + width);
    EV2H_CHECK_ARG(((uintptr_t)scratch & 15) == 0);
    if (scratch_bytes < ev2h_render_scratch_bytes(B, nv)) {
        ev2h_set_error("ev2h_render_hands: scratch of %zu bytes, %zu needed", scratch_bytes, ev2h_render_scratch_bytes(B, nv));
        return EV2H_ERR_WORKSPACE;
    }
    RenderArgs a{};
    a.verts[0] = verts_left; a.verts[1] = verts_right;
    a.vstride[0] = stride_left; a.vstride[1] = stride_right;
    a.faces = faces; a.vf_offsets = vf_offsets; a.vf_faces = vf_faces;
    a.nv = nv; a.nfaces = nfaces; a.vf_len = vf_len;
    a.width = width; a.height = height;
    a.f = f; a.cx = cx; a.cy = cy; a.znear = znear;
    a.scratch = static_cast<float*>(scratch);
    a.scratch_stride = RND_HEADER_FLOATS + (size_t)2 * nv * RND_RECORD_FLOATS;
    a.frame = frame; a.frame_width = frame_width; a.render_x0 = render_x0; a.clear_x0 = clear_x0; a.clear_width = clear_width;
    a.depth = depth; a.face_id = face_id;
    render_setup_kernel<<<B, RND_THREADS, 0, (hipStream_t)stream>>>(a);
    EV2H_CHECK_LAUNCH();
    const int tiles_x = ceil_div(width, RND_TILE_W), tiles_y = ceil_div(height, RND_TILE_H);
    render_raster_kernel<<<dim3(tiles_x * tiles_y, B), RND_THREADS, (size_t)2 * nv * sizeof(float4), (hipStream_t)stream>>>(a, tiles_x);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_demo_point_panels(const int32_t* yx, const float* pos, const float* neg, const float* logits, size_t logits_stride,
                                      int B, int N, int width, int height, uint8_t* frame, int frame_width, int event_x0, int seg_x0,
                                      ev2h_stream_t stream) {
    EV2H_CHECK_ARG(yx && frame && B > 0 && N > 0 && width > 0 && height > 0 && frame_width >= width);
    EV2H_CHECK_ARG(event_x0 < 0 || (pos && neg && event_x0 + width <= frame_width));
    EV2H_CHECK_ARG(seg_x0 < 0 || (logits && seg_x0 + width <= frame_width && logits_stride >= (size_t)4 * N));
    EV2H_CHECK_ARG(event_x0 >= 0 || seg_x0 >= 0);
    const size_t total = (size_t)B * N;
    EV2H_CHECK_ARG(total <= (size_t)1 << 30);
    demo_point_panels_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(yx, pos, neg, logits, logits_stride, B, N, width, height,
                                                                                           frame, frame_width, event_x0, seg_x0);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
