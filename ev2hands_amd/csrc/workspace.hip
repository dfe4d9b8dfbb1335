// The workspace layout, its debug accessors (buffers and range records by name) and the F16X2 spread report.
#include <cstring>

#include "planes.hpp"
#include "workspace.hpp"

#define X(id, name, count) name,
static const char* const kWsNames[WS_COUNT] = {EV2H_WS_BUFFERS(X)};
#undef X
#define X(id, name) name,
static const char* const kRangeNames[R_COUNT] = {EV2H_RANGE_RECORDS(X)};
#undef X

thread_local int g_last_l0_bf16 = 0;

void build_layout(Layout& L, int B, int N) {
    const size_t R = (size_t)B * N;
    const size_t b = (size_t)B;
#define X(id, name, count) count,
    const size_t counts[WS_COUNT] = {EV2H_WS_BUFFERS(X)};
#undef X
    L.total = 0;
    for (int i = 0; i < WS_COUNT; ++i) {
        L.off[i] = L.total;
        L.count[i] = counts[i];
        L.total += (counts[i] * 4 + 255) / 256 * 256;
    }
}

static int find_name(const char* const* names, int n, const char* name) {
    for (int i = 0; i < n; ++i)
        if (!strcmp(names[i], name)) return i;
    return -1;
}

extern "C" size_t ev2h_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    Layout L;
    build_layout(L, B, N);
    return L.total;
}

extern "C" const void* ev2h_workspace_buffer(void* workspace, int B, int N, const char* name, size_t* count) {
    if (!workspace || !name || B <= 0 || N <= 0) return nullptr;
    Layout L;
    build_layout(L, B, N);
    if (!strncmp(name, "rng.", 4)) {                  // one F16X2 range record: "rng.<tensor>" -> uint32 [B]
        const int r = find_name(kRangeNames, R_COUNT, name + 4);
        if (r < 0) return nullptr;
        if (count) *count = (size_t)B;
        return static_cast<char*>(workspace) + L.off[WS_RANGES] + (size_t)r * B * 4;
    }
    const int id = find_name(kWsNames, WS_COUNT, name);
    if (id < 0) return nullptr;
    if (count) *count = L.count[id];
    return static_cast<char*>(workspace) + L.off[id];
}

extern "C" const void* ev2h_workspace_buffer_ex(void* workspace, int B, int N, const char* name, size_t* count, int* elem_type) {
    const void* p = ev2h_workspace_buffer(workspace, B, N, name, count);
    if (elem_type) *elem_type = (p && !strcmp(name, "l0")) ? g_last_l0_bf16 : 0;      // 1 = bf16, 2 = fp16 times p1scale[5][b]
    return p;
}

// ---------------------------------------------------------------------------------------- F16X2 spread report
// The operand tensors of the F16X2 contractions that are MATERIALISED in the workspace, as their consumers read them: buffer,
// rows per window, row stride, column range, and the range record(s) the consumer derives its power-of-two scale from (two
// records: the consumer takes their maximum -- a concatenated input).  Not listed: operands that never reach memory (the hidden
// layers inside the fused set-abstraction / row-chain kernels, whose scales come from bounds): TEHNet.verify_precision compares
// whole forwards for those.
struct SpreadEntry { const char* name; WsId buf; int rows; int ld; int col0; int ncols; int rec; int rec2; size_t hand_off; };
constexpr int EV2H_MAX_SPREAD = 32;

static int spread_entries(SpreadEntry* e) {      // rows == 0: N rows per window
    int n = 0;
    e[n++] = {"feat", WS_FEAT8, 0, 8, 0, 8, R_FEAT, -1, 0};
    e[n++] = {"l1", WS_L1CAT, 512, 576, 0, 320, R_L1A, -1, 0};
    e[n++] = {"l1cat", WS_L1CAT, 512, 576, 0, 576, R_L1A, R_L1B, 0};
    e[n++] = {"l2", WS_L2BUF, 128, 520, 0, 515, R_L2, R_FEAT, 0};
    e[n++] = {"sa3h1", WS_SA3H1, 128, 256, 0, 256, R_SA3H1, -1, 0};
    e[n++] = {"sa3h2", WS_SA3H2, 128, 512, 0, 512, R_SA3H2, -1, 0};
    e[n++] = {"l3", WS_L3, 1, 1024, 0, 1024, R_L3, -1, 0};
    e[n++] = {"fp3h", WS_FP3H, 128, 256, 0, 256, R_FP3H, -1, 0};
    e[n++] = {"fp3o", WS_FP3O, 128, 256, 0, 256, R_FP3O, -1, 0};
    e[n++] = {"fp2h", WS_FP2H, 512, 256, 0, 256, R_FP2H, -1, 0};
    e[n++] = {"l1new", WS_L1NEW, 512, 128, 0, 128, R_L1NEW, -1, 0};
    e[n++] = {"l0", WS_L0, 0, 256, 0, 256, R_L0, -1, 0};
    for (int h = 0; h < 2; ++h) {
        e[n++] = {h ? "hfR" : "hfL", WS_HF8, 0, 8, 0, 8, R_HF + h, -1, (size_t)h};
        e[n++] = {h ? "m1R" : "m1L", hand(WS_M1BUF_L, h), 128, 520, 0, 515, R_M1 + h, R_FEAT, 0};
        e[n++] = {h ? "msa2hR" : "msa2hL", hand(WS_MSA2H_L, h), 128, 256, 0, 256, R_MSA2H + h, -1, 0};
        e[n++] = {h ? "m2R" : "m2L", hand(WS_M2_L, h), 1, 512, 0, 512, R_M2 + h, -1, 0};
        e[n++] = {h ? "fc1R" : "fc1L", hand(WS_FC1_L, h), 1, 1024, 0, 1024, R_FC1 + h, -1, 0};
    }
    return n;
}

namespace {
// counts[b] = {non-zero values, values with 0 < |v| s < 2^-3 (low fp16 plane subnormal: fewer than 22 bits survive the split),
// values with 0 < |v| s < 2^-14 (high plane subnormal too: fewer than 11 bits)}, s = the consumer's power-of-two scale
// half_elems: the buffer holds fp16 values (F16 mode's l0: stored times a power of two, and so is its record -- the ratios are the same)
__global__ __launch_bounds__(256) void spread_count_kernel(const float* __restrict__ buf, size_t window_stride, int rows, int ld, int col0, int ncols,
                                                           const unsigned* __restrict__ rec, const unsigned* __restrict__ rec2,
                                                           unsigned* __restrict__ counts, int half_elems) {
    const int b = blockIdx.y;
    unsigned a = rec[b];
    if (rec2) a = max(a, rec2[b]);
    const float s = f16x2_scale(a);
    const float* base = buf + (size_t)b * window_stride;
    const size_t total = (size_t)rows * ncols;
    unsigned nz = 0, lo = 0, hi = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / ncols;
        const int c = (int)(i - r * ncols);
        const float v = fabsf(half_elems ? (float)reinterpret_cast<const _Float16*>(buf)[(size_t)b * window_stride + r * ld + col0 + c] : base[r * ld + col0 + c]) * s;
        nz += v > 0.f;
        lo += v > 0.f && v < 0.125f;
        hi += v > 0.f && v < 6.103515625e-05f;
    }
    nz = (unsigned)wave_sum_f32((float)nz); lo = (unsigned)wave_sum_f32((float)lo); hi = (unsigned)wave_sum_f32((float)hi);   // < 2^24 per wave: exact
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&counts[(size_t)b * 3 + 0], nz);
        atomicAdd(&counts[(size_t)b * 3 + 1], lo);
        atomicAdd(&counts[(size_t)b * 3 + 2], hi);
    }
}
}  // namespace

extern "C" int ev2h_range_report_entries(const char** names, int max_names) {
    SpreadEntry e[EV2H_MAX_SPREAD];
    const int n = spread_entries(e);
    for (int i = 0; i < n && names && i < max_names; ++i) names[i] = e[i].name;
    return n;
}

extern "C" int ev2h_range_report(void* workspace, int B, int N, uint32_t* counts, ev2h_stream_t st) {
    EV2H_CHECK_ARG(workspace && counts && B > 0 && N >= 128 && N <= 32768);
    Ws ws;
    ws.base = static_cast<char*>(workspace);
    ws.B = B;
    ws.ranges_on = true;
    build_layout(ws.L, B, N);
    SpreadEntry e[EV2H_MAX_SPREAD];
    const int n = spread_entries(e);
    EV2H_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)n * B * 3 * sizeof(uint32_t), (hipStream_t)st));
    for (int i = 0; i < n; ++i) {
        const int rows = e[i].rows ? e[i].rows : N;
        const float* p = ws.f(e[i].buf) + e[i].hand_off * (size_t)B * N * 8;      // hf8: [2][B * N][8]
        const size_t per_window = (size_t)rows * e[i].ld;
        const int gx = (int)std::min<size_t>(64, ((size_t)rows * e[i].ncols + 4095) / 4096);
        spread_count_kernel<<<dim3(std::max(gx, 1), B), 256, 0, (hipStream_t)st>>>(p, per_window, rows, e[i].ld, e[i].col0, e[i].ncols, ws.r(e[i].rec),
                                                                                  e[i].rec2 >= 0 ? ws.r(e[i].rec2) : nullptr, counts + (size_t)i * B * 3,
                                                                                  (e[i].buf == WS_L0 && g_last_l0_bf16 == 2) ? 1 : 0);
        EV2H_CHECK_LAUNCH();
    }
    return EV2H_OK;
}
