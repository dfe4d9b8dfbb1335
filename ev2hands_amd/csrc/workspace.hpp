// The workspace of ev2h_forward: one declaration per buffer and per F16X2 range record, from which the id, the debug name
// (ev2h_workspace_buffer) and the size all come.  The order IS the layout (tests/workspace_layout.json pins it).
#pragma once
#include <algorithm>

#include "common.hpp"
#include "ev2hands_hip.h"

size_t ev2h_fps_state_ld(int N);      // points.hip

// X(id, name, elements of 4 bytes); R = B * N rows, b = B windows
#define EV2H_WS_HAND_BUFFERS(X, S, s)   \
    X(P1M##S, "P1m" s, R * 256)         \
    X(FPSM##S, "fpsm" s, b * 128)       \
    X(CTRM##S, "ctrm" s, b * 128 * 4)   \
    X(GIDXM0##S, "gidxm0" s, b * 128 * 64)  \
    X(GIDXM1##S, "gidxm1" s, b * 128 * 128) \
    X(CNTM##S, "cntm" s, b * 128 * 2)   \
    X(M1BUF##S, "m1buf" s, b * 128 * 520)   \
    X(MSA2H##S, "msa2h" s, b * 128 * 256)   \
    X(M2##S, "m2" s, b * 512)           \
    X(FC1##S, "fc1" s, b * 1024)
#define EV2H_WS_BUFFERS(X)              \
    X(PTS4, "pts4", R * 4)              \
    X(FEAT8, "feat8", R * 8)            \
    X(FPS1, "fps1", b * 512)            \
    X(CTR1, "ctr1", b * 512 * 4)        \
    X(P1A, "P1a", R * 160)              \
    X(GIDX1_0, "gidx1_0", b * 512 * 32) \
    X(GIDX1_1, "gidx1_1", b * 512 * 64) \
    X(GIDX1_2, "gidx1_2", b * 512 * 128)    \
    X(CNT1, "cnt1", b * 512 * 3)        \
    X(L1CAT, "l1cat", b * 512 * 576)    \
    X(P1B, "P1b", b * 512 * 256)        \
    X(FPS2, "fps2", b * 128)            \
    X(CTR2, "ctr2", b * 128 * 4)        \
    X(GIDX2_0, "gidx2_0", b * 128 * 64) \
    X(GIDX2_1, "gidx2_1", b * 128 * 128)    \
    X(CNT2, "cnt2", b * 128 * 2)        \
    X(L2BUF, "l2buf", b * 128 * 520)    \
    X(SA3H1, "sa3h1", b * 128 * 256)    \
    X(SA3H2, "sa3h2", b * 128 * 512)    \
    X(L3, "l3", b * 1024)               \
    X(FP3BIAS, "fp3bias", b * 256)      \
    X(FP3H, "fp3h", b * 128 * 256)      \
    X(FP3O, "fp3o", b * 128 * 256)      \
    X(FP2H, "fp2h", b * 512 * 256)      \
    X(L1NEW, "l1new", b * 512 * 128)    \
    /* 16-bit modes: layer-1 table of fp1 (fp1in / fp1h1 / fp1h2 are then unused) */ \
    X(FP1T, "fp1T", b * 512 * 128)      \
    X(FP1IN, "fp1in", R * 128)          \
    X(FP1H1, "fp1h1", R * 128)          \
    X(FP1H2, "fp1h2", R * 128)          \
    X(L0, "l0", R * 256)                \
    X(CLSH, "clsh", R * 256)            \
    X(LOGITS_PM, "logits_pm", R * 4)    \
    X(Q1, "q1", R * 512)                \
    /* (fused form: one partial per 128 rows) */ \
    X(ZPART, "zpart", std::max(ev2h_attn_sim_folded_scratch(B, N), b * ceil_div(N, 128) * 12 * 512)) \
    X(SIM, "sim", b * 2 * 4 * 256)      \
    X(HF8, "hf8", 2 * R * 8)            \
    X(NN2_IDX, "nn2_idx", b * 512 * 3)  \
    X(NN2_W, "nn2_w", b * 512 * 3)      \
    X(NN1_IDX, "nn1_idx", R * 3)        \
    X(NN1_W, "nn1_w", R * 3)            \
    EV2H_WS_HAND_BUFFERS(X, _L, "L")    \
    EV2H_WS_HAND_BUFFERS(X, _R, "R")    \
    /* F16X2 range records (uint32 [R_COUNT][B]) ... */ \
    X(RANGES, "ranges", (size_t)R_COUNT * b) \
    /* chunked sampling of small batches: running minima between the launches */ \
    X(FPS_STATE, "fps_state", b * 3 * ev2h_fps_state_ld(N)) \
    /* ... and the storage scales of the five layer-1 tables (float [5][B]) + [5]: of l0 when it is stored as fp16 (F16) */ \
    X(P1SCALE, "p1scale", 6 * b)

// F16X2 range records (ev2hands_hip.h "Range records"): one uint32 [B] array per tensor that a contraction reads.
// X(id, name); a per-hand tensor has two records, left then right: R_HF + h
#define EV2H_RANGE_RECORDS(X)                                                                                               \
    X(FEAT, "feat") X(L1A, "l1a") X(L1B, "l1b") X(L2, "l2") X(SA3H1, "sa3h1") X(SA3H2, "sa3h2") X(L3, "l3") X(FP3H, "fp3h") \
    X(FP3O, "fp3o") X(FP2H, "fp2h") X(L1NEW, "l1new") X(FP1IN, "fp1in") X(FP1H1, "fp1h1") X(FP1H2, "fp1h2") X(L0, "l0")     \
    X(CLSH, "clsh") X(Q1, "q1") X(HF, "hfL") X(HF_R, "hfR") X(M1, "m1L") X(M1_R, "m1R") X(MSA2H, "msa2hL")                  \
    X(MSA2H_R, "msa2hR") X(M2, "m2L") X(M2_R, "m2R") X(FC1, "fc1L") X(FC1_R, "fc1R") X(P1A, "p1a") X(P1B, "p1b")            \
    X(P1M, "p1mL") X(P1M_R, "p1mR") X(FP1T, "fp1t")

#define X(id, name, count) WS_##id,
enum WsId { EV2H_WS_BUFFERS(X) WS_COUNT };
#undef X
#define X(id, name) R_##id,
enum RangeId { EV2H_RANGE_RECORDS(X) R_COUNT };
#undef X

// the right hand's buffer of a left-hand id: hand(WS_M1BUF_L, h)
constexpr WsId hand(WsId left, int h) { return WsId(left + h * (WS_P1M_R - WS_P1M_L)); }

struct Layout {
    size_t off[WS_COUNT];       // bytes
    size_t count[WS_COUNT];     // elements (4 bytes each)
    size_t total = 0;
};
void build_layout(Layout& L, int B, int N);

struct Ws {
    char* base;
    Layout L;
    int B = 0;
    bool ranges_on = false;      // F16X2: range records are maintained and used
    float* f(WsId id) const { return reinterpret_cast<float*>(base + L.off[id]); }
    int32_t* i(WsId id) const { return reinterpret_cast<int32_t*>(base + L.off[id]); }
    uint32_t* r(int id) const { return ranges_on ? reinterpret_cast<uint32_t*>(base + L.off[WS_RANGES]) + (size_t)id * B : nullptr; }
    float* p1scale(int k) const { return ranges_on ? f(WS_P1SCALE) + (size_t)k * B : nullptr; }
};

// how the calling thread's last ev2h_forward stored l0: 0 float32, 1 bf16 (BF16), 2 fp16 x p1scale[5][b] (F16)
// (ev2h_workspace_buffer_ex tells a debugger what "l0" holds)
extern thread_local int g_last_l0_bf16;
