// The library-owned side stream of ev2h_forward (side_stream.hip): one per caller stream, host thread and device.
#pragma once
#include "common.hpp"
#include "ev2hands_hip.h"

constexpr int FPS_CHUNKS = 4;       // launches enc.sa1's sampling is drawn in on the chunked path (forward.hip)

// The fork/join events of one forward, named by what has happened when the event fires.  (recorded on -> waited on by)
enum SideEvent {
    EV_SAMPLED,             // caller -> side: all three samplings drawn (un-chunked path only)
    EV_HAND_QUERIES,        // side -> caller: both hands' ball queries done (waited on before the regressors)
    EV_HF8,                 // caller -> side: hf8 written (right-hand regressor)
    EV_JOIN,                // side -> caller: the side stream has finished
    EV_INPUT,               // caller -> side: input prepared (the fork)
    EV_SA1_TABLE,           // side -> caller: enc.sa1's layer-1 table written (waited on by the un-chunked path only)
    EV_L0,                  // caller -> side: l0 written (classifier)
    EV_LOGITS,              // side -> caller: logits written (fused query convolution, attention)
    EV_SA2_QUERY,           // side -> caller: enc.sa2's sampling + ball query done
    EV_FP1_NN,              // side -> caller: fp1's 3-NN selection done
    // caller -> side: enc.sa3 done and fp3's bias row written (forward.hip: side_queries) -- the selections nobody reads before fp1
    // and the regressors wait for it, so that they run beside fp3 / fp2 and not beside the fused set-abstraction kernels
    EV_ENC_SA3,
    // side -> caller, + c: quarter c of enc.sa1's centroids drawn (chunked path) -- and, where the side stream runs the ball queries
    // (forward.hip: side_queries), their neighbours found.  Such a query writes centroid range c of WS_GIDX1_* / WS_CNT1 while the
    // caller's stream still reads the ranges of earlier quarters: the ranges are disjoint (ev2h_ball_query_range's s_off / s_cnt,
    // ev2h_sa_desc.s_off), so only this edge orders them.
    EV_SA1_QUARTER0,
    EV_COUNT = 15
};
static_assert(EV_SA1_QUARTER0 + FPS_CHUNKS == EV_COUNT, "one event per chunk of enc.sa1's sampling");

struct SideCtx {
    hipStream_t stream = nullptr;
    hipEvent_t ev[EV_COUNT] = {};
    int state = 0;               // 0 = not tried, 1 = ready, -1 = disabled
    void* owner = nullptr;       // the caller's stream this side stream serves (slot 0: the first caller's, claimed at its first forward)
    bool claimed = false;
    bool bound = false;          // ev2h_bind_stream has measured this pair (and replaced the stream if it shared the caller's hardware queue)
    unsigned long long last_use = 0;      // tick of the last forward / probe that looked this slot up (recycling, see ev2h_side_ctx)
};

// the side stream that serves `caller_stream` on the current device, or nullptr (single-stream mode); claim: this call binds a slot
// to its caller stream (ev2h_forward, ev2h_bind_stream, the probe -- not ev2h_init)
SideCtx* ev2h_side_ctx(void* caller_stream, bool claim);
extern thread_local int g_side_disabled;      // ev2h_set_side_stream(0): run everything on the caller's stream (per host thread)
