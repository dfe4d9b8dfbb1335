// The forward's side streams: the slot table, the stream-concurrency probe and ev2h_bind_stream.
//
// The two MANO regressors are independent after the attention block, and their ball queries depend only on the
// sampled centroids.  They are forked onto one library-owned side stream per host thread (fork/join with events,
// hipGraph-capturable), so the small kernels of one hand (ball query, table GEMM, head GEMMs, MANO) overlap the
// MFMA-heavy kernels of the other and fill their tails: +1.5-2 % windows/s at B=256, outputs bit-identical
// (tests/test_gpu_forward.py::test_two_stream_fork_is_bit_identical).  EV2H_TWO_STREAMS=0 keeps everything on the caller's
// stream.  Kernels of the two hands then overlap in time, so bench.py brackets a launch site before the fork (sa2.1).
// One side stream (+ its events) per host thread AND per device: a second wrapper on another GPU in the same thread gets
// its own stream on that device.
#include <cstdlib>
#include <vector>

#include "side_stream.hpp"

constexpr int EV2H_MAX_DEVICES = 16;
// [r6] One side stream PER CALLER STREAM (up to EV2H_SIDE_SLOTS per host thread and device): forwards that are in flight at the same
// time on different streams (ev2hands_amd/inflight.py, dist.GatherPipeline(inflight=K)) used to share ONE side stream -- harmless
// while it carried only the tails of a forward, but since enc.sa1's sampling runs there (chunked, ev2h_fps_multi_chunk) forward
// i + 1's sampling queued behind forward i's right-hand regressor and two forwards in flight bought nothing (16 x 8192: 7 557
// against 7 568 windows/s with one).  Slot 0 is the stream ev2h_init creates first (it wants a hardware queue of its own).
constexpr int EV2H_SIDE_SLOTS = 4;
static thread_local SideCtx g_side[EV2H_MAX_DEVICES][EV2H_SIDE_SLOTS];
static thread_local unsigned long long g_side_tick = 0;
thread_local int g_side_disabled = 0;

extern "C" int ev2h_set_side_stream(int enabled) {
    const int prev = !g_side_disabled;
    g_side_disabled = !enabled;
    return prev;
}

static void side_open(SideCtx& c) {
    if (c.state == 0) {
        const char* e = getenv("EV2H_TWO_STREAMS");
        c.state = -1;
        // A NORMAL-priority, non-blocking stream, created as early as possible (ev2h_init).  Measured alternatives, 1-rank RCCL
        // process, B = 256 (profiles/r3_dist_overhead.txt): a low- or high-priority side stream (its own queue class): -12 %;
        // GPU_MAX_HW_QUEUES=8 with the side stream created first: -10 % (more hardware queues than the scheduler maps at once);
        // side stream created after torch's / RCCL's streams with the default 4 queues: -5 % (it shares the caller's queue).
        if (!(e && atoi(e) == 0) && hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) == hipSuccess) {
            bool ok = true;
            for (int i = 0; i < EV_COUNT; ++i) ok = ok && hipEventCreateWithFlags(&c.ev[i], hipEventDisableTiming) == hipSuccess;
            if (ok) c.state = 1;
        }
    }
}

SideCtx* ev2h_side_ctx(void* caller_stream, bool claim) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= EV2H_MAX_DEVICES) return nullptr;
    int slot = 0;
    if (caller_stream || g_side[dev][0].claimed) {
        // the slot that already serves this caller stream, else the first free one; all taken: the slot that has not been looked up
        // for the longest time is RECYCLED if it has been idle for a while (a host that keeps making new streams -- one
        // InflightForward per request, torch's pool handing out other handles -- would otherwise be stuck with its first four
        // forever), else slot 0 is shared (correct, only serialised: more than four streams in rotation must not evict each other --
        // every eviction costs a probe).  Handing a side stream to a new owner is safe whatever it is still running: each forward
        // forks it by an event wait and joins it by an event before it returns, and the enqueue calls of one host thread do not interleave.
        int found = -1, free_ = -1, lru = 0;
        for (int i = 0; i < EV2H_SIDE_SLOTS; ++i) {
            if (g_side[dev][i].claimed && g_side[dev][i].owner == caller_stream) { found = i; break; }
            if (!g_side[dev][i].claimed && free_ < 0) free_ = i;
            if (g_side[dev][i].last_use < g_side[dev][lru].last_use) lru = i;
        }
        slot = found >= 0 ? found : (free_ >= 0 ? free_ : 0);
        if (found < 0 && free_ < 0 && claim && g_side_tick - g_side[dev][lru].last_use >= 16) {
            slot = lru;
            g_side[dev][slot].claimed = false;          // re-claimed just below, for the new owner; measured again by ev2h_bind_stream
            g_side[dev][slot].bound = false;
        }
    }
    SideCtx& c = g_side[dev][slot];
    if (claim && !c.claimed) { c.claimed = true; c.owner = caller_stream; }
    if (claim && c.claimed && c.owner == caller_stream) c.last_use = ++g_side_tick;
    side_open(c);
    return c.state == 1 ? &c : nullptr;
}

namespace {
// spins for ~ticks of the constant-rate real-time counter (100 MHz on gfx950) without touching memory
__global__ void spin_kernel(unsigned long long ticks) {
    const unsigned long long r0 = wall_clock64();
    while (wall_clock64() - r0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// (time of one spin kernel on each of a and b at once) / (time of one on a alone): ~1.0-1.3 = concurrent, ~2 = the streams share a hardware queue
hipError_t probe_pair(hipStream_t a, hipStream_t b, int spin_us, float* ratio) {
    *ratio = 0.f;
    hipEvent_t e[6] = {};
    hipError_t err = hipSuccess;
    for (auto& x : e) if (err == hipSuccess) err = hipEventCreate(&x);
    int rate_khz = 100000, dev = 0;                         // wall_clock64 ticks per millisecond
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || rate_khz <= 0) rate_khz = 100000;
    const unsigned long long ticks = (unsigned long long)rate_khz * (unsigned long long)spin_us / 1000ull;
    float one = 0.f, two = 0.f;
    for (int rep = 0; rep < 2 && err == hipSuccess; ++rep) {   // (first repetition: code load, queue wake-up)
        err = hipEventRecord(e[0], a);
        spin_kernel<<<1, 64, 0, a>>>(ticks);
        if (err == hipSuccess) err = hipEventRecord(e[1], a);
        if (err == hipSuccess) err = hipEventRecord(e[4], a);                   // fork exactly as ev2h_forward does
        if (err == hipSuccess) err = hipStreamWaitEvent(b, e[4], 0);
        if (err == hipSuccess) err = hipEventRecord(e[2], a);
        spin_kernel<<<1, 64, 0, a>>>(ticks);
        spin_kernel<<<1, 64, 0, b>>>(ticks);
        if (err == hipSuccess) err = hipEventRecord(e[5], b);
        if (err == hipSuccess) err = hipStreamWaitEvent(a, e[5], 0);
        if (err == hipSuccess) err = hipEventRecord(e[3], a);
        if (err == hipSuccess) err = hipStreamSynchronize(a);
    }
    if (err == hipSuccess) err = hipEventElapsedTime(&one, e[0], e[1]);
    if (err == hipSuccess) err = hipEventElapsedTime(&two, e[2], e[3]);
    for (auto& x : e) if (x) (void)hipEventDestroy(x);
    if (err == hipSuccess) *ratio = one > 0.f ? two / one : 0.f;
    return err;
}
constexpr float SERIALISED = 1.6f;          // concurrent pairs measure 1.0-1.3 (the second launch's latency), serialised ones 1.9-2.1
}  // namespace

extern "C" int ev2h_streams_concurrent(ev2h_stream_t a, ev2h_stream_t b, int spin_us, float* ratio) {
    EV2H_CHECK_ARG(ratio && spin_us > 0 && spin_us <= 100000);
    const hipError_t err = probe_pair((hipStream_t)a, (hipStream_t)b, spin_us, ratio);
    if (err != hipSuccess) { ev2h_set_error("ev2h_streams_concurrent: %s", hipGetErrorString(err)); return EV2H_ERR_HIP; }
    return EV2H_OK;
}

extern "C" int ev2h_side_stream_probe(ev2h_stream_t stream, int spin_us, float* ratio) {
    EV2H_CHECK_ARG(ratio && spin_us > 0 && spin_us <= 100000);
    *ratio = 0.f;
    SideCtx* side = ev2h_side_ctx(stream, true);
    if (!side || g_side_disabled) {
        ev2h_set_error("ev2h_side_stream_probe: the side stream is switched off");
        return EV2H_ERR_ARG;
    }
    const hipError_t err = probe_pair((hipStream_t)stream, side->stream, spin_us, ratio);
    if (err != hipSuccess) { ev2h_set_error("ev2h_side_stream_probe: %s", hipGetErrorString(err)); return EV2H_ERR_HIP; }
    return EV2H_OK;
}

// [r6] HIP multiplexes a process's streams onto a few hardware queues (4 by default) and two streams that share one run IN ORDER, without
// any error.  Which queue a stream gets depends on what the process created before it (torch's pool of 32, RCCL's streams, other
// libraries): with the library's side stream created first and one forward at a time the default mapping works (ev2h_init), but
// with forwards in flight on several caller streams -- each with a side stream of its own -- no creation order is right for every
// host (measured in the 1-rank RCCL process, 16 x 8192, profiles/r6_side_slots_ab.txt: every slot created at ev2h_init: two in flight
// 9 010 windows/s but ONE in flight 5 980 instead of 7 400 and B = 256 -4 %; slots created at first use: one in flight 7 400, two
// 7 350 instead of 9 000).  So the mapping is MEASURED: ev2h_bind_stream probes candidate side streams against the caller's stream and
// against the streams this thread has bound before, and keeps the one that really runs beside them.
extern "C" int ev2h_bind_stream(ev2h_stream_t stream, int* info) {
    if (info) info[0] = info[1] = info[2] = 0;
    if (g_side_disabled) return EV2H_OK;
    int dev = 0;
    EV2H_CHECK_HIP(hipGetDevice(&dev));
    EV2H_CHECK_ARG(dev >= 0 && dev < EV2H_MAX_DEVICES);
    SideCtx* side = ev2h_side_ctx(stream, true);
    if (!side) return EV2H_OK;                                  // single-stream mode: nothing to bind
    if (!(side->claimed && side->owner == stream)) return EV2H_OK;   // every slot taken: this stream shares slot 0 (serialised with its owner's tails, correct)
    if (side->bound) return EV2H_OK;                            // measured before: the cheap path of a call per forward
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return EV2H_OK;      // the probe synchronises: not now (stays unbound)
    // the streams bound before on this thread and device: a good side stream also stays out of THEIR way
    std::vector<hipStream_t> others;
    for (int i = 0; i < EV2H_SIDE_SLOTS; ++i) {
        SideCtx& o = g_side[dev][i];
        if (&o == side || !o.claimed || o.state != 1) continue;
        others.push_back((hipStream_t)o.owner);
        others.push_back(o.stream);
    }
    constexpr int SPIN_US = 40;
    hipError_t err = hipSuccess;
    auto score = [&](hipStream_t cand, float* own_ratio) {      // 100 if serialised with its own caller stream, + 1 per other stream it is serialised with
        int sc = 0;
        float r = 0.f;
        if (err == hipSuccess) err = probe_pair(st, cand, SPIN_US, &r);
        *own_ratio = r;
        if (r > SERIALISED) sc += 100;
        for (hipStream_t o : others) {
            float ro = 0.f;
            if (err == hipSuccess) err = probe_pair(o, cand, SPIN_US, &ro);
            if (ro > SERIALISED) ++sc;
        }
        return sc;
    };
    float best_ratio = 0.f;
    int best = score(side->stream, &best_ratio), tried = 1;
    std::vector<hipStream_t> rejected;
    while (err == hipSuccess && best > 0 && tried < 8) {
        hipStream_t cand = nullptr;
        if (hipStreamCreateWithFlags(&cand, hipStreamNonBlocking) != hipSuccess) break;
        ++tried;
        float r = 0.f;
        const int sc = score(cand, &r);
        if (err == hipSuccess && sc < best) { rejected.push_back(side->stream); side->stream = cand; best = sc; best_ratio = r; }
        else rejected.push_back(cand);
    }
    // (destroyed only now: a destroyed stream's queue slot would be handed to the next candidate)
    for (hipStream_t r : rejected) (void)hipStreamDestroy(r);
    if (err != hipSuccess) { ev2h_set_error("ev2h_bind_stream: %s", hipGetErrorString(err)); return EV2H_ERR_HIP; }
    side->bound = true;
    // (best > 0: more streams in flight than hardware queues -- two forwards and their side streams fill the default four.  Running
    //  such a caller stream WITHOUT a side stream was measured and is worse: 16 x 8192, three in flight, 8 470 against 9 030 windows/s.)
    if (info) { info[0] = tried; info[1] = (int)(best_ratio * 1000.f + 0.5f); info[2] = best % 100; }
    return EV2H_OK;
}
