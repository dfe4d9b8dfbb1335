// Counter-based random draws on the device: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
// numbers: as easy as 1, 2, 3", SC'11).  A draw is a pure function of (seed, window id, stream, position): it does not depend on
// the batch a window is in, on its place in that batch, or on any draw made before.  tests/ref_philox.py is the NumPy restatement
// the kernels agree with bit for bit, held to the published known answers.
//
//   key     = (seed & 0xffffffff, seed >> 32), seed an unsigned 64-bit integer
//   counter = (block, window_id, stream, 0); one block is four 32-bit words
//   stream 0, the resampling indices: draw n of a window is word n % 4 of block n / 4
//   stream 1, the four farthest-point-sampling seeds: block 0, words 0..3 = enc.sa1, enc.sa2, left.sa1, right.sa1
//   stream 2, the training augmentation of an Ev2Hands-S window with M unique pixels (events.hip: event_window_augment_timesort_kernel):
//     block 0, word 0 is the coin: the window is augmented iff w0 >= 2^31; K = M / 32 noise rows follow
//     noise row j, block 1 + 2j: x = bounded(w0, width), y = bounded(w1, height), src = bounded(w2, M - 1) (the pixel-order row whose
//       mean time the noise time starts from), ps = w3 & 1, a = (w3 >> 8) & 7, b = (w3 >> 16) & 7; n_pos = a + ps, n_neg = b + !ps
//     noise row j, block 2 + 2j: u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53, a double in [0, 1) with 53 random bits;
//       t = (double)t_avg[src] + u * 1e3, the product rounded before the sum
//   stream 3, the Ev2Hands-R fine-tuning item (finetune.hip: finetune_resolve_kernel): block a belongs to attempt a = 0, 1, ... of a window;
//     the window length is 1 + (w0 >> 31) ms, the coin is up iff w1 >= 2^31, and if the attempt at global index i is rejected the
//     next index is bounded(w2, i - (min_events - 1)), the reference's inclusive randint(0, i - 2048) at min_events = 2048
//   stream 4, the polarity flips of an augmented fine-tuning window (events.hip: FlipPolarity): row e of the window (e < 32768, counted
//     from its first row) is flipped iff bit e & 31 of word (e >> 5) & 3 of block e >> 7 is set
//   stream 5, the five point lights of a simulated frame (shade.hip: shade_lights_kernel; the reference's generate_train_lights,
//     HandSimulator/utils.py:286-313, as a pure function of (seed, global frame)): window_id = the global frame number's low 32 bits.
//     light k = 0 .. 4, block 2k: the radiant intensity is 1 + (w0 >> 30), white; w1, w2, w3 give the jitter of x, y, z.  A uniform is
//     (word >> 8) * 2^-24, a float32 in [0, 1) (exact); the jitter is uniform / 10.  Lights 0, 1, 2 stand at (0, -1, 1), (0, 1, 1),
//     (1, 1, 2) + jitter.  Lights 3 and 4 take w0, w1, w2 of block 2k + 1 as three more uniforms u and stand at (2 u - 1) * 2 + jitter
//     per axis.  Every arithmetic step is one float32 rounding; the position is then mapped (x, y, z) -> (x, -y, -z) into the
//     rasteriser's camera frame.  Blocks 1, 3, 5 and word 3 of blocks 7 and 9 are not used.  These are the project's own draws, not
//     numpy's or Python's.
//   stream 6, the translation jitter of a simulated frame's rendered hands (forearm.hip: jitter_rows_kernel; the reference's
//     trans_jitter = 5 * np.random.random(3) / 1000, HandSimulator/twohands.py:67-73, as a pure function of (seed, global frame, hand)):
//     window_id = the global frame number's low 32 bits, block = the hand (0 left, 1 right); words 0, 1, 2 give the uniforms of x, y, z
//     as (word >> 8) * 2^-24; the jitter is (amplitude_mm * u) / 1000 metres, two float32 roundings, added to the float32 `transl` with
//     one more.  Word 3 is not used.
//   a 32-bit word u becomes an index below M by multiply-shift, (u * M) >> 32 in 64 bits.  There is NO rejection step, so the
//   indices are not exactly uniform: some values are hit by ceil(2^32 / M) words and the others by floor(2^32 / M), a relative
//   bias of at most M / 2^32 -- below 7.7e-6 for M <= 32768 (the largest table a window can have).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace ev2h_random {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;        // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;        // key increments (Weyl sequence)
constexpr uint32_t STREAM_SAMPLE = 0, STREAM_FPS = 1, STREAM_AUGMENT = 2, STREAM_FINETUNE = 3, STREAM_FLIP = 4, STREAM_LIGHTS = 5, STREAM_JITTER = 6;

struct u32x4 { uint32_t v[4]; };

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return u32x4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ u32x4 window_block(uint64_t seed, uint32_t window_id, uint32_t stream, uint32_t block) {
    return philox4x32_10(block, window_id, stream, 0u, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
}

// u -> [0, bound): the high word of the 64-bit product
__device__ __forceinline__ uint32_t bounded(uint32_t u, uint32_t bound) { return (uint32_t)(((uint64_t)u * (uint64_t)bound) >> 32); }

// two words -> a double in [0, 1) with 53 random bits (exact: the integer fits a double's significand)
__device__ __forceinline__ double unit_double(uint32_t w0, uint32_t w1) {
    return (double)(((uint64_t)(w0 >> 5) << 26) | (uint64_t)(w1 >> 6)) * 0x1p-53;
}

// a word -> a float32 in [0, 1) with 24 random bits (exact)
__device__ __forceinline__ float unit_float(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }

// word w (0..3) of a block by selects, not an indexed (scratch) read
__device__ __forceinline__ uint32_t block_word(const u32x4& b, uint32_t w) { return w == 0 ? b.v[0] : w == 1 ? b.v[1] : w == 2 ? b.v[2] : b.v[3]; }

// whether row e of window window_id is flipped (stream 4)
__device__ __forceinline__ bool flip_bit(uint64_t seed, uint32_t window_id, uint32_t e) {
    return (block_word(window_block(seed, window_id, STREAM_FLIP, e >> 7), (e >> 5) & 3u) >> (e & 31u)) & 1u;
}

// resampling index n of a window with M unique pixels
__device__ __forceinline__ int sample_index(uint64_t seed, uint32_t window_id, uint32_t n, uint32_t M) {
    const u32x4 b = window_block(seed, window_id, STREAM_SAMPLE, n >> 2);
    return (int)bounded(block_word(b, n & 3u), M);
}

}  // namespace ev2h_random
