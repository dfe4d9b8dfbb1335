// The lit part of the simulator's appearance model, once: the glTF 2.0 metallic-roughness BRDF under point lights, the byte of a
// value and the reference's grey-level mask.  shade.hip (the hands) and forearm.hip (the forearm cylinders) both include it, so a
// forearm pixel and a hand pixel with the same normal, position and albedo get the same bytes.  include/ev2hands_hip.h
// (ev2h_esim_shade) and tests/ref_shade.py state the rule; every expression here is float32 with one rounding per operation
// (-ffp-contract=off), in the order that statement gives.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace ev2h_shade {

constexpr float SHD_PI = 3.14159265358979323846f;

__device__ __forceinline__ uint8_t to_byte(float x) { return (uint8_t)(int)(fminf(fmaxf(x, 0.f), 1.f) * 255.f + 0.5f); }

// augment_background's mask on the rounded bytes: cv2's 14-bit BGR2GRAY constants met by an RGB pixel, above 10 keeps the render
__device__ __forceinline__ bool grey_keeps(uint8_t o0, uint8_t o1, uint8_t o2) {
    return ((1868 * (int)o0 + 9617 * (int)o1 + 4899 * (int)o2 + 8192) >> 14) > 10;
}

// val += the lights' sum at the surface point P (metres, the rasteriser's camera frame) with UNIT normal n and albedo base;
// n is turned towards the viewer first.  lt: n_lights rows of (position, RGB radiant intensity), uniform over the workgroup.
__device__ __forceinline__ void add_lights(float nx, float ny, float nz, float Px, float Py, float Pz, const float (&base)[3],
                                           float metallic, float alpha2, float kd, const float* __restrict__ lt, int n_lights,
                                           float (&val)[3]) {
    const float plen = sqrtf(Px * Px + Py * Py + Pz * Pz);
    const float vx = -Px / plen, vy = -Py / plen, vz = -Pz / plen;
    float ndv = nx * vx + ny * vy + nz * vz;
    if (ndv < 0.f) { nx = -nx; ny = -ny; nz = -nz; ndv = -ndv; }
    float f0[3], cdiff[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f0[k] = 0.04f + (base[k] - 0.04f) * metallic;
        cdiff[k] = base[k] * kd;
    }
    const float a2 = alpha2, oma2 = 1.f - a2;
    for (int j = 0; j < n_lights; ++j) {
        const float lx = lt[6 * j] - Px, ly = lt[6 * j + 1] - Py, lz = lt[6 * j + 2] - Pz;
        const float d2 = lx * lx + ly * ly + lz * lz;
        if (!(d2 > 0.f)) continue;
        const float d = sqrtf(d2);
        const float ux = lx / d, uy = ly / d, uz = lz / d;
        const float ndl = nx * ux + ny * uy + nz * uz;
        if (!(ndl > 0.f)) continue;
        const float hx = ux + vx, hy = uy + vy, hz = uz + vz;
        const float h2 = hx * hx + hy * hy + hz * hz;
        if (!(h2 >= 1e-30f)) continue;
        const float hl = sqrtf(h2);
        const float hnx = hx / hl, hny = hy / hl, hnz = hz / hl;
        const float vdh = vx * hnx + vy * hny + vz * hnz;
        const float ndh = nx * hnx + ny * hny + nz * hnz;
        const float m = fmaxf(0.f, 1.f - vdh);
        const float m5 = m * m * m * m * m;
        float spec = 0.f;                                                // D Vis
        if (ndv > 0.f) {
            const float t = ndh * ndh * (a2 - 1.f) + 1.f;
            const float D = a2 / (SHD_PI * (t * t));
            const float vis = 0.5f / (ndl * sqrtf(ndv * ndv * oma2 + a2) + ndv * sqrtf(ndl * ndl * oma2 + a2));
            spec = D * vis;
        }
        const float geo = ndl / d2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float Fr = f0[k] + (1.f - f0[k]) * m5;
            val[k] += ((1.f - Fr) * cdiff[k] / SHD_PI + Fr * spec) * (lt[6 * j + 3 + k] * geo);
        }
    }
}

}  // namespace ev2h_shade
