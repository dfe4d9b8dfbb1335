// The float64 evaluation of the MANO layer's joint chain, the pieces that mano_backward_kernel (loss_grad.hip) and the fits' Hand
// (mano_fit_steps.hpp) run alike, each written once: widened float32 inputs, theta + 1e-8 Rodrigues through the quaternion
// normalisation.  Not for mano.hip (float32, the forward's own arithmetic) nor pose_track.hip's layer_quat (another rounding).
#pragma once
#include "common.hpp"

namespace {

// the layer's output order: position -> source (0..15 chain joints, 16..20 fingertips), and its inverse
__constant__ int c_mano_reorder[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};
__constant__ int c_mano_position[21] = {0, 5, 6, 7, 9, 10, 11, 17, 18, 19, 13, 14, 15, 1, 2, 3, 4, 8, 12, 16, 20};

// Rodrigues, quaternion route, theta + 1e-8 inside the norm: R[9] of the axis-angle t[3]
__device__ __forceinline__ void mano_rotation(const double* t, double* R) {
    const double x = t[0], y = t[1], z = t[2];
    const double ex = x + 1e-8, ey = y + 1e-8, ez = z + 1e-8;
    const double ang = sqrt(ex * ex + ey * ey + ez * ez);
    const double ha = ang * 0.5, cs = cos(ha), sn = sin(ha);
    double qw = cs, qx = sn * (x / ang), qy = sn * (y / ang), qz = sn * (z / ang);
    const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw /= qn; qx /= qn; qy /= qn; qz /= qn;
    R[0] = qw * qw + qx * qx - qy * qy - qz * qz; R[1] = 2 * qx * qy - 2 * qw * qz; R[2] = 2 * qw * qy + 2 * qx * qz;
    R[3] = 2 * qw * qz + 2 * qx * qy; R[4] = qw * qw - qx * qx + qy * qy - qz * qz; R[5] = 2 * qy * qz - 2 * qw * qx;
    R[6] = 2 * qx * qz - 2 * qw * qy; R[7] = 2 * qw * qx + 2 * qy * qz; R[8] = qw * qw - qx * qx - qy * qy + qz * qz;
}

// G[k] = G[par] * [R_k | J_k - J_par] on rows of [R | t]
__device__ __forceinline__ void chain_step(const double* P, const double* R, const double* Jk, const double* Jp, double* G) {
    const double d[3] = {Jk[0] - Jp[0], Jk[1] - Jp[1], Jk[2] - Jp[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double p0 = P[4 * r], p1 = P[4 * r + 1], p2 = P[4 * r + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) G[4 * r + c] = fma(p2, R[6 + c], fma(p1, R[3 + c], p0 * R[c]));
        G[4 * r + 3] = fma(p2, d[2], fma(p1, d[1], p0 * d[0])) + P[4 * r + 3];
    }
}

// Kinematic chain: finger f's three joints 3 f + 1 .. 3 f + 3 walked down from the root G[0] = [R_0 | J_0], which finger 0 writes.
// Called by five lanes, one per finger.
__device__ __forceinline__ void finger_chain(int f, const double (*R)[9], const double (*J)[3], double (*G)[12]) {
    double P[12], Gk[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        P[4 * r] = R[0][3 * r]; P[4 * r + 1] = R[0][3 * r + 1]; P[4 * r + 2] = R[0][3 * r + 2]; P[4 * r + 3] = J[0][r];
    }
    if (f == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) G[0][e] = P[e];
    }
#pragma unroll
    for (int lev = 1; lev <= 3; ++lev) {
        const int k = 3 * f + lev, par = lev == 1 ? 0 : k - 1;
        chain_step(P, R[k], J[k], J[par], Gk);
#pragma unroll
        for (int e = 0; e < 12; ++e) { G[k][e] = Gk[e]; P[e] = Gk[e]; }
    }
}

}  // namespace
