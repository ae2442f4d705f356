// The SMPL kinematic chain and its adjoint, joint by joint (lbs.py:276-377), in the single-lane form of k_smpl_pose_bwd: THE
// arithmetic of mp_smpl_pose_bwd / mp_smpl_pose_bwd_lbs (smpl.hip) and of the keypoint fit (keypoint_fit.hip).  The arrays may
// live in registers, scratch or LDS; every function is one joint's share, so a caller may run the joints in a loop on one lane or,
// where they do not depend on each other (Rodrigues and its adjoint), one joint per lane.
//   R [24][9] joint rotations, G [24][12] world transforms (rows 0..2), J [72] rest joints,
//   dG / dR / dJ the adjoints of G / R / J.
#pragma once
#include <hip/hip_runtime.h>

namespace mp {

// batch_rodrigues with angle = |theta + 1e-8|, axis = theta / angle (lbs.py:290-296)
__device__ __forceinline__ void smpl_rodrigues(const float* th, float* R) {
    const float ax = th[0] + 1e-8f, ay = th[1] + 1e-8f, az = th[2] + 1e-8f;
    const float ang = sqrtf(ax * ax + ay * ay + az * az);
    const float n[3] = {th[0] / ang, th[1] / ang, th[2] / ang};
    float s, c;
    sincosf(ang, &s, &c);
    const float K[9] = {0.f, -n[2], n[1], n[2], 0.f, -n[0], -n[1], n[0], 0.f};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            float kk = 0.f;
            for (int k = 0; k < 3; ++k) kk += K[3 * a + k] * K[3 * k + b];
            R[3 * a + b] = (a == b ? 1.f : 0.f) + s * K[3 * a + b] + (1.f - c) * kk;
        }
}

// G_j = G_p [R_j | J_j - J_p]  (G_0 = [R_0 | J_0]); p = parents[j], the parents come first
template <class RT, class GT>
__device__ __forceinline__ void smpl_chain_joint(int j, int p, const float* J, RT& R, GT& G) {
    float rel[3];
    for (int a = 0; a < 3; ++a) rel[a] = J[3 * j + a] - (j > 0 ? J[3 * p + a] : 0.f);
    if (j == 0) {
        for (int a = 0; a < 3; ++a) { for (int b = 0; b < 3; ++b) G[0][4 * a + b] = R[0][3 * a + b]; G[0][4 * a + 3] = rel[a]; }
    } else {
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) {
                float v = 0.f;
                for (int k = 0; k < 3; ++k) v += G[p][4 * a + k] * R[j][3 * k + b];
                G[j][4 * a + b] = v;
            }
            float v = G[p][4 * a + 3];
            for (int k = 0; k < 3; ++k) v += G[p][4 * a + k] * rel[k];
            G[j][4 * a + 3] = v;
        }
    }
}

// A_j = G_j with the translation column G_j[:,3] - G_j[:,:3] J_j (lbs.py:372-375): dA [12] -> dG_j (set), dJ_j (accumulated)
template <class GT, class DGT, class DJT>
__device__ __forceinline__ void smpl_rel_transform_adjoint(int j, const float* dA, const float* J, GT& G, DGT& dG, DJT& dJ) {
    for (int a = 0; a < 3; ++a) {
        for (int k = 0; k < 3; ++k) {
            dG[j][4 * a + k] = dA[4 * a + k] - dA[4 * a + 3] * J[3 * j + k];
            dJ[j][k] -= dA[4 * a + 3] * G[j][4 * a + k];
        }
        dG[j][4 * a + 3] = dA[4 * a + 3];
    }
}

// adjoint of smpl_chain_joint for j >= 1, the children first: dG_j -> dR_j (set), dG_p, dJ_j, dJ_p (accumulated)
template <class RT, class GT, class DGT, class DJT, class DRT>
__device__ __forceinline__ void smpl_chain_joint_adjoint(int j, int p, const float* J, RT& R, GT& G, DGT& dG, DJT& dJ, DRT& dR) {
    float rel[3];
    for (int a = 0; a < 3; ++a) rel[a] = J[3 * j + a] - J[3 * p + a];
    float drel[3] = {0.f, 0.f, 0.f};
    for (int b = 0; b < 3; ++b)
        for (int c2 = 0; c2 < 3; ++c2) {
            float v = 0.f;
            for (int a = 0; a < 3; ++a) v += G[p][4 * a + b] * dG[j][4 * a + c2];
            dR[j][3 * b + c2] = v;
        }
    for (int b = 0; b < 3; ++b)
        for (int a = 0; a < 3; ++a) drel[b] += G[p][4 * a + b] * dG[j][4 * a + 3];
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) {
            float v = dG[j][4 * a + 3] * rel[b];
            for (int c2 = 0; c2 < 3; ++c2) v += dG[j][4 * a + c2] * R[j][3 * b + c2];
            dG[p][4 * a + b] += v;
        }
        dG[p][4 * a + 3] += dG[j][4 * a + 3];
    }
    for (int a = 0; a < 3; ++a) { dJ[j][a] += drel[a]; dJ[p][a] -= drel[a]; }
}

// the root: G_0 = [R_0 | J_0]
template <class DGT, class DJT, class DRT>
__device__ __forceinline__ void smpl_chain_root_adjoint(DGT& dG, DJT& dJ, DRT& dR) {
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) dR[0][3 * a + b] = dG[0][4 * a + b];
        dJ[0][a] += dG[0][4 * a + 3];
    }
}

// adjoint of smpl_rodrigues: dR [9] -> d theta [3]
__device__ __forceinline__ void smpl_rodrigues_adjoint(const float* th, const float* dR, float* dth) {
    const float t3[3] = {th[0], th[1], th[2]};
    const float e3[3] = {t3[0] + 1e-8f, t3[1] + 1e-8f, t3[2] + 1e-8f};
    const float ang = sqrtf(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
    const float n[3] = {t3[0] / ang, t3[1] / ang, t3[2] / ang};
    float s, c;
    sincosf(ang, &s, &c);
    const float K[9] = {0.f, -n[2], n[1], n[2], 0.f, -n[0], -n[1], n[0], 0.f};
    float KK[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            float kk = 0.f;
            for (int k = 0; k < 3; ++k) kk += K[3 * a + k] * K[3 * k + b];
            KK[3 * a + b] = kk;
        }
    float dang = 0.f;
    for (int e = 0; e < 9; ++e) dang += dR[e] * (c * K[e] + s * KK[e]);
    // dK (adjoint of K): from s K and (1-c) K K  ->  dK = s dR + (1-c) (dR K^T + K^T dR)
    float dK[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            float v = s * dR[3 * a + b];
            for (int k = 0; k < 3; ++k) v += (1.f - c) * (dR[3 * a + k] * K[3 * b + k] + K[3 * k + a] * dR[3 * k + b]);
            dK[3 * a + b] = v;
        }
    const float dn[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
    float ndot = 0.f;
    for (int k = 0; k < 3; ++k) ndot += dn[k] * t3[k];
    for (int i = 0; i < 3; ++i) dth[i] = dang * e3[i] / ang + dn[i] / ang - ndot * e3[i] / (ang * ang * ang);
}

}  // namespace mp
