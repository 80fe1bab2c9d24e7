// Private device helpers shared by the dataset-side sources (smplx.hip: frames_to_world; rederive.hip: the between-stage
// re-derivation; clips.hip: the clip builder): scipy's float64 rotation-vector <-> matrix conversions and the reference's
// float32 quaternion algebra without fma contraction.
#pragma once
#include "common.h"

namespace rohm {

// scipy Rotation.from_rotvec(...).as_matrix(), incl. the small-angle series of from_rotvec
__device__ __forceinline__ void rotvec_to_matrix_f64(const double* rv, double* M) {
    const double a2 = rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2];
    const double a = sqrt(a2);
    const double sc = (a <= 1e-3) ? 0.5 - a2 / 48.0 + a2 * a2 / 3840.0 : sin(a / 2.0) / a;
    const double x = sc * rv[0], y = sc * rv[1], z = sc * rv[2], w = cos(a / 2.0);
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    M[0] = x2 - y2 - z2 + w2; M[1] = 2 * (xy - zw);       M[2] = 2 * (xz + yw);
    M[3] = 2 * (xy + zw);       M[4] = -x2 + y2 - z2 + w2; M[5] = 2 * (yz - xw);
    M[6] = 2 * (xz - yw);       M[7] = 2 * (yz + xw);       M[8] = -x2 - y2 + z2 + w2;
}

__device__ __forceinline__ void matrix_to_rotvec_f64(const double* M, double* rv) {
    // scipy Rotation.from_matrix (Markley's quaternion extraction) followed by as_rotvec
    double dec[4] = {M[0], M[4], M[8], M[0] + M[4] + M[8]};
    int choice = 0;
    for (int i = 1; i < 4; ++i)
        if (dec[i] > dec[choice]) choice = i;
    double q[4];
    if (choice != 3) {
        const int i = choice, j = (i + 1) % 3, k = (j + 1) % 3;
        q[i] = 1 - dec[3] + 2 * M[i * 3 + i];
        q[j] = M[j * 3 + i] + M[i * 3 + j];
        q[k] = M[k * 3 + i] + M[i * 3 + k];
        q[3] = M[k * 3 + j] - M[j * 3 + k];
    } else {
        q[0] = M[7] - M[5];
        q[1] = M[2] - M[6];
        q[2] = M[3] - M[1];
        q[3] = 1 + dec[3];
    }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] /= n;
    if (q[3] < 0) for (int i = 0; i < 4; ++i) q[i] = -q[i];
    const double ang = 2 * atan2(sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), q[3]);
    const double a2 = ang * ang;
    const double sc = (ang <= 1e-3) ? 2 + a2 / 12 + 7 * a2 * a2 / 2880 : ang / sin(ang / 2);
    rv[0] = sc * q[0]; rv[1] = sc * q[1]; rv[2] = sc * q[2];
}

// scipy Rotation.from_rotvec(rv).as_euler('zxy', degrees=True): extrinsic rotations about z, x, y, i.e.
// R = Ry(e[2]) Rx(e[1]) Rz(e[0]); first and third angle in [-180, 180], the middle one in [-90, 90]
__device__ __forceinline__ void rotvec_to_euler_zxy_deg_f64(const double* rv, double* e) {
    double M[9];
    rotvec_to_matrix_f64(rv, M);
    const double k = 180.0 / M_PI;
    e[0] = atan2(M[3], M[4]) * k;
    e[1] = asin(fmin(1.0, fmax(-1.0, -M[5]))) * k;
    e[2] = atan2(M[2], M[8]) * k;
}

// scipy Rotation.from_euler('zxy', e, degrees=True).as_rotvec(): q = qy qx qz, w >= 0, rotation angle in [0, pi]
__device__ __forceinline__ void euler_zxy_deg_to_rotvec_f64(const double* e, double* rv) {
    const double k = M_PI / 360.0;
    const double ca = cos(e[0] * k), sa = sin(e[0] * k), cb = cos(e[1] * k), sb = sin(e[1] * k);
    const double cc = cos(e[2] * k), sc = sin(e[2] * k);
    // qx qz = (cb ca, sb ca, -sb sa, cb sa); then qy = (cc, 0, sc, 0) from the left
    const double w1 = cb * ca, x1 = sb * ca, y1 = -sb * sa, z1 = cb * sa;
    double q[4] = {cc * x1 + sc * z1, cc * y1 + sc * w1, cc * z1 - sc * x1, cc * w1 - sc * y1};   // x, y, z, w
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] /= n;
    if (q[3] < 0) for (int i = 0; i < 4; ++i) q[i] = -q[i];
    const double ang = 2 * atan2(sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), q[3]);
    const double a2 = ang * ang;
    const double sc2 = (ang <= 1e-3) ? 2 + a2 / 12 + 7 * a2 * a2 / 2880 : ang / sin(ang / 2);
    rv[0] = sc2 * q[0]; rv[1] = sc2 * q[1]; rv[2] = sc2 * q[2];
}

// scipy's Rotation.from_rotvec: (x, y, z, w), incl. the small-angle series (cf. rotvec_to_matrix_f64)
__device__ __forceinline__ void rotvec_to_quat_f64(const double* rv, double* q) {
    const double a2 = rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2];
    const double a = sqrt(a2);
    const double sc = (a <= 1e-3) ? 0.5 - a2 / 48.0 + a2 * a2 / 3840.0 : sin(a / 2.0) / a;
    q[0] = sc * rv[0]; q[1] = sc * rv[1]; q[2] = sc * rv[2]; q[3] = cos(a / 2.0);
}

// unit quaternion -> shortest rotation vector (the tail of matrix_to_rotvec_f64)
__device__ __forceinline__ void quat_to_rotvec_f64(double* q, double* rv) {
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] /= n;
    if (q[3] < 0) for (int i = 0; i < 4; ++i) q[i] = -q[i];
    const double ang = 2 * atan2(sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), q[3]);
    const double a2 = ang * ang;
    const double sc = (ang <= 1e-3) ? 2 + a2 / 12 + 7 * a2 * a2 / 2880 : ang / sin(ang / 2);
    rv[0] = sc * q[0]; rv[1] = sc * q[1]; rv[2] = sc * q[2];
}

__device__ __forceinline__ void slerp_rotvec_f64(const double* r0, const double* r1, double alpha, double* out) {
    double q0[4], q1[4], q[4];
    rotvec_to_quat_f64(r0, q0);
    rotvec_to_quat_f64(r1, q1);
    double d = q0[0] * q1[0] + q0[1] * q1[1] + q0[2] * q1[2] + q0[3] * q1[3];
    if (d < 0) {
        d = -d;
        for (int i = 0; i < 4; ++i) q1[i] = -q1[i];
    }
    const double omega = atan2(sqrt(fmax(1.0 - d * d, 0.0)), d);
    const double so = sin(omega);
    double w0 = 1.0 - alpha, w1 = alpha;
    if (!(so < 1e-8)) {
        w0 = sin((1.0 - alpha) * omega) / so;
        w1 = sin(alpha * omega) / so;
    }
    for (int i = 0; i < 4; ++i) q[i] = w0 * q0[i] + w1 * q1[i];
    quat_to_rotvec_f64(q, out);
}

// angle (rad) of the relative rotation between two rotation vectors: 2 atan2(|v|, |w|) of qa^-1 qb, accurate at angle 0
// (an arccos of the trace is not); tests/track_ref.py `geodesic`
__device__ __forceinline__ double geodesic_rotvec_f64(const double* ra, const double* rb) {
    double qa[4], qb[4];
    rotvec_to_quat_f64(ra, qa);
    rotvec_to_quat_f64(rb, qb);
    const double w = qa[3] * qb[3] + qa[0] * qb[0] + qa[1] * qb[1] + qa[2] * qb[2];
    const double v[3] = {qa[3] * qb[0] - qb[3] * qa[0] - (qa[1] * qb[2] - qa[2] * qb[1]),
                         qa[3] * qb[1] - qb[3] * qa[1] - (qa[2] * qb[0] - qa[0] * qb[2]),
                         qa[3] * qb[2] - qb[3] * qa[2] - (qa[0] * qb[1] - qa[1] * qb[0])};
    return 2.0 * atan2(sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), fabs(w));
}

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }

__device__ __forceinline__ void cross_rn(const float* a, const float* b, float* o) {
    o[0] = sub(mul(a[1], b[2]), mul(a[2], b[1]));
    o[1] = sub(mul(a[2], b[0]), mul(a[0], b[2]));
    o[2] = sub(mul(a[0], b[1]), mul(a[1], b[0]));
}

// qrot (quaternion.py:52-71): v + 2 (w (u x v) + u x (u x v)), u = q.xyz
__device__ __forceinline__ void qrot_rn(const float* q, const float* v, float* o) {
    float uv[3], uuv[3];
    cross_rn(q + 1, v, uv);
    cross_rn(q + 1, uv, uuv);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = add(v[c], mul(2.f, add(mul(q[0], uv[c]), uuv[c])));
}

// qbetween(v0, +y) normalised (quaternion.py:26-28,385-394), float32; NaN when v0 has no direction
__device__ __forceinline__ void qbetween_y_rn(const float* v0, float* q) {
    const float v1[3] = {0.f, 1.f, 0.f};
    float v[3];
    cross_rn(v0, v1, v);
    const float n0 = add(add(mul(v0[0], v0[0]), mul(v0[1], v0[1])), mul(v0[2], v0[2]));
    const float dt = add(add(mul(v0[0], v1[0]), mul(v0[1], v1[1])), mul(v0[2], v1[2]));
    const float w = add(sqrtf(mul(n0, 1.f)), dt);
    const float qn = sqrtf(add(add(add(mul(w, w), mul(v[0], v[0])), mul(v[1], v[1])), mul(v[2], v[2])));
    q[0] = __fdiv_rn(w, qn); q[1] = __fdiv_rn(v[0], qn); q[2] = __fdiv_rn(v[1], qn); q[3] = __fdiv_rn(v[2], qn);
}

// w and z of qmul(q1, qinv(q0)) (quaternion.py:31-49: terms[i][j] = r_i q_j with r = qinv(q0), q = q1)
__device__ __forceinline__ void qmul_inv_wz_rn(const float* q1, const float* q0, float& vw, float& vz) {
    const float r[4] = {q0[0], -q0[1], -q0[2], -q0[3]};
    vw = sub(sub(sub(mul(r[0], q1[0]), mul(r[1], q1[1])), mul(r[2], q1[2])), mul(r[3], q1[3]));
    vz = add(add(sub(mul(r[0], q1[3]), mul(r[1], q1[2])), mul(r[2], q1[1])), mul(r[3], q1[0]));
}

}  // namespace rohm
