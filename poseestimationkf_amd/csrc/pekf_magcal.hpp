// pekf_magcal.hpp -- what the two phase-1 kernels share (k_magcal, pekf_magcal.hip: the whole plane in one
// launch; k_magcal_resume, pekf_magcal_resume.hip: the plane fed in chunks): the block shape, the event ring, the
// sweep count, sym6 and the Jacobi rotation.
//
// Below them, for k_magcal_resume alone: one sample's row of the normal equations, the 6 x 6 solve with R's
// principal square root, and the store of a phone's outputs -- k_magcal's own statements a second time, as
// phase 2's pass is stated twice (pekf_phase2.hpp says why).  They were written to be called by both kernels;
// k_magcal calling them computed the same bits with the same VGPRs and no scratch, but its gfx950 listing was
// not instruction for instruction the one it had (scripts/live_listing_diff.py: the accumulators of pass 2 in
// other registers, four more scalar instructions at the loop's exit; the row alone, shared, moved registers
// too), so k_magcal stays as it was written and measured.  Change one statement, change the other: every test of
// tests/test_magcal_resume.py compares the two kernels bit for bit.
//
// Last, MagcalState: the layout of k_magcal_resume's session state, which k_session_recycle
// (pekf_session_recycle.hip) needs too, to write a column's fresh form.
#pragma once
#include "pekf_phase3.hpp"

namespace pekf {

constexpr int kMcBlock = 256;
constexpr bool kMcNtl = true;   // non-temporal event loads: every event is read once per pass (as phase 2's)
constexpr int kMcRing = 8;         // event rows in flight per lane (k_frontend_init's)
constexpr int kJacobiSweeps = 6;   // 3 x 3 symmetric: off-diagonal below 1e-15 of the norm after 6

// index of entry (i, j), i <= j, of a symmetric 6 x 6 held as its 21 upper entries
__host__ __device__ constexpr int sym6(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// One Jacobi rotation of the symmetric 3 x 3 {a[p][p], a[q][q], a[p][q], a[r][p], a[r][q]} (r the third
// index) and of the eigenvector columns p, q.  tau = (aqq - app) / (2 apq), t = the smaller root of
// t^2 + 2 tau t - 1 = 0; a zero apq needs no rotation.
__device__ __forceinline__ void jacobi_rot(double &app, double &aqq, double &apq, double &arp, double &arq,
                                           double (&vp)[3], double (&vq)[3]) {
#pragma clang fp contract(off)
    if (apq == 0.0) return;
    const double tau = (aqq - app) / (2.0 * apq);
    const double t = __builtin_copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double kp = vp[k], kq = vq[k];
        vp[k] = c * kp - s * kq;
        vq[k] = s * kp + c * kq;
    }
}

// Pass 2, one sample: the centred sample's row [x^2, y^2, z^2, 2xy, 2zx, 2yz] added to the 21 unique entries of
// A^T A and the 6 of A^T 1 (setUncalibratedValues, :65-80).  (sx, sy, sz): the sample as a double.
__device__ __forceinline__ void magcal_add_row(double sx, double sy, double sz, double bx, double by, double bz,
                                               double (&ata)[21], double (&atb)[6]) {
    const double x = sx - bx, y = sy - by, z = sz - bz;
    const double d[6] = {x * x, y * y, z * z, 2.0 * x * y, 2.0 * z * x, 2.0 * y * z};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        atb[i] += d[i];
#pragma unroll
        for (int j = i; j < 6; ++j) ata[sym6(i, j)] = __builtin_fma(d[i], d[j], ata[sym6(i, j)]);
    }
}

// A phone's outputs: status st, and for st == 0 the bias, W and the fit; otherwise bias 0, W = I, fit NaN.
__device__ __forceinline__ void magcal_store(int64_t b, int st, double bx, double by, double bz,
                                             const double (&w)[3][3], const double (&xs)[6], double *cal, double *fit,
                                             int32_t *status) {
    const bool ok = st == 0;
    const double nan = __builtin_nan("");
    double *c = cal + 12 * b;
    c[0] = ok ? bx : 0.0;
    c[1] = ok ? by : 0.0;
    c[2] = ok ? bz : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 + 3 * i + j] = ok ? w[i][j] : (i == j ? 1.0 : 0.0);
    if (fit) {
#pragma unroll
        for (int i = 0; i < 6; ++i) fit[6 * b + i] = ok ? xs[i] : nan;
    }
    status[b] = st;
}

// From the normal equations to the phone's outputs (setW, :159-200): the Cholesky solve, R's eigen-decomposition,
// W = V sqrt(D) V^T, the status and the store.  fired: the phone has had its message n_cal + 1.
__device__ __forceinline__ void magcal_solve_store(int64_t b, bool fired, double bx, double by, double bz,
                                                   double (&ata)[21], const double (&atb)[6], double *cal, double *fit,
                                                   int32_t *status) {
    // the 6 x 6 solve: Cholesky A^T A = L L^T in place (L[j][i] in ata's entry (i, j)), no pivoting
    bool spd = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = ata[sym6(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= ata[sym6(k, j)] * ata[sym6(k, j)];
        spd = spd && d > 0.0 && isfinite(d);
        const double l = sqrt(d), il = 1.0 / l;
        ata[sym6(j, j)] = l;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = ata[sym6(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= ata[sym6(k, i)] * ata[sym6(k, j)];
            ata[sym6(j, i)] = s * il;
        }
    }
    double xs[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {  // L y = A^T 1
        double s = atb[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= ata[sym6(k, i)] * xs[k];
        xs[i] = s / ata[sym6(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {  // L^T x = y
        double s = xs[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= ata[sym6(i, k)] * xs[k];
        xs[i] = s / ata[sym6(i, i)];
    }

    // R = [[a, d, e], [d, b, f], [e, f, c]] (:165-175) and its eigen-decomposition by cyclic Jacobi
    double a00 = xs[0], a11 = xs[1], a22 = xs[2], a01 = xs[3], a02 = xs[4], a12 = xs[5];
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};  // eigenvector columns
#pragma unroll
    for (int s = 0; s < kJacobiSweeps; ++s) {
        jacobi_rot(a00, a11, a01, a02, a12, v0, v1);
        jacobi_rot(a00, a22, a02, a01, a12, v0, v2);
        jacobi_rot(a11, a22, a12, a01, a02, v1, v2);
    }
    const bool ell = a00 > 0.0 && a11 > 0.0 && a22 > 0.0 && isfinite(a00) && isfinite(a11) && isfinite(a22);
    // W = V sqrt(D) V^T (:191-196): the 6 unique entries, mirrored
    double w[3][3];
    {
#pragma clang fp contract(off)
        const double r0 = sqrt(a00), r1 = sqrt(a11), r2 = sqrt(a22);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j)
                w[i][j] = w[j][i] = (r0 * v0[i] * v0[j] + r1 * v1[i] * v1[j]) + r2 * v2[i] * v2[j];
    }
    const int st = !fired ? 1 : !spd ? 2 : !ell ? 3 : 0;
    magcal_store(b, st, bx, by, bz, w, xs, cal, fit, status);
}

// The state of a session's phase 1, lane-minor planes as the other session states (pekf_phase3.hpp: state_plane):
//   planes 0, 1 (16 B per lane each): {sum x, sum y}, {sum z, the message count in the low word};
//   then 3 n_cal planes of 8 B per lane: component c of sample k of every phone is plane 3 k + c, so the phones
//   that advance together store and load contiguous rows.
// Per phone 32 + 24 n_cal bytes, rounded up to a multiple of 16 (an odd n_cal leaves 8 B unused).  Both event
// forms keep doubles: (double)f of an f32 sample is exact.
struct MagcalState {
    static constexpr int kHeadPlanes = 2;
    static __host__ __device__ constexpr int64_t bytes_per_phone(int n_cal) {
        return 16 * kHeadPlanes + (((int64_t)24 * n_cal + 15) & ~(int64_t)15);
    }
    // component c of sample k of lane b.  One view of the buffer for stores and loads alike: pass 2 reads back
    // what the same lane may have stored earlier in the same launch.
    static __device__ __forceinline__ double *sample(void *state, int64_t batch, int64_t b, int k, int c) {
        return reinterpret_cast<double *>(state_plane(state, batch, 0, kHeadPlanes)) + ((int64_t)(3 * (int64_t)k + c) * batch + b);
    }
};

}  // namespace pekf
