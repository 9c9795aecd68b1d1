// pekf_magcal.hip -- phase 1 of the server's client session on the device: the per-phone magnetometer
// calibration (KFS/Magnetometer_Calibration.cpp), batched, one lane per phone.
//
// The client's "Magnetometer Calibration" stage sends magnetometer messages only
// (ASC/SensorActivities.java:57-65); the server hands every phase-1 message's sample to setValues,
// whatever its Type field says (KFS/Parser.cpp:30-34,144-147).  setValues (:13-43) keeps the first
// total_values (= n_cal, 100) samples and their running sum; message n_cal + 1 divides the sum (the
// bias, :20-22) and fits an ellipsoid (setW, :178-200): with v = m - bias, the least-squares solution of
// [x^2, y^2, z^2, 2xy, 2zx, 2yz] . {a, b, c, d, e, f} = 1 over the n_cal samples (:65-80,159-164),
// R = [[a, d, e], [d, b, f], [e, f, c]] (:165-175) and W = V sqrt(D) V^T, R's principal square root
// (:184-196).  A sample is corrected to W (m - bias): the commented body of CorrectValues (:46-55),
// called at KFS/Parser.cpp:107 (phase 2, the raw sample) and :239 (phase 3, the interpolated sample).
//
// k_magcal: two passes over the event planes of phase 2 / 3's form ([n_events][batch], float4 or, with
// PEKF_EV_F64_EVENTS, double4), read with k_frontend_init's block reader (pekf_phase3.hpp:
// load_event_block).  Pass 1: the FP64 sum of the first n_cal samples in arrival
// order, divided by n_cal -- the reference's own sequence of operations, so the bias is its bias bit for
// bit.  Pass 2: the 21 unique entries of A^T A and the 6 of A^T 1, summed in FP64 from zero (what
// KFS/Matrix_multiplication.cu's ATA / ATb mean; that kernel adds into memory it never clears).  Then,
// per lane and with every index a compile-time constant (no scratch): an unpivoted Cholesky solve of the
// 6 x 6 system (the reference: colPivHouseholderQr, :164; samples spread over an ellipsoid give
// cond(A^T A) of a few hundred) and a cyclic Jacobi eigen-decomposition of R -- pairs (0,1), (0,2), (1,2),
// kJacobiSweeps sweeps, rotation t = sgn(tau) / (|tau| + sqrt(1 + tau^2)) (no trigonometric call; an
// infinite tau gives t = 0).  The reference's own loops stop at an off-diagonal of 1e-3 (JacobiMethod,
// :116-157); both approximate the principal root, which is what is built here.
//
// k_magcal_apply: W (m - bias) written over every magnetometer event (type 2) of an event plane, for the
// phones whose status is 0; every other event and every other phone's column is not written.  f32
// planes: the corrected sample is computed in FP64 and rounded to f32.  The correction is affine, so
// applying it to the raw samples before phase 3's interpolation (Parser.cpp:107's place) equals applying
// it after (:239's place) in real arithmetic: phase 3 agrees with the reference's placement within
// rounding, not bit for bit.
#include "pekf_magcal.hpp"

namespace pekf {

constexpr int kApplyRows = 64;     // k_magcal_apply: rows per lane at least (its 96 B of cal read once per chunk)
// k_magcal_apply: rows in flight per lane, plain loads and 24 B stores.  Measured at 1,048,576 phones x 1,024 FP64
// events (scripts/bench_magcal.py, interleaved twice): 12.0 ms; 8 rows in flight 12.1; whole 32 B events stored
// 12.1; non-temporal loads 17.2 (the stores go to the lines just read).
constexpr int kApplyRing = 4;

// (kMcBlock, kMcRing, kJacobiSweeps, sym6 and jacobi_rot: pekf_magcal.hpp, shared with k_magcal_resume.  Pass 2's
// body and the solve below are stated a second time there, for that kernel: calling the shared statement from
// here changed this kernel's register allocation and schedule, pekf_magcal.hpp says more.  Change one, change both;
// tests/test_magcal_resume.py holds the two to the same bits.)
template <bool EV64>
__global__ __launch_bounds__(kMcBlock) void k_magcal(int64_t batch, int64_t n_events,
                                                     const std::conditional_t<EV64, double4, float4> *__restrict__ ev,
                                                     int n_cal, double *__restrict__ cal, double *__restrict__ fit,
                                                     int32_t *__restrict__ status) {
    using EvT = std::conditional_t<EV64, double4, float4>;
    const int64_t b = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    if (b >= batch) return;
    const uint32_t lane = (uint32_t)b;
    const int32_t n_ev = (int32_t)n_events;  // < 2^30, checked on the host: the uniform tests stay scalar
    // pass 1: the sum of the first n_cal samples (setValues, :27-35); the lane counts its messages up to
    // n_cal + 1, the one that fires the fit (:18-25)
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int cnt = 0;
    for (int32_t e0 = 0; e0 < n_ev; e0 += kMcRing) {
        if (__all(cnt > n_cal)) break;  // every lane of the wave has seen its message n_cal + 1
        EvT r[kMcRing];
        load_event_block<kMcRing, kMcNtl>(ev, batch, lane, e0, n_ev, r);  // padded with null events: no messages
#pragma unroll
        for (int k = 0; k < kMcRing; ++k) {
#pragma clang fp contract(off)
            const EvT v4 = r[k];
            if (!is_message(v4)) continue;
            if (cnt < n_cal) {
                sx += (double)v4.x;
                sy += (double)v4.y;
                sz += (double)v4.z;
            }
            if (cnt <= n_cal) ++cnt;
        }
    }
    const bool fired = cnt > n_cal;
    const double bx = sx / (double)n_cal, by = sy / (double)n_cal, bz = sz / (double)n_cal;  // :20-22

    // pass 2: the normal equations of the same n_cal samples, centred (setUncalibratedValues, :65-80)
    double ata[21] = {}, atb[6] = {};
    int c2 = fired ? 0 : n_cal;  // a phone whose fit never fired reads nothing
    for (int32_t e0 = 0; e0 < n_ev; e0 += kMcRing) {
        if (__all(c2 >= n_cal)) break;
        EvT r[kMcRing];
        load_event_block<kMcRing, kMcNtl>(ev, batch, lane, e0, n_ev, r);
#pragma unroll
        for (int k = 0; k < kMcRing; ++k) {
            const EvT v4 = r[k];
            if (!is_message(v4) || c2 >= n_cal) continue;
            ++c2;
            const double x = (double)v4.x - bx, y = (double)v4.y - by, z = (double)v4.z - bz;
            const double d[6] = {x * x, y * y, z * z, 2.0 * x * y, 2.0 * z * x, 2.0 * y * z};
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                atb[i] += d[i];
#pragma unroll
                for (int j = i; j < 6; ++j) ata[sym6(i, j)] = __builtin_fma(d[i], d[j], ata[sym6(i, j)]);
            }
        }
    }

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

// grid.y: chunks of `rows` rows each; one lane per phone walks its chunk
template <bool EV64>
__global__ __launch_bounds__(kMcBlock) void k_magcal_apply(int64_t batch, int64_t n_events, int32_t rows,
                                                           std::conditional_t<EV64, double4, float4> *__restrict__ ev,
                                                           const double *__restrict__ cal,
                                                           const int32_t *__restrict__ status) {
    using EvT = std::conditional_t<EV64, double4, float4>;
    const int64_t b = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    if (b >= batch) return;
    if (status && status[b] != 0) return;  // not calibrated: the column is not written
    const int32_t n_ev = (int32_t)n_events;
    const int64_t first = (int64_t)blockIdx.y * rows;  // < n_events <= 2^30 by the host's chunking
    const int32_t r0 = (int32_t)first;
    if (r0 >= n_ev) return;
    const int32_t r1 = rows < n_ev - r0 ? r0 + rows : n_ev;
    double c[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = cal[12 * b + k];
    EvT *col = ev + b;
    for (int32_t e0 = r0; e0 < r1; e0 += kApplyRing) {
        EvT r[kApplyRing];
#pragma unroll
        for (int k = 0; k < kApplyRing; ++k) {  // rows past the chunk: its last row again (read only)
            const int32_t e = e0 + k < r1 ? e0 + k : r1 - 1;
            r[k] = col[(int64_t)e * batch];
        }
#pragma unroll
        for (int k = 0; k < kApplyRing; ++k) {
            if (e0 + k >= r1) break;  // uniform
            const EvT v4 = r[k];
            if (event_type(v4) != kEvMag) continue;
            const double x = (double)v4.x - c[0], y = (double)v4.y - c[1], z = (double)v4.z - c[2];
            const double ox = c[3] * x + c[4] * y + c[5] * z, oy = c[6] * x + c[7] * y + c[8] * z,
                         oz = c[9] * x + c[10] * y + c[11] * z;
            EvT *q = col + (int64_t)(e0 + k) * batch;
            if constexpr (EV64) {  // the time / type word stays as it is
                *reinterpret_cast<double2 *>(q) = make_double2(ox, oy);
                q->z = oz;
            } else {
                *q = make_float4((float)ox, (float)oy, (float)oz, v4.w);
            }
        }
    }
}

}  // namespace pekf

using namespace pekf;

extern "C" int pekf_magcal_dev(int64_t batch, int64_t n_events, const void *ev_planes, int n_cal, double *cal,
                               double *fit, int32_t *status, uint32_t flags, void *stream) {
    PEKF_CHECK_ARG(batch >= 0 && n_events >= 0, "negative size");
    PEKF_CHECK_ARG(n_cal >= 6 && n_cal < (1 << 30), "n_cal must be >= 6 (the fit has 6 unknowns) and < 2^30");
    PEKF_CHECK_ARG(n_events < ((int64_t)1 << 30), "n_events must be < 2^30 per launch");
    PEKF_CHECK_ARG((flags & ~(PEKF_EV_TIME_EVENTS | PEKF_EV_F64_EVENTS)) == 0, "unknown flags");
    if (batch == 0) return PEKF_OK;
    PEKF_CHECK_ARG(ev_planes && cal && status, "null pointer");
    PEKF_CHECK_ARG((uintptr_t)ev_planes % 16 == 0, "misaligned event planes");
    const dim3 grid(grid_for(batch, kMcBlock)), block(kMcBlock);
    dispatch_bools(
        [&](auto ev64) {  // time events are always honoured, as in phase 2
            using Ev = std::conditional_t<ev64.value, double4, float4>;
            hipLaunchKernelGGL(k_magcal<ev64.value>, grid, block, 0, as_stream(stream), batch, n_events,
                               static_cast<const Ev *>(ev_planes), n_cal, cal, fit, status);
        },
        (flags & PEKF_EV_F64_EVENTS) != 0);
    return launched("k_magcal");
}

extern "C" int pekf_magcal_apply_dev(int64_t batch, int64_t n_events, void *ev_planes, const double *cal,
                                     const int32_t *status, uint32_t flags, void *stream) {
    PEKF_CHECK_ARG(batch >= 0 && n_events >= 0, "negative size");
    PEKF_CHECK_ARG(n_events < ((int64_t)1 << 30), "n_events must be < 2^30 per launch");
    PEKF_CHECK_ARG((flags & ~(PEKF_EV_TIME_EVENTS | PEKF_EV_F64_EVENTS)) == 0, "unknown flags");
    if (batch == 0 || n_events == 0) return PEKF_OK;
    PEKF_CHECK_ARG(ev_planes && cal, "null pointer");
    PEKF_CHECK_ARG((uintptr_t)ev_planes % 16 == 0, "misaligned event planes");
    // chunks of at least kApplyRows rows, at most 65,535 of them (grid.y)
    int64_t chunks = (n_events + kApplyRows - 1) / kApplyRows;
    if (chunks > 65535) chunks = 65535;
    const int64_t rows = (n_events + chunks - 1) / chunks;
    const dim3 grid(grid_for(batch, kMcBlock), (unsigned)chunks), block(kMcBlock);
    dispatch_bools(
        [&](auto ev64) {
            using Ev = std::conditional_t<ev64.value, double4, float4>;
            hipLaunchKernelGGL(k_magcal_apply<ev64.value>, grid, block, 0, as_stream(stream), batch, n_events,
                               (int32_t)rows, static_cast<Ev *>(ev_planes), cal, status);
        },
        (flags & PEKF_EV_F64_EVENTS) != 0);
    return launched("k_magcal_apply");
}
