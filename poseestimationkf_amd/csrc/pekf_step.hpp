// pekf_step.hpp -- device code of the fused hot path shared by pekf_run.hip (one-record launches,
// the filter handle's update), pekf_run_multi.hip (multi-record launches over 40 B and FP64 records)
// and pekf_live.hip: the state layouts and the one-record kernels' state mover, the record planes' row
// cursor, one record of main_file.py:42-45 on a lane's registers (ekf_record_step: the FP64 step in its
// two forms, plain and loop, and the mixed-precision step, chosen by the covariance's type), the change
// to the reference frame's basis and the multi-record stream kernel template k_run.  The files are
// compiled with different scheduling strategies (Makefile), never different arithmetic.
#pragma once

#include <type_traits>

#include "pekf_internal.hpp"
#include "pekf_math.hpp"
#include "pekf_tile.hpp"

namespace pekf {

constexpr int kRunBlock = 256;

// Cache policy of the record loads: nt (aux = 2), as each record is read once per launch.
// Same box, config 3: 136.8 / 137.7 ms against 137.8 / 138.8 with the default policy
// (profiles/r1/ab_nt_loads/); sc0 nt 137.0 / 137.9; nt sc1 and sc0 nt sc1 +0.2 % (profiles/r3/ab_rec_cache_policy/).
#ifndef PEKF_REC_AUX
#define PEKF_REC_AUX 2
#endif

// Filter state in HBM.  AoS (default, the ABI's natural layout): X[b][4], P[b][4][4].  SoA
// (PEKF_RUN_STATE_SOA): X[4][batch] and the 10 unique entries of P as P[10][batch]
// (00 01 02 03 11 12 13 22 23 33): every state load / store of a wave is one contiguous
// 512 B access, which matters when a launch covers few records (online serving).
template <bool SOA, typename PT>
__device__ __forceinline__ void load_state(const double *X, const double *P, int64_t b, int64_t batch,
                                           double *x, Sym4T<PT> &S) {
    if (SOA) {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = X[k * batch + b];
        S = {(PT)P[0 * batch + b], (PT)P[1 * batch + b], (PT)P[2 * batch + b], (PT)P[3 * batch + b],
             (PT)P[4 * batch + b], (PT)P[5 * batch + b], (PT)P[6 * batch + b], (PT)P[7 * batch + b],
             (PT)P[8 * batch + b], (PT)P[9 * batch + b]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = X[4 * b + k];
        const double *pp = P + 16 * b;
        S = {(PT)pp[0], (PT)pp[1], (PT)pp[2], (PT)pp[3], (PT)pp[5],
             (PT)pp[6], (PT)pp[7], (PT)pp[10], (PT)pp[11], (PT)pp[15]};
    }
}

template <bool SOA, typename PT>
__device__ __forceinline__ void store_state(double *X, double *P, int64_t b, int64_t batch, const double *x,
                                            const Sym4T<PT> &S) {
    if (SOA) {
#pragma unroll
        for (int k = 0; k < 4; ++k) X[k * batch + b] = x[k];
        const double v[10] = {S.a00, S.a01, S.a02, S.a03, S.a11, S.a12, S.a13, S.a22, S.a23, S.a33};
#pragma unroll
        for (int k = 0; k < 10; ++k) P[k * batch + b] = v[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) X[4 * b + k] = x[k];
        double *po = P + 16 * b;
        po[0] = S.a00; po[1] = S.a01; po[2] = S.a02; po[3] = S.a03;
        po[4] = S.a01; po[5] = S.a11; po[6] = S.a12; po[7] = S.a13;
        po[8] = S.a02; po[9] = S.a12; po[10] = S.a22; po[11] = S.a23;
        po[12] = S.a03; po[13] = S.a13; po[14] = S.a23; po[15] = S.a33;
    }
}

// AoS P (full 4x4) <-> its upper triangle, for state moved through a WaveTile
template <typename PT>
__device__ __forceinline__ Sym4T<PT> sym_from16(const double (&p)[16]) {
    return {(PT)p[0], (PT)p[1], (PT)p[2], (PT)p[3], (PT)p[5], (PT)p[6], (PT)p[7], (PT)p[10], (PT)p[11], (PT)p[15]};
}
template <typename PT>
__device__ __forceinline__ void sym_to16(const Sym4T<PT> &S, double (&p)[16]) {
    p[0] = S.a00; p[1] = S.a01; p[2] = S.a02; p[3] = S.a03;
    p[4] = S.a01; p[5] = S.a11; p[6] = S.a12; p[7] = S.a13;
    p[8] = S.a02; p[9] = S.a12; p[10] = S.a22; p[11] = S.a23;
    p[12] = S.a03; p[13] = S.a13; p[14] = S.a23; p[15] = S.a33;
}

// The state of a one-record kernel (k_run_one, k_update; the AoS side of k_state_layout) between HBM
// and the lanes.  AoS: X and P move through the wave's tile in coalesced blocks (pekf_tile.hpp) --
// gather() starts the loads, where the kernel gathers its other operands; to_lanes() transposes them
// where the state is wanted.  SoA: per lane, one contiguous 512 B access per component and wave
// (load_state), and nothing to gather.  b: the lane's filter; an idle lane reads a valid one and
// stores nothing.
template <bool SOA, typename PT>
struct StateMover {
    const WaveTile &t;
    double *X, *P;
    int64_t batch;
    double cx[4], cp[16];  // AoS: the wave's blocks of X and P, in block order

    __device__ __forceinline__ StateMover(const WaveTile &tile, double *Xio, double *Pio, int64_t n)
        : t(tile), X(Xio), P(Pio), batch(n) {}
    __device__ __forceinline__ void gather() {
        if constexpr (!SOA) {
            t.gather(X, cx);
            t.gather(P, cp);
        }
    }
    __device__ __forceinline__ void to_lanes(int64_t b, double (&x)[4], Sym4T<PT> &S) const {
        if constexpr (SOA) {
            load_state<true>(X, P, b, batch, x, S);
        } else {
            double pv[16];
            t.to_lanes(cx, x);
            t.to_lanes(cp, pv);
            S = sym_from16<PT>(pv);
        }
    }
    __device__ __forceinline__ void store(int64_t b, const double (&x)[4], const Sym4T<PT> &S) const {
        if constexpr (SOA) {
            if (t.active()) store_state<true>(X, P, b, batch, x, S);
        } else {
            double pv[16];
            sym_to16(S, pv);
            t.store(X, x);
            t.store(P, pv);
        }
    }
};

// Buffer resource of one plane row (raw, byte-addressed; gfx9 DWORD3 0x00020000)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const void *row, int64_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(row), 0, (int)(uint32_t)bytes, 0x00020000);
}

// One aligned plane element of a row: 16 B is one load, a double4 two (the second at the
// instruction's immediate offset).  AUX: the cache policy bits.
template <int AUX>
__device__ __forceinline__ void row_load(__amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t so, float4 &v) {
    v = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, so, AUX));
}
template <int AUX>
__device__ __forceinline__ void row_load(__amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t so, float2 &v) {
    v = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs, off, so, AUX));
}
template <int AUX>
__device__ __forceinline__ void row_load(__amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t so, double2 &v) {
    v = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(rs, off, so, AUX));
}
template <int AUX>
__device__ __forceinline__ void row_load(__amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t so, double4 &v) {
    double2 lo, hi;
    row_load<AUX>(rs, off, so, lo);
    row_load<AUX>(rs, off + 16u, so, hi);
    v = make_double4(lo.x, lo.y, hi.x, hi.y);
}

// The rows of the three record planes a multi-record launch walks through, for the 40 B record (R =
// Rec: row r of a plane is batch x 16 B for gd / am, batch x 8 B for my) and the 80 B FP64 record
// (Rec64: batch x 32 B and batch x 16 B); the window wraps.  Rows are read through buffer
// descriptors of a CHUNK of consecutive rows with the row's offset inside the chunk in the
// instruction's scalar offset (soffset), so moving to the next row is two scalar adds and a compare,
// and the descriptors are rebuilt only when a chunk ends: chunk offsets stay below 2^31 (128 rows at
// config 3, the whole 1,024-row window at config 2).  Each descriptor's record count is its chunk's
// byte size and the range check covers soffset (measured: scripts/buffer_range_probe.hip), so an
// offset past the chunk would read zeros, never another allocation.  The lane offsets are 32-bit:
// batch < 2^28 (Rec) or 2^27 (Rec64), checked on the host.
template <typename R>
struct RowCursor {
    using Big = decltype(R::gd);    // gd, am
    using Small = decltype(R::my);
    const char *g, *a, *m;
    uint32_t row_big, row_small;    // bytes per row
    uint32_t off_big, off_small;    // this lane's offset within a row
    int32_t window, chunk_rows;
    int32_t row = 0, end = 0;
    uint32_t s_big = 0, s_small = 0;
    __amdgpu_buffer_rsrc_t rg, ra, rm;

    __device__ __forceinline__ RowCursor(const Big *gd, const Big *am, const Small *my, int64_t batch, int64_t win,
                                         uint32_t lane)
        : g(reinterpret_cast<const char *>(gd)), a(reinterpret_cast<const char *>(am)),
          m(reinterpret_cast<const char *>(my)), row_big((uint32_t)batch * (uint32_t)sizeof(Big)),
          row_small((uint32_t)batch * (uint32_t)sizeof(Small)), off_big(lane * (uint32_t)sizeof(Big)),
          off_small(lane * (uint32_t)sizeof(Small)), window((int32_t)win) {
        const uint32_t c = (1u << 31) / row_big;
        chunk_rows = c ? (int32_t)c : 1;
    }
    __device__ __forceinline__ void start(int32_t r) {
        row = r;
        end = (window - r < chunk_rows) ? window : r + chunk_rows;
        const uint64_t n = (uint64_t)(end - r);
        rg = row_rsrc(g + (uint64_t)r * row_big, (int64_t)(n * row_big));
        ra = row_rsrc(a + (uint64_t)r * row_big, (int64_t)(n * row_big));
        rm = row_rsrc(m + (uint64_t)r * row_small, (int64_t)(n * row_small));
        s_big = 0;
        s_small = 0;
    }
    __device__ __forceinline__ void advance() {
        if (++row == end) {
            start(row == window ? 0 : row);
        } else {
            s_big += row_big;
            s_small += row_small;
        }
    }
    __device__ __forceinline__ R load() const {
        R v;
        row_load<PEKF_REC_AUX>(rg, off_big, s_big, v.gd);
        row_load<PEKF_REC_AUX>(ra, off_big, s_big, v.am);
        row_load<PEKF_REC_AUX>(rm, off_small, s_small, v.my);
        return v;
    }
    // acc / mag of the record `lag` rows behind the cursor again (rare: the degenerate-Wahba fallback),
    // through one-row descriptors and the lane offsets the loop holds anyway (no 64-bit lane index is
    // kept live for this)
    __device__ __forceinline__ void reload(int32_t lag, double *acc, double *mag) const {
        int32_t r = row - lag;
        while (r < 0) r += window;
        Big va;
        Small vm;
        row_load<0>(row_rsrc(a + (uint64_t)r * row_big, row_big), off_big, 0, va);
        row_load<0>(row_rsrc(m + (uint64_t)r * row_small, row_small), off_small, 0, vm);
        acc[0] = va.x; acc[1] = va.y; acc[2] = va.z;
        mag[0] = va.w; mag[1] = vm.x; mag[2] = vm.y;
    }
};

// |X|^2 of the state entering a launch.  After any record the state is unit (X /= |X|,
// ExtendedKalmanFilter.py:79, or X = z from the normalised RK4 step) to within ~40 ulp of the
// one-Newton-step rsqrt, and that is snapped to exactly 1: the stream kernel carries n2 = 1 as a
// constant after a launch's first record, and every launch shape (n records at once, one record
// per launch, the handle's per-record update) rounds identically.  A state that is not unit (a
// user's set_state) keeps its |X|^2, which the reference's Jb and RK4 use (:60-62).
// The snap is an error of the one-record kernels' skip record, which stores z normalised by the snapped
// |X|^2: half the window.  40 ulp of the rsqrt leave |X|^2 - 1 <= 2 * 4.2e-15 ~ 1e-14; kNormSnap is
// three times that and costs at most 1.45e-14 = 131 u, inside the 303 Y u (Y >= 1) that
// tests/test_step_halves.py holds the propagation to (at 1e-13 a set_state X of |X|^2 = 1 - 9e-14 came
// back 4.5e-14 = 405 u off: 316 Y u on the float32 set, whose Y is 1.27, 1.04 times the bound; the float64
// set, Y = 1.81, still passed).  2.9e-14 and not the 2^-45 beside it: a constant with both
// words set, as 1e-13 was, leaves every kernel's instruction sequence what it was (a zero low word
// changed the register allocation and the schedule of k_run and k_live).
constexpr double kNormSnap = 2.9e-14;
__device__ __forceinline__ double state_norm2(const double *x) {
    const double n2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3];
    return fabs(n2 - 1.0) < kNormSnap ? 1.0 : n2;
}

// a * b - c as one three-address v_fma_f64 with a negated operand.  Left to itself the compiler
// picks the accumulating v_fmac_f64 for e = v sc - z and sets -z up in the accumulator registers
// ahead of the rare Wahba fallback branch (a negation and two register copies per component).
__device__ __forceinline__ double fma_sub(double a, double b, double c) {
    double d;
    asm("v_fma_f64 %0, %1, %2, -%3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// c - a * b, likewise
__device__ __forceinline__ double fma_rsub(double a, double b, double c) {
    double d;
    asm("v_fma_f64 %0, -%1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

// The two forms of a record step (ekf_record_step below), as the LOOP argument of everything here
constexpr bool kPlainForm = false, kLoopForm = true;

// Per-launch constants of the FP64 ekf_record_step.  Plain form (LOOP = false): the covariance is
// carried as P itself; loop form (LOOP = true): as N with P = rI + beta D N D, beta = sqrt(2) r,
// D = diag(1, 1, -1, -1), so that the next N = -D (S^)^-1 D comes out of the Schur inverse of
// innovation_cov_n's S^ with no update arithmetic (pekf_math.hpp).
struct StepK {
    double g2, r2;  // plain: 2g, 2r (innovation_cov2) | loop: 2g/beta, 2r/beta (innovation_cov_n)
    double rp, rr;  // plain: r, 2r^2 (P = rI - 2r^2 (2S)^-1) | loop: r2 / 2 (innovation_cov_n's rbh), unused
    double sy;      // Y's weight in the unnormalised X update: plain 1/(2r), loop 1/sqrt(2)
};
// ... and of the mixed-precision step (the f32 ekf_record_step below), which carries P in both forms
struct StepKMixed {
    double g2, ir;  // 2g, 1 / r
    float r2, rp;   // 2r, r
};
template <bool MIXED, bool LOOP>
__device__ __forceinline__ auto step_consts(double qs, double rs) {
    if constexpr (MIXED) {
        return StepKMixed{0.5 * qs, 1.0 / rs, (float)(2.0 * rs), (float)rs};
    } else {
        const double g = 0.25 * qs;  // Jb Q Jb^T = (q/4)(|X|^2 I - X X^T)
        if constexpr (LOOP) {
            const double ib = 1.0 / (kSqrt2 * rs);
            return StepK{2.0 * g * ib, 2.0 * rs * ib, rs * ib, 0.0, 1.0 / kSqrt2};
        } else {
            return StepK{2.0 * g, 2.0 * rs, rs, 2.0 * (rs * rs), 0.5 / rs};
        }
    }
}

// Where the loop-form kernels (k_run, k_live) take Q = qI and R = rI from: a pair of kernel arguments, NoiseQ and
// NoiseR.  Launch-wide (NOISE = false): the two doubles q and r.  Per filter (the kernels' NOISE form): a plane
// double2 [batch] of {q, r} in device memory, 16-byte aligned, and nothing -- each lane reads its own entry once,
// before the record loop, and everything derived from it (step_consts, the r of enter_ref_basis and
// from_ref_basis) is the lane's own, written by the same expressions in the same order: a lane whose entry is
// (q, r) rounds exactly as the launch-wide form with that q and r.  The fused algebra needs Q = qI and R = rI
// per filter, not the same q and r in every lane.  (Two arguments in both forms, so that the launch-wide
// kernels' argument block, and with it their code, is what it was.)
struct NoNoiseArg {};
template <bool NOISE>
using NoiseQ = std::conditional_t<NOISE, const double2 *, double>;
template <bool NOISE>
using NoiseR = std::conditional_t<NOISE, NoNoiseArg, double>;
// The precondition of a plane entry is r finite and > 0 (S = P- + rI must be SPD), q finite and >= 0, which no
// host check can see in device memory: a lane whose entry breaks it takes NaN for both, so its own X and P
// become NaN and nothing else happens (no index or trip count anywhere depends on these values).
__device__ __forceinline__ void lane_noise(double q, double r, int64_t, double &qs, double &rs) {
    qs = q;
    rs = r;
}
__device__ __forceinline__ void lane_noise(const double2 *plane, NoNoiseArg, int64_t b, double &qs, double &rs) {
    const double2 v = plane[b];
    const bool ok = v.y > 0.0 && v.y < __builtin_inf() && v.x >= 0.0 && v.x < __builtin_inf();
    qs = ok ? v.x : __builtin_nan("");
    rs = ok ? v.y : __builtin_nan("");
}
// The lane's r again at a launch's end (from_ref_basis): re-read, not held through the record loop, where the
// per-filter form then keeps three doubles of StepK (g2, r2, rp) and no more.  (volatile: a load the compiler
// may not merge with lane_noise's.)
__device__ __forceinline__ double lane_r_again(double, int64_t, double rs) { return rs; }
__device__ __forceinline__ double lane_r_again(const double2 *plane, int64_t b, double) {
    const double r = *reinterpret_cast<const volatile double *>(&plane[b].y);
    return r > 0.0 && r < __builtin_inf() ? r : __builtin_nan("");
}

// Wahba-skip: no Correction for this record (X = z, P = P- = S - rI)
template <bool LOOP>
__device__ __forceinline__ void record_skip(double *x, const double *z, Sym4 &P, const Sym4 &S2, const StepK &k) {
    x[0] = z[0]; x[1] = z[1]; x[2] = z[2]; x[3] = z[3];
    const double hf = 0.5;
    if (LOOP)  // D N D = (S - 2r I) / beta = S^/2 - rb I
        P = {fma(hf, S2.a00, -k.r2), hf * S2.a01, -hf * S2.a02, -hf * S2.a03, fma(hf, S2.a11, -k.r2),
             -hf * S2.a12, -hf * S2.a13, fma(hf, S2.a22, -k.r2), hf * S2.a23, fma(hf, S2.a33, -k.r2)};
    else
        P = {fma(hf, S2.a00, -k.rp), hf * S2.a01, hf * S2.a02, hf * S2.a03, fma(hf, S2.a11, -k.rp),
             hf * S2.a12, hf * S2.a13, fma(hf, S2.a22, -k.rp), hf * S2.a23, fma(hf, S2.a33, -k.rp)};
}

// ---- Correction (ExtendedKalmanFilter.py:70-80) from S^-1 (Si) and Wahba's Y = v sc ----
template <bool LOOP>
__device__ __forceinline__ void record_correct(double *x, const double *z, Sym4 &P, const Sym4 &Si, const double *v,
                                               double sc, const StepK &k) {
    // e = Y - z (loop form: D e, whose last two components are z - Y)
    const double e0 = fma_sub(v[0], sc, z[0]), e1 = fma_sub(v[1], sc, z[1]);
    const double e2 = LOOP ? fma_rsub(v[2], sc, z[2]) : fma_sub(v[2], sc, z[2]);
    const double e3 = LOOP ? fma_rsub(v[3], sc, z[3]) : fma_sub(v[3], sc, z[3]);
    // X = z + K e = Y - r S^-1 e (:77), normalised (:79): X ~ Y / (2r) - S^-1 e / 2, or (loop form,
    // S^-1 = -(2/beta) D Si D) X ~ Y / sqrt(2) + D Si D e, left unnormalised
    const double u0 = Si.a00 * e0 + Si.a01 * e1 + Si.a02 * e2 + Si.a03 * e3;
    const double u1 = Si.a01 * e0 + Si.a11 * e1 + Si.a12 * e2 + Si.a13 * e3;
    const double u2 = Si.a02 * e0 + Si.a12 * e1 + Si.a22 * e2 + Si.a23 * e3;
    const double u3 = Si.a03 * e0 + Si.a13 * e1 + Si.a23 * e2 + Si.a33 * e3;
    const double sr = sc * k.sy;
    const double x0 = fma(v[0], sr, LOOP ? u0 : -u0), x1 = fma(v[1], sr, LOOP ? u1 : -u1);
    const double x2 = fma(v[2], sr, -u2), x3 = fma(v[3], sr, -u3);
    if (LOOP) {
        x[0] = x0; x[1] = x1; x[2] = x2; x[3] = x3;
    } else {
        const double in = rsqrt<true>(x0 * x0 + x1 * x1 + x2 * x2 + x3 * x3);
        x[0] = x0 * in; x[1] = x1 * in; x[2] = x2 * in; x[3] = x3 * in;
    }
    // P = P- - K P- = r K = r I - r^2 S^-1 = r I - (2 r^2) Si (:78)
    if (LOOP) {
        P = Si;  // P = rI + beta D N D: nothing to compute
    } else {
        const double rp = k.rp, rr = k.rr;
        P = {rp - rr * Si.a00, -rr * Si.a01, -rr * Si.a02, -rr * Si.a03, rp - rr * Si.a11,
             -rr * Si.a12, -rr * Si.a13, rp - rr * Si.a22, -rr * Si.a23, rp - rr * Si.a33};
    }
}

// One record of main_file.py:42-45 -- Prediction(gyro, T) then Correction(mag, acc) -- on the
// lane's state (x, P) in registers, all in FP64; n2 = state_norm2 of x (1 for every record after a
// launch's first).  gy = the gyro sample, dt_ns = T - previousT, missing: the record has no magnetometer
// sample (record_skip).  reload(acc, mag) re-reads the record's samples for the rare degenerate-Wahba
// fallback; it is not called on the common path.  The step has two forms; the kernels that run the same
// form share this code and give bit-identical results for the same inputs:
//
//            basis (Wf)                covariance  X after the record  halvings       rsqrt  callers
//   plain    world (Frame)             P           normalised          multiplies     1      k_run_one, k_update
//   loop     reference frame's (RefW,  N (StepK)   unnormalised        omod (inside   2      k_run (FP64), k_live
//            RefWLazy; pekf_math.hpp)                                  OmodMode)
//
// Plain (LOOP = false), for the one-record launches, whose state comes from HBM and returns there every
// record: the measurement is the matrix chain of wahba_quat_toward(const Frame &, ..).
// Loop (LOOP = true), for the kernels that keep a filter in registers over many records, between
// enter_ref_basis and from_ref_basis:
//  - In the reference frame's basis the measurement is Wahba's quaternion as a product of two plane
//    rotations (wahba_product_ref: the measured plane's normal to z, then the best turn about z), scaled
//    and flipped toward z by wahba_toward_from_product.
//  - The covariance is carried as N (StepK), and X is left unnormalised, X = x / |x| with |x| ~ 0.7:
//    its norm folds into the next record's RK4 normalisation (z = rk4(x) / |rk4(x)| whatever |x|) and
//    Jb term (g (|X|^2 I - X X^T) = g I - (g / |x|^2) x x^T, |X|^2 = 1 as state_norm2 snaps it), and
//    1/|x|^2 = in^2 kk comes from RK4's own rsqrt: 8 operations instead of the 13 of normalising X.
//  - The exact halvings fold into the instructions that form the products (omod, pekf_math.hpp) -- the
//    gyro is never scaled to h = w/2, and the Newton steps of the rsqrt seeds need no separate multiply
//    by 1/2: 9 VALU fewer per record, the same values bit for bit.  The caller opens the OmodMode.
// The loop form's options:
// LAZY: x arrives unnormalised (n2 ignored), as every record after a launch's first finds it; the
// caller normalises once at the end of the launch.
// PIN: S^-1 depends only on the Prediction; it is held ahead of the rare fallback branch, in the basic
// block of the Wahba chain, so that the two independent chains interleave (left to itself the compiler
// sinks it past the branch, behind the Wahba chain).  Worth it where a SIMD has one wave and the
// record's dependency chain is exposed (config 2: -2.3 %); neutral at 3 waves per SIMD (config 3),
// where the other waves fill those gaps anyway (profiles/r2/ab_pin_schur/).
// HOIST: the Correction's state-independent half -- S^-1 and Wahba's unnormalised quaternion q' -- is
// formed ahead of the missing-magnetometer branch, in the Prediction's basic block (held there by an
// empty asm), so one block carries two independent dependency chains (the Prediction's and the
// record's own); only q'.z, its scale and flip and the update stay behind the branch.  For launches of
// at most one wave per SIMD (config 2), where nothing else fills the chain's stalls (launch_run_multi
// selects it).
// PIN and HOIST move instructions only: the arithmetic is the same, bit for bit.
template <bool LOOP, bool LAZY = false, bool PIN = false, bool HOIST = false, typename Ref, typename Reload>
__device__ __forceinline__ void ekf_record_step(double *x, double n2, Sym4 &P, const Ref &Wf, const StepK &k,
                                                const double *gy, double dt_ns, bool missing,
                                                const double *acc, const double *mag, const Reload &reload) {
    static_assert(LOOP || !(LAZY || PIN || HOIST), "LAZY, PIN and HOIST are options of the loop form");
    static_assert(LOOP != std::is_same<Ref, Frame>::value, "plain form: world basis; loop form: the reference frame's");
    constexpr int F = LOOP ? 2 : 1;  // rsqrt form
    // ---- Prediction (ExtendedKalmanFilter.py:58-68) ----
    double z[4];
    Sym4 S2;
    if constexpr (LOOP) {
        const double n2x = LAZY ? x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3] : n2;
        double kk, irk;
        // th2x2 = 2 |h|^2 = |w|^2 / 2 (0.5*Omega(w) = Omega(h), h = w/2)
        const double th2x2 = fma_half(gy[2], gy[2], fma(gy[1], gy[1], gy[0] * gy[0]));
        rk4_closed_w(x, n2x, dt_ns, gy, th2x2, z, kk, irk);                  // (:62)
        const double g2x = LAZY ? ((irk * irk) * kk) * k.g2 : k.g2;           // 2g / |x|^2
        S2 = innovation_cov_n(P, gy, th2x2, x, LAZY ? 1.0 : n2, k.g2, k.r2, k.rp, g2x);
    } else {
        const double hw[3] = {0.5 * gy[0], 0.5 * gy[1], 0.5 * gy[2]};  // 0.5*Omega(w) = Omega(w/2)
        const double th2 = hw[0] * hw[0] + hw[1] * hw[1] + hw[2] * hw[2];
        rk4_closed(x, n2, dt_ns, hw, th2, z);                              // (:62)
        // S2 = 2S, S = P- + rI with P- = A P A^T + Jb Q Jb^T, Jb from the prior X (:60-61, :63).
        // Exactly twice S (see innovation_cov2), so every result below is bit-identical to the
        // undoubled recursion: (2S)^-1 = S^-1/2, and the constants absorb the factor.
        S2 = innovation_cov2(P, hw, gy, th2, x, n2, k.g2, k.r2, k.g2);
    }

    if constexpr (HOIST) {
        const Sym4 Si = spd_inverse_schur<LOOP>(S2);
        const double ka = fabs(acc[2]);              // (:71)
        double qm[4];
        wahba_product_ref<F>(Wf, acc, mag, ka, qm);
        asm volatile("" ::"v"(Si.a00), "v"(Si.a01), "v"(Si.a02), "v"(Si.a03), "v"(Si.a11), "v"(Si.a12),
                     "v"(Si.a13), "v"(Si.a22), "v"(Si.a23), "v"(Si.a33), "v"(qm[0]), "v"(qm[1]), "v"(qm[2]),
                     "v"(qm[3]));
        if (missing) {
            record_skip<LOOP>(x, z, P, S2, k);
        } else {
            double v[4], sc;
            wahba_toward_from_product<F>(Wf, qm, ka, z, v, sc, reload);  // Wahba.py:8-47 + the flip of :73-75
            record_correct<LOOP>(x, z, P, Si, v, sc, k);
        }
        return;
    }
    if (missing) {
        record_skip<LOOP>(x, z, P, S2, k);
    } else {
        // K = P- S^-1 = I - r S^-1  (:64-66); Si = S^-1 / 2, or (loop form) the next N = -D (S^)^-1 D
        const Sym4 Si = spd_inverse_schur<LOOP>(S2);
        const double ka = fabs(acc[2]);              // (:71)
        double v[4], sc;
        auto pin = [&] {
            if constexpr (PIN)
                asm volatile("" ::"v"(Si.a00), "v"(Si.a01), "v"(Si.a02), "v"(Si.a03), "v"(Si.a11), "v"(Si.a12),
                             "v"(Si.a13), "v"(Si.a22), "v"(Si.a23), "v"(Si.a33));
        };
        // Wahba.py:8-47 + the flip of :73-75: Y = v sc
        wahba_quat_toward<F>(Wf, acc, mag, ka, 1.0 - ka, z, v, sc, reload, pin);
        record_correct<LOOP>(x, z, P, Si, v, sc, k);
    }
}

// ---- The same record with the covariance recursion in f32 (PEKF_RUN_MIXED_PRECISION) ----
// The FP64 step's algebra adds P- to rI and takes P = rI - r^2 S^-1 and K = I - r S^-1 as differences
// from r.  In f32 that rounds the parts of P of size ~q/4 at eps32 r: a relative error ~eps32 r / q in
// P and, through K, in X (measured: DESIGN.md §4.3).  Here r enters only inside the inverse, and the
// gain and the posterior are products:
//   2P- = innovation_cov2 with no r term,  S^-1 / 2 = (2P- + 2rI)^-1,  P = r K = r (2P-)(S^-1 / 2),
//   X = z + K e = z + P e / r,
// so every rounding is relative to the quantity it rounds.  2P- is formed in FP64 from the f32 P and
// rounded once: innovation_cov2's trace-butterfly form cancels (for P ~ cI it is 4|h|^2 c - 2|h|^2 c),
// its f32 roundings are common to the whole diagonal, and where the gyro term dominates (P+ ~ |h|^2 P)
// the relative error of P is never forgotten and adds up record after record.  S, its
// inverse and the product P- S^-1 are f32.  The covariance is carried as P in every launch shape (in the
// multi-record loop in the reference frame's basis).  P e is formed in FP64 from the f32 P, e = Y - z
// stays FP64, and RK4, Wahba and the normalisation are the FP64 step's.
// It is ekf_record_step's overload for an f32 covariance and a StepKMixed, so a kernel writes one call
// for either precision.  LOOP and LAZY are the FP64 step's: LOOP = false normalises X every record;
// LOOP = true (the multi-record loop, in the reference frame's basis) leaves X = z + K e unnormalised.
// No omod, so rsqrt form 1 in both.  It has none of the FP64 loop's schedules: PIN and HOIST are named
// only so that k_run can hand its own flags to either overload, and must be false.
template <bool LOOP, bool LAZY = false, bool PIN = false, bool HOIST = false, typename Ref, typename Reload>
__device__ __forceinline__ void ekf_record_step(double *x, double n2, Sym4T<float> &P, const Ref &Wf,
                                                const StepKMixed &k, const double *gy, double dt_ns, bool missing,
                                                const double *acc, const double *mag, const Reload &reload) {
    static_assert(LOOP || !LAZY, "LAZY is an option of the loop form");
    static_assert(!PIN && !HOIST, "PIN and HOIST are schedules of the FP64 loop form");
    // ---- Prediction (ExtendedKalmanFilter.py:58-68) ----
    const double n2x = LAZY ? x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3] : n2;
    const double hw[3] = {0.5 * gy[0], 0.5 * gy[1], 0.5 * gy[2]};  // 0.5*Omega(w) = Omega(w/2)
    const double th2 = hw[0] * hw[0] + hw[1] * hw[1] + hw[2] * hw[2];
    double z[4], kk, irk;
    rk4_closed(x, n2x, dt_ns, hw, th2, z, kk, irk);                      // (:62)
    const double g2x = LAZY ? ((irk * irk) * kk) * k.g2 : k.g2;          // 2g / |x|^2
    const Sym4 Pd = {P.a00, P.a01, P.a02, P.a03, P.a11, P.a12, P.a13, P.a22, P.a23, P.a33};
    const Sym4 Md = innovation_cov2(Pd, hw, gy, th2, x, LAZY ? 1.0 : n2, k.g2, 0.0, g2x);  // 2P- (:61)
    const Sym4T<float> M2 = {(float)Md.a00, (float)Md.a01, (float)Md.a02, (float)Md.a03, (float)Md.a11,
                             (float)Md.a12, (float)Md.a13, (float)Md.a22, (float)Md.a23, (float)Md.a33};
    if (missing) {  // Wahba-skip: X = z, P = P-
        x[0] = z[0]; x[1] = z[1]; x[2] = z[2]; x[3] = z[3];
        const float hf = 0.5f;
        P = {hf * M2.a00, hf * M2.a01, hf * M2.a02, hf * M2.a03, hf * M2.a11,
             hf * M2.a12, hf * M2.a13, hf * M2.a22, hf * M2.a23, hf * M2.a33};
        return;
    }
    Sym4T<float> S2 = M2;  // 2S = 2P- + 2rI (:63)
    S2.a00 += k.r2; S2.a11 += k.r2; S2.a22 += k.r2; S2.a33 += k.r2;
    const Sym4T<float> Si = spd_inverse_schur(S2);                        // S^-1 / 2
    // ---- Correction (ExtendedKalmanFilter.py:70-80) ----
    const double ka = fabs(acc[2]);  // (:71)
    double v[4], sc;                 // Wahba.py:8-47 + the flip of :73-75: Y = v sc
    wahba_quat_toward<1>(Wf, acc, mag, ka, 1.0 - ka, z, v, sc, reload);
    P = sym_product_upper(M2, Si, k.rp);  // P = P- - K P- = r K (:66, :78)
    const double e0 = fma_sub(v[0], sc, z[0]), e1 = fma_sub(v[1], sc, z[1]);
    const double e2 = fma_sub(v[2], sc, z[2]), e3 = fma_sub(v[3], sc, z[3]);
    const double p00 = P.a00, p01 = P.a01, p02 = P.a02, p03 = P.a03, p11 = P.a11;
    const double p12 = P.a12, p13 = P.a13, p22 = P.a22, p23 = P.a23, p33 = P.a33;
    const double u0 = p00 * e0 + p01 * e1 + p02 * e2 + p03 * e3;
    const double u1 = p01 * e0 + p11 * e1 + p12 * e2 + p13 * e3;
    const double u2 = p02 * e0 + p12 * e1 + p22 * e2 + p23 * e3;
    const double u3 = p03 * e0 + p13 * e1 + p23 * e2 + p33 * e3;
    const double x0 = fma(u0, k.ir, z[0]), x1 = fma(u1, k.ir, z[1]);      // X = z + K e (:77)
    const double x2 = fma(u2, k.ir, z[2]), x3 = fma(u3, k.ir, z[3]);
    if (!LOOP) {  // (:79)
        const double in = rsqrt<true>(x0 * x0 + x1 * x1 + x2 * x2 + x3 * x3);
        x[0] = x0 * in; x[1] = x1 * in; x[2] = x2 * in; x[3] = x3 * in;
    } else {
        x[0] = x0; x[1] = x1; x[2] = x2; x[3] = x3;
    }
}

// A multi-record launch runs the filter in its reference frame's own basis (RefW in pekf_math.hpp:
// the same filter, with Wahba's rotation 24 operations cheaper per record) with the covariance
// carried as N, P = rI + beta D N D (StepK); the state is rotated in once and out once per launch.
// to_ref_basis: the state entering the launch, x -> q_W^* x, P -> N of q_W^* P q_W.
template <typename PT>
__device__ __forceinline__ void to_ref_basis(const double *qw, double *x, Sym4T<PT> &P, double rs) {
    double xw[4];
    qmul_left<true>(qw, x, xw);
    x[0] = xw[0]; x[1] = xw[1]; x[2] = xw[2]; x[3] = xw[3];
    P = sym_rotate<true>(qw, P);
    if constexpr (std::is_same<PT, double>::value) {  // the mixed loop carries P itself (the f32 ekf_record_step)
        const PT ib = (PT)(1.0 / (kSqrt2 * rs)), rp = (PT)rs;
        P = {(P.a00 - rp) * ib, P.a01 * ib, -P.a02 * ib, -P.a03 * ib, (P.a11 - rp) * ib,
             -P.a12 * ib, -P.a13 * ib, (P.a22 - rp) * ib, P.a23 * ib, (P.a33 - rp) * ib};
    }
}
// The launch's prologue: the reference pair's Frame as the RefW (HOLD: q_W held through the loop, for
// trajectory output) or the RefWLazy (q_W recomputed from `pair` at the launch's end and in the rare
// fallback: 8 VGPRs fewer), and (x, P) into its basis.  idle (HOLD only): a filter with no records in
// this launch rotates by the identity, which is exact; its state is not written back.
template <bool HOLD, typename PT>
__device__ __forceinline__ std::conditional_t<HOLD, RefW, RefWLazy> enter_ref_basis(const Frame &Wf, const double *pair,
                                                                                    bool idle, double *x,
                                                                                    Sym4T<PT> &P, double rs) {
    std::conditional_t<HOLD, RefW, RefWLazy> Wr;
    Wr.aW = Wf.alpha; Wr.b1W = Wf.beta1; Wr.b2W = Wf.beta2;
    double qw[4];
    frame_quat(Wf, qw);
    if constexpr (HOLD) {
        if (idle) { qw[0] = 1.0; qw[1] = qw[2] = qw[3] = 0.0; }
        Wr.q[0] = qw[0]; Wr.q[1] = qw[1]; Wr.q[2] = qw[2]; Wr.q[3] = qw[3];
    } else {
        Wr.pair = pair;
    }
    to_ref_basis(qw, x, P, rs);
    return Wr;
}
// The loop's unnormalised reference-basis X as the world-basis unit quaternion (a trajectory row,
// the launch's final X); qw: q_W, as the caller may want it too
template <typename RW>
__device__ __forceinline__ void ref_to_world(const RW &Wr, const double *x, double *xo, double *qw) {
    const double in = rsqrt<true>(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]);
    const double xn[4] = {x[0] * in, x[1] * in, x[2] * in, x[3] * in};
    Wr.quat(qw);
    qmul_left<false>(qw, xn, xo);
}
// from_ref_basis: back at the launch's end, X normalised.
template <typename PT, typename RW>
__device__ __forceinline__ void from_ref_basis(const RW &Wr, double *x, Sym4T<PT> &P, double rs) {
    if constexpr (std::is_same<PT, double>::value) {
        const PT be = (PT)(kSqrt2 * rs), rp = (PT)rs;
        P = {fma(be, P.a00, rp), be * P.a01, -be * P.a02, -be * P.a03, fma(be, P.a11, rp),
             -be * P.a12, -be * P.a13, fma(be, P.a22, rp), be * P.a23, fma(be, P.a33, rp)};
    }
    double xo[4], qw[4];
    ref_to_world(Wr, x, xo, qw);
    x[0] = xo[0]; x[1] = xo[1]; x[2] = xo[2]; x[3] = xo[3];
    P = sym_rotate<false>(qw, P);
}

// Occupancy target of k_run in waves per SIMD (0: the compiler's choice)
#ifndef PEKF_RUN_WAVES
#define PEKF_RUN_WAVES 0
#endif
#if PEKF_RUN_WAVES
#define PEKF_RUN_ATTR __attribute__((amdgpu_waves_per_eu(PEKF_RUN_WAVES)))
#else
#define PEKF_RUN_ATTR
#endif

// The multi-record stream kernel: n_steps >= 1 records of main_file.py:42-45 per filter, one lane per
// filter, instantiated by pekf_run_multi.hip alone (one-record launches: k_run_one, pekf_run.hip).
// R: the record in the planes -- Rec (40 B: f32 samples, a u32 dt word with the missing-magnetometer
// bit) or Rec64 (80 B of doubles: dt the float64 T - previousT itself, any pause, clock step or
// fraction, no escape word; every record carries a magnetometer sample, as a log's always does).
// MIXED = false: every operation in FP64 (the headline path).
// MIXED = true (opt-in, PEKF_RUN_MIXED_PRECISION): the covariance recursion (P-, S^-1, K, P)
// in FP32 while RK4, Wahba, R->q and the X update stay FP64 (the f32 ekf_record_step).
// COUNTS: filter b applies only its first counts[b] records of the launch (a separate
// instantiation so the uniform-length path carries no per-step lane predicate).
// PIN: the Schur-inverse-first schedule of the multi-record loop (ekf_record_step, launch_run_multi).
// LONGDT (Rec): the window has a dt side plane dtx[window][batch] (float64 ns): a record whose dt word is
// PEKF_DT_ESCAPE takes its dt from there -- gaps of 2^31 ns or more, negative or fractional ones, any
// T - previousT the reference accepts (ExtendedKalmanFilter.py:62).  A separate instantiation, so the
// windows without escapes (every synthetic and front-end stream but the rare long pause) pay nothing.
// HOIST: the Correction's state-independent half ahead of the missing branch (ekf_record_step).
// NOISE: per-filter noise (NoiseQ / NoiseR above; pekf_run_noise.hip instantiates these kernels): the lane's own
// q and r in place of the launch's, FP64 on AoS state.
template <typename R, bool TRAJ, bool MIXED, bool SOA, bool COUNTS, bool PIN = false, bool LONGDT = false,
          bool HOIST = false, bool NOISE = false>
__global__ __launch_bounds__(kRunBlock) PEKF_RUN_ATTR void k_run(int64_t batch, int64_t n_steps, int64_t window,
                                                   int64_t step0, const decltype(R::gd) *__restrict__ gd,
                                                   const decltype(R::gd) *__restrict__ am,
                                                   const decltype(R::my) *__restrict__ my,
                                                   const double *__restrict__ refs,
                                                   double *__restrict__ Xio, double *__restrict__ Pio,
                                                   NoiseQ<NOISE> q_arg, NoiseR<NOISE> r_arg,
                                                   double *__restrict__ traj,
                                                   const int32_t *__restrict__ counts,
                                                   const double *__restrict__ dtx) {
    using PT = typename std::conditional<MIXED, float, double>::type;
    constexpr bool kRec64 = std::is_same<R, Rec64>::value;
    static_assert(!(kRec64 && LONGDT), "an FP64 record's dt is the float64 itself: no side plane");
    static_assert(!NOISE || !(MIXED || SOA || HOIST), "per-filter noise: FP64, AoS state, no HOIST");
    const int64_t b = (int64_t)blockIdx.x * kRunBlock + threadIdx.x;
    if (b >= batch) return;
    double qs, rs;
    lane_noise(q_arg, r_arg, b, qs, rs);
    const int32_t my_steps = COUNTS ? (counts[b] < n_steps ? counts[b] : (int32_t)n_steps) : (int32_t)n_steps;

    // per-filter constants: the Wahba reference frame of (acc0, mag0) (Wahba.py:4-6)
    Frame Wf;
    {
        const double a0[3] = {refs[6 * b + 0], refs[6 * b + 1], refs[6 * b + 2]};
        const double m0[3] = {refs[6 * b + 3], refs[6 * b + 4], refs[6 * b + 5]};
        make_frame<true>(a0, m0, Wf);
    }
    double x[4];
    Sym4T<PT> P;
    load_state<SOA>(Xio, Pio, b, batch, x, P);

    // Record of stream row r: raw buffer loads whose lane offset is fixed and whose row offset is
    // the wave-uniform soffset within a chunk of rows (RowCursor), so a record costs two scalar adds
    // and a compare of address work, no per-step vector address arithmetic.
    const uint32_t lane = (uint32_t)b;
    RowCursor<R> rows(gd, am, my, batch, window, lane);
    // rows the cursor runs ahead of the record a step works on (ping-pong: one; deeper prefetch rings
    // were measured and not kept, profiles/r1/README.md)
    constexpr int32_t kLag = 1;
    rows.start((int32_t)(step0 % window));
    R ra = rows.load(), rb;
    // Without trajectory output q_W is recomputed where it is needed rather than held through the loop
    const auto Wr = enter_ref_basis<TRAJ>(Wf, refs + 6 * b, COUNTS && my_steps == 0, x, P, rs);
    // One record: Prediction + Correction (main_file.py:42-45) on (x, P) in registers, in the
    // reference basis with the covariance as N; lazy: X arrives unnormalised (every record after the
    // launch's first)
    auto step = [&](const R &cur, int32_t t, double n2, auto lazy) {
        if (!COUNTS || t < my_steps) {
            const double gy[3] = {cur.gd.x, cur.gd.y, cur.gd.z};
            const double acc[3] = {cur.am.x, cur.am.y, cur.am.z};
            const double mag[3] = {cur.am.w, cur.my.x, cur.my.y};
            double dtn;
            bool missing = false;
            if constexpr (kRec64) {
                dtn = cur.gd.w;
            } else {
                const uint32_t word = __float_as_uint(cur.gd.w);
                dtn = (double)(word & PEKF_DT_MASK);
                if constexpr (LONGDT) {  // the escaped record's row, (step0 + t) % window (rare: off the fast path)
                    if ((word & PEKF_DT_MASK) == PEKF_DT_ESCAPE) dtn = dtx[((step0 + t) % window) * batch + b];
                }
                missing = (word & PEKF_MISSING_MAG_BIT) != 0;
            }
            auto reload = [&](double *a, double *m) { rows.reload(kLag, a, m); };  // rare: this record again
            ekf_record_step<kLoopForm, decltype(lazy)::value, PIN, HOIST>(
                x, n2, P, Wr, step_consts<MIXED, kLoopForm>(qs, rs), gy, dtn, missing, acc, mag, reload);
        }
        if (TRAJ) {
            // a filter with no records in this launch (COUNTS) repeats its stored X unchanged
            // (x was rotated by the identity, which is exact; it is not normalised or written back)
            double xo[4] = {x[0], x[1], x[2], x[3]}, qw[4];
            if (!COUNTS || my_steps > 0) ref_to_world(Wr, x, xo, qw);
            double2 *o = reinterpret_cast<double2 *>(traj + (int64_t)t * batch * 4) + 2 * (int64_t)lane;
            o[0] = make_double2(xo[0], xo[1]);
            o[1] = make_double2(xo[2], xo[3]);
        }
    };
    using eager = std::false_type;
    using lazy = std::true_type;

    // Time loop, unrolled by two with ping-pong records: the next row's record is always in
    // flight while the current one is processed, and no registers are copied between steps.
    // The prefetch is unconditional (the row wraps inside the resident window, so it is always
    // a valid address).  The launch's first record takes |X|^2 from the loaded state; from then on
    // the state is unit and n2 = 1 is a compile-time constant (see state_norm2).  32-bit step counter
    // (n_steps < 2^31 is checked on the host).
    const int32_t n32 = (int32_t)n_steps;
    rows.advance();
    rb = rows.load();
    // the FP64 loop folds its exact halvings into output modifiers, which need this MODE
    OmodMode mode;
    if constexpr (!MIXED) mode.enter();
    step(ra, 0, state_norm2(x), eager{});
    for (int32_t t = 1; t < n32;) {
        rows.advance();
        ra = rows.load();
        step(rb, t, 1.0, lazy{});
        if (++t == n32) break;
        rows.advance();
        rb = rows.load();
        step(ra, t, 1.0, lazy{});
        ++t;
    }
    if constexpr (!MIXED) mode.leave();
    if (COUNTS && my_steps == 0) return;
    from_ref_basis(Wr, x, P, lane_r_again(q_arg, b, rs));
    store_state<SOA>(Xio, Pio, b, batch, x, P);
}

}  // namespace pekf
