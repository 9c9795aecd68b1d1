// pekf_percall.hip -- per-call operators behind the drop-in Python API (one thread per item).
//
// These keep the reference's dense formulation (ExtendedKalmanFilter.py, Wahba.py) so
// each call matches NumPy to rounding; the fused time-loop kernel is pekf_run.hip.  Each fixed-width
// operator is one entry of the operator table below: its operand widths, its status mapping, its kernel
// name and its lane-private body.  The batched kernel k_op<Op>, the n = 1 routes (k_call1<Op>, the
// resident service) and the host entry points all read the operand layout from that entry.  The batched
// kernel moves the per-item operands through WaveTile (pekf_tile.hpp): coalesced block reads and writes,
// transposed through LDS; the bodies work on per-lane copies.
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "pekf_internal.hpp"
#include "pekf_math.hpp"
#include "pekf_tile.hpp"

namespace pekf {

constexpr int kBlock = 256;

__device__ __forceinline__ void d_norm(int64_t i, int64_t len, const double *a,
                                                double *out) {
    double s = 0.0;
    for (int64_t k = 0; k < len; ++k) s += a[i * len + k] * a[i * len + k];
    out[i] = sqrt(s);
}

// written out: len is a run-time width, so norm is no table entry and has no n = 1 route
__global__ __launch_bounds__(kBlock) void k_norm(int64_t n, int64_t len, const double *a,
                                                double *out, Done done) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) d_norm(i, len, a, out);
    done.signal();  // the whole block reaches this point (no early return)
}

// ---------------------------------------------------------------------------------------------
// The operator table.  An entry states
//   In, Out   doubles per item of each input and output, in ABI order (Widths<>, pekf_internal.hpp:
//             offsets, totals and the widest operand follow from them);
//   kErr/kMsg the error a non-zero status maps to (PEKF_OK: the operator has no status plane);
//   kName     the batched kernel's name in launch errors;
//   body      the operator on one item: a pointer per input (lane-private) and per output, then a sink
//             and the status word.  The body tells the sink that output k is complete with
//             done.template put<k>() as soon as it is -- a tile store in k_op, nothing in the n = 1 routes,
//             whose output pointers are the destination -- so that a wide result does not stay live across
//             the work that follows it.

struct OpRk4 {
    using In = Widths<4, 1, 3>;  // q0, dt, w
    using Out = Widths<4>;
    static constexpr int kErr = PEKF_OK;
    static constexpr const char *kMsg = nullptr, *kName = "k_rk4";
    template <class S>
    __device__ __forceinline__ static void body(const double *q0, const double *dt, const double *w, double *q,
                                                const S &done, int32_t *) {
        rk4_literal(q0, dt[0], w, q);
        done.template put<0>();
    }
};

struct OpJacA {
    using In = Widths<3>;  // w
    using Out = Widths<16>;
    static constexpr int kErr = PEKF_OK;
    static constexpr const char *kMsg = nullptr, *kName = "k_jac_a";
    template <class S>
    __device__ __forceinline__ static void body(const double *w, double *A, const S &done, int32_t *) {
        omega_half(w, A);
        done.template put<0>();
    }
};

struct OpJacB {
    using In = Widths<4>;  // q
    using Out = Widths<12>;
    static constexpr int kErr = PEKF_OK;
    static constexpr const char *kMsg = nullptr, *kName = "k_jac_b";
    template <class S>
    __device__ __forceinline__ static void body(const double *q, double *J, const S &done, int32_t *) {
        xi_half(q, J);
        done.template put<0>();
    }
};

// conj(q1) (x) q2 as the reference's 4x4 left-multiplication (ExtendedKalmanFilter.py:16-23)
struct OpComparator {
    using In = Widths<4, 4>;  // q1, q2
    using Out = Widths<4>;
    static constexpr int kErr = PEKF_OK;
    static constexpr const char *kMsg = nullptr, *kName = "k_comparator";
    template <class S>
    __device__ __forceinline__ static void body(const double *a, const double *b, double *q, const S &done,
                                                int32_t *) {
        const double c0 = a[0], c1 = -a[1], c2 = -a[2], c3 = -a[3];
        const double L[16] = {c0, -c1, -c2, -c3, c1, c0, -c3, c2, c2, c3, c0, -c1, c3, -c2, c1, c0};
        matmul<4, 4, 1>(L, b, q);
        done.template put<0>();
    }
};

// KalmanFilter.Prediction (ExtendedKalmanFilter.py:58-68), in two phases so that a batched
// kernel needs R only once P^- is formed.  Phase 1: P^- = A P A^T + Jb Q Jb^T (:59-61).
__device__ __forceinline__ void d_predict_cov(const double *gyro, const double *X, const double *P,
                                              const double *Q, double *pm) {
    double A[16], At[16], Jb[12], Jbt[12], t16[16], a16[16], t12[12], b16[16];
    omega_half(gyro, A);
    xi_half(X, Jb);
    transpose<4, 4>(A, At);
    transpose<4, 3>(Jb, Jbt);
    matmul<4, 4, 4>(A, P, t16);
    matmul<4, 4, 4>(t16, At, a16);
    matmul<4, 3, 3>(Jb, Q, t12);
    matmul<4, 3, 4>(t12, Jbt, b16);
#pragma unroll
    for (int k = 0; k < 16; ++k) pm[k] = a16[k] + b16[k];
}

// Phase 2: z = RK4 (:62), S = P^- + R, K = P^- inv(S) (:63-66); status 1 = singular S.
__device__ __forceinline__ void d_predict_gain(const double *gyro, const double *dt, const double *X,
                                               const double *pm, const double *R, double *z, double *K,
                                               int32_t *status) {
    double S[16], Si[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) S[k] = pm[k] + R[k];
    rk4_literal(X, dt[0], gyro, z);
    const bool ok = inverse4(S, Si);
    *status = ok ? 0 : 1;
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 16; ++k) K[k] = NAN;
        return;
    }
    matmul<4, 4, 4>(pm, Si, K);
}

struct OpPredict {
    using In = Widths<3, 1, 4, 16, 9, 16>;  // gyro, dt, X, P, Q, R
    using Out = Widths<4, 16, 16>;          // z, P^-, K
    static constexpr int kErr = PEKF_ERR_SINGULAR;
    static constexpr const char *kMsg = "Singular matrix", *kName = "k_predict";
    template <class S>
    __device__ __forceinline__ static void body(const double *gyro, const double *dt, const double *X,
                                                const double *P, const double *Q, const double *R, double *z,
                                                double *Pm, double *K, const S &done, int32_t *status) {
        d_predict_cov(gyro, X, P, Q, Pm);
        done.template put<1>();  // before the gain is formed
        d_predict_gain(gyro, dt, X, Pm, R, z, K, status);
        done.template put<0>();
        done.template put<2>();
    }
};

// KalmanFilter.Correction (ExtendedKalmanFilter.py:70-80), in parts so that a batched kernel
// can form P - K P before the Wahba solve and keep only K live across it.  Phase 1: Y = Wahba(Acc, Mag, |Acc_z|,
// 1 - |Acc_z|) (:71), flipped when Y . z < 0 (:73-75); status 1 = non-finite B (SVD failure).
__device__ __forceinline__ void d_correct_measure(const double *mag, const double *acc, const double *z,
                                                  const double *acc0, const double *mag0, double *y,
                                                  int32_t *status) {
    const double ka = fabs(acc[2]);
    *status = wahba_b_finite(acc0, mag0, acc, mag, ka, 1.0 - ka) ? 0 : 1;
    double R[9];
    wahba_rotation_vectors(acc0, mag0, acc, mag, ka, 1.0 - ka, R);
    rotm_to_quat(R, y);
    const double cmp = y[0] * z[0] + y[1] * z[1] + y[2] * z[2] + y[3] * z[3];
    if (cmp < 0.0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = -y[k];
    }
}

// Phase 2: X = z + K (Y - z), X /= norm(X) (:76,78-79).
__device__ __forceinline__ void d_correct_state(const double *y, const double *z, const double *K, double *X) {
    double e[4], ke[4], x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = y[k] - z[k];
    matmul<4, 4, 1>(K, e, ke);
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = z[k] + ke[k];
    const double nrm = loop_norm4(x);
#pragma unroll
    for (int k = 0; k < 4; ++k) X[k] = x[k] / nrm;
}

// P = P - K P (:77): independent of the measurement.
__device__ __forceinline__ void d_correct_cov(const double *P, const double *K, double *Pout) {
    double kp[16];
    matmul<4, 4, 4>(K, P, kp);
#pragma unroll
    for (int k = 0; k < 16; ++k) Pout[k] = P[k] - kp[k];
}

struct OpCorrect {
    using In = Widths<3, 3, 4, 16, 16, 3, 3>;  // mag, acc, z, P, K, acc0, mag0
    using Out = Widths<4, 16>;                 // X, P
    static constexpr int kErr = PEKF_ERR_SVD;
    static constexpr const char *kMsg = "SVD did not converge", *kName = "k_correct";
    template <class S>
    __device__ __forceinline__ static void body(const double *mag, const double *acc, const double *z,
                                                const double *P, const double *K, const double *acc0,
                                                const double *mag0, double *X, double *Pout, const S &done,
                                                int32_t *status) {
        double y[4];
        d_correct_cov(P, K, Pout);
        done.template put<1>();  // first: only K stays live across the Wahba solve
        d_correct_measure(mag, acc, z, acc0, mag0, y, status);
        d_correct_state(y, z, K, X);
        done.template put<0>();
    }
};

// Wahba's rotation from two vector pairs, as a quaternion or as the matrix; status 1 = non-finite B
template <bool QUAT>
struct OpWahba {
    using In = Widths<3, 3, 3, 3, 1, 1>;  // acc0, mag0, acc, mag, k_acc, k_mag
    using Out = Widths<QUAT ? 4 : 9>;
    static constexpr int kErr = PEKF_ERR_SVD;
    static constexpr const char *kMsg = "SVD did not converge", *kName = "k_wahba";
    template <class S>
    __device__ __forceinline__ static void body(const double *acc0, const double *mag0, const double *acc,
                                                const double *mag, const double *ka, const double *km,
                                                double *out, const S &done, int32_t *status) {
        double R[9];
        wahba_rotation_vectors(acc0, mag0, acc, mag, ka[0], km[0], R);
        // after the solve: formed beside it, the check's operands lengthen the solve's live ranges
        *status = wahba_b_finite(acc0, mag0, acc, mag, ka[0], km[0]) ? 0 : 1;
        if constexpr (QUAT) {
            rotm_to_quat(R, out);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) out[k] = R[k];
        }
        done.template put<0>();
    }
};

struct OpR2q {
    using In = Widths<9>;  // M
    using Out = Widths<4>;
    static constexpr int kErr = PEKF_OK;
    static constexpr const char *kMsg = nullptr, *kName = "k_r2q";
    template <class S>
    __device__ __forceinline__ static void body(const double *M, double *q, const S &done, int32_t *) {
        rotm_to_quat(M, q);
        done.template put<0>();
    }
};

template <int W>
__device__ __forceinline__ double (&span(double *p))[W] {
    return *reinterpret_cast<double(*)[W]>(p);
}

// Sinks of a body: output K, complete in an item's lane-private outputs o, goes to its plane as a tile
// store; or, where the body wrote to the destination itself, nothing is left to do
template <class Op>
struct TileSink {
    const WaveTile &t;
    double *const *plane;
    double *o;
    template <int K>
    __device__ __forceinline__ void put() const {
        t.store(plane[K], span<Op::Out::w(K)>(o + Op::Out::off(K)));
    }
};
struct InPlace {
    template <int K>
    __device__ __forceinline__ void put() const {}
};

// The batched kernel: every operand's loads are issued up front (one memory round trip per wave), then
// transposed to lanes; the body stores each output as it completes.
template <class Op, size_t... I, size_t... O>
__device__ __forceinline__ void op_tile(const WaveTile &t, const OpPtrs<Op> &p, int32_t *status,
                                        std::index_sequence<I...>, std::index_sequence<O...>) {
    using In = typename Op::In;
    double c[In::total], v[In::total], o[Op::Out::total];
    (t.gather(p.in[I], span<In::w(I)>(c + In::off(I))), ...);
    (t.to_lanes(span<In::w(I)>(c + In::off(I)), span<In::w(I)>(v + In::off(I))), ...);
    int32_t st = 0;
    Op::body(v + In::off(I)..., o + Op::Out::off(O)..., TileSink<Op>{t, p.out, o}, &st);
    if constexpr (Op::kErr != PEKF_OK)
        if (status && t.active()) status[t.first + t.lane] = st;
}

template <class Op>
__global__ __launch_bounds__(kBlock) void k_op(int64_t n, OpPtrs<Op> p, int32_t *status, Done done) {
    // LDS for the WaveTiles of a block, sized by the operator's widest operand
    constexpr int kSlice = tile_doubles<std::max(Op::In::widest, Op::Out::widest)>();
    __shared__ double pool[kBlock / kWave * kSlice];
    op_tile<Op>(WaveTile(pool, kSlice, n), p, status, std::make_index_sequence<Op::In::count>{},
                std::make_index_sequence<Op::Out::count>{});
    done.signal();  // the whole block reaches this point (no early return)
}

// n = 1 calls (what main_file.py makes, one record at a time): the inputs travel by value in the
// kernel-argument segment with the dispatch itself instead of being read over PCIe from pinned
// host memory, so the kernel starts with its operands in hand.  The body is the table's, on a
// private copy (promoted to registers after inlining).
constexpr int kBlobDoubles = 64;
struct Blob {
    double v[kBlobDoubles];
};

template <class Op, size_t... I, size_t... O>
__device__ __forceinline__ void run1(const double *v, double *o, int32_t *st, std::index_sequence<I...>,
                                     std::index_sequence<O...>) {
    Op::body(v + Op::In::off(I)..., o + Op::Out::off(O)..., InPlace{}, st);
}
template <class Op>
__device__ __forceinline__ void run1(const double *v, double *o, int32_t *st) {
    run1<Op>(v, o, st, std::make_index_sequence<Op::In::count>{}, std::make_index_sequence<Op::Out::count>{});
}

// The table itself: an operator's position is its code in a service request.
template <class... Op>
struct OpList {
    static constexpr int kMaxIn = std::max({Op::In::total...}), kMaxOut = std::max({Op::Out::total...});
    template <class T>
    static constexpr int code() {
        int k = 0, at = -1;
        ((std::is_same_v<T, Op> ? at = k++ : k++), ...);
        return at;
    }
    static constexpr int outputs(int op) {  // doubles an operator returns
        int k = 0, n = 0;
        ((op == k++ ? n = Op::Out::total : 0), ...);
        return n;
    }
    // the operator `op` on lane-private operands, its outputs at their offsets in o
    __device__ __forceinline__ static void run(int op, const double *v, double *o, int32_t *st) {
        int k = 0;
        ((op == k++ ? run1<Op>(v, o, st) : void()), ...);
    }
};
using Ops = OpList<OpPredict, OpCorrect, OpWahba<true>, OpWahba<false>, OpRk4, OpJacA, OpJacB, OpComparator, OpR2q>;
constexpr int kCallMaxOut = Ops::kMaxOut;  // the widest operator's outputs
static_assert(Ops::kMaxIn <= kBlobDoubles, "every operator's inputs fit the Blob");

template <class Op>
__global__ __launch_bounds__(64) void k_call1(Blob b, double *out, int32_t *status, Done done) {
    if (threadIdx.x == 0) {
        double v[kBlobDoubles];
#pragma unroll
        for (int k = 0; k < kBlobDoubles; ++k) v[k] = b.v[k];
        *status = 0;  // stays 0 for the operators that cannot fail
        run1<Op>(v, out, status);
    }
    done.signal();
}

// ---------------------------------------------------------------------------------------------
// Resident per-call service.  A launch per n = 1 call costs a dispatch and a completion signal
// (7.6 us round trip with an empty kernel, scripts/sync_probe.hip); a resident one-wave kernel
// polling a mailbox in coherent pinned host memory answers in ~4 us (scripts/pingpong_probe.hip).
// Mailbox (host memory, mapped):
//   request  [0, 512): 8 lines of 64 B = 7 payload doubles + a stamp word (hash32 of the line's
//            payload << 32 | op << 16 | seq16).  The host writes each line's payload, then its
//            stamp (release); the wave reads all 8 lines with one 512 B load and accepts a request
//            when the 8 stamps agree on a new sequence number AND every line's payload matches its
//            stamp's hash (the memory model does not promise a line to be read as one snapshot).
//   response [1024, ...): outputs (doubles), status, then the sequence number, written last
//            after a system-scope fence; the host polls it in its own memory.
// The kernel always ends: it exits on a stop request or after kSvcIdleMs without a request
// (measured on the constant-rate wall clock); the host restarts it on demand, so a process that
// stops calling leaves nothing running for more than kSvcIdleMs.
constexpr int kSvcLinePayload = 7;
constexpr int kSvcPayload = 8 * kSvcLinePayload;  // 56 doubles
constexpr int kSvcRespDoubles = 64;
constexpr size_t kSvcRespOff = 1024, kSvcStatusOff = kSvcRespOff + kSvcRespDoubles * 8, kSvcSeqOff = kSvcStatusOff + 64;
static_assert(Ops::kMaxIn <= kSvcPayload, "every operator's inputs fit a request");
static_assert(kCallMaxOut <= kSvcRespDoubles, "every operator's outputs fit the response area");
constexpr size_t kSvcBytes = 2048;
constexpr uint32_t kSvcStop = 0xFFFFu;
constexpr int kSvcIdleMs = 5;

// 32-bit mix of one request word and its position, XORed over a line's 7 payload words into the
// line's stamp; the same function on both sides of the mailbox (32-bit multiplies only).
__host__ __device__ inline uint32_t svc_mix(uint64_t w, uint32_t pos) {
    uint32_t h = ((uint32_t)w ^ (pos * 0x9E3779B9u)) * 0x85EBCA6Bu;
    h ^= ((uint32_t)(w >> 32) + (h >> 15)) * 0xC2B2AE35u;
    return h ^ (h >> 16);
}

// XOR over each group of 8 lanes (DPP: quad_perm [1,0,3,2], [2,3,0,1], then row_half_mirror).
__device__ inline uint32_t xor8(uint32_t h) {
    h ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)h, 0xB1, 0xF, 0xF, false);
    h ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)h, 0x4E, 0xF, 0xF, false);
    h ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)h, 0x141, 0xF, 0xF, false);
    return h;
}

// The request's operation on lane 0, out of line so that the polling loop carries none of its
// hoisted constants (inlined, they were copied through AGPRs on every poll).
__device__ __noinline__ void svc_run(uint32_t op, double *sh, int32_t *sh_status) {
    // the payload as the Blob of k_call1 (same operand order, same bodies)
    double v[kSvcPayload];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int j = 0; j < kSvcLinePayload; ++j) v[k * kSvcLinePayload + j] = sh[k * 8 + j];
    double o[kCallMaxOut] = {};
    int32_t st = 0;
    Ops::run((int)op, v, o, &st);
#pragma unroll
    for (int k = 0; k < kCallMaxOut; ++k) sh[k] = o[k];  // static indices: o stays in registers
    *sh_status = st;
}

// Prediction and Correction spread over the service wave's lanes.  On lane 0 alone a predict is ~620
// serial FP64 instructions (~0.9 us of a 5.2 us call, scripts/percall_latency.cpp against the bare
// round trip of scripts/pingpong_probe.hip), most of them the 4x4 products.  Here lane l < 16 forms
// entry (l / 4, l % 4) of each product with the source expression matmul<> uses for that entry (a
// dot product from s = 0.0, the same contraction), so every entry rounds as on lane 0: the answers
// stay bit-identical to the launch per call and to the batched kernels (tests/test_percall_service.py).
// The parts with no product structure -- RK4, the pivoted inverse, the Wahba solve -- run on every
// lane at once, which costs what they cost on one.  sx: LDS scratch shared through the wave.
constexpr int kSvcScratch = 112;

// v[lane] for lanes 0..3 without indexing registers by a lane-varying value
__device__ __forceinline__ double pick4(const double *v, int lane) {
    return lane == 0 ? v[0] : lane == 1 ? v[1] : lane == 2 ? v[2] : v[3];
}

__device__ __forceinline__ double dot_row_col(const double *a, int as, const double *b, int bs, int n) {
    double s = 0.0;
    for (int t = 0; t < n; ++t) s += a[t * as] * b[t * bs];  // matmul<>'s entry: s += a * b from 0.0
    return s;
}

// payload index of operand word k (8 lines of 7 doubles; sh[line * 8 + j])
__device__ __forceinline__ constexpr int svc_at(int k) { return (k / kSvcLinePayload) * 8 + k % kSvcLinePayload; }

__device__ __noinline__ void svc_predict_wave(double *sh, double *sx, int32_t *sh_status) {
    const int lane = threadIdx.x, l = lane & 15, i = l >> 2, j = l & 3;
    using In = OpPredict::In;  // gyro, dt, X, P, Q, R
    using Out = OpPredict::Out;
    double g[3], dt, x[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = sh[svc_at(In::off(0) + k)];
    dt = sh[svc_at(In::off(1))];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = sh[svc_at(In::off(2) + k)];
    double *A = sx, *Jb = sx + 16, *P = sx + 28, *Q = sx + 44, *T = sx + 53, *T12 = sx + 69, *Si = sx + 81;
    if (lane < 16) P[l] = sh[svc_at(In::off(3) + l)];
    if (lane < 9) Q[lane] = sh[svc_at(In::off(4) + lane)];
    const double R = sh[svc_at(In::off(5) + l)];
    if (lane == 0) {
        double a[16], jb[12];
        omega_half(g, a);
        xi_half(x, jb);
#pragma unroll
        for (int k = 0; k < 16; ++k) A[k] = a[k];
#pragma unroll
        for (int k = 0; k < 12; ++k) Jb[k] = jb[k];
    }
    __syncthreads();
    // d_predict_cov: t16 = A P, t12 = Jb Q (lanes 16..27), then P- = t16 A^T + t12 Jb^T
    if (lane < 16) T[l] = dot_row_col(A + 4 * i, 1, P + j, 4, 4);
    if (lane >= 16 && lane < 28) {
        const int r = (lane - 16) / 3, c = (lane - 16) % 3;
        T12[lane - 16] = dot_row_col(Jb + 3 * r, 1, Q + c, 3, 3);
    }
    __syncthreads();
    const double a16 = dot_row_col(T + 4 * i, 1, A + 4 * j, 1, 4);     // (A P) A^T: At[t][j] = A[j][t]
    const double b16 = dot_row_col(T12 + 3 * i, 1, Jb + 3 * j, 1, 3);  // (Jb Q) Jb^T
    const double pm = a16 + b16;
    // d_predict_gain: S = P- + R, z = RK4, K = P- inv(S)
    const double s = pm + R;
    __syncthreads();
    if (lane < 16) {
        T[l] = s;
        P[l] = pm;  // P is no longer needed: it holds P- from here
    }
    __syncthreads();
    double S[16], inv[16], z[4];
#pragma unroll
    for (int k = 0; k < 16; ++k) S[k] = T[k];
    rk4_literal(x, dt, g, z);
    const bool ok = inverse4(S, inv);  // inv is meaningful only when ok
    if (lane == 0 && ok) {
#pragma unroll
        for (int k = 0; k < 16; ++k) Si[k] = inv[k];
    }
    __syncthreads();
    const double kk = ok ? dot_row_col(P + 4 * i, 1, Si + j, 4, 4) : NAN;
    __syncthreads();
    // outputs: z, P^-, K
    if (lane < 4) sh[Out::off(0) + lane] = pick4(z, lane);
    if (lane < 16) {
        sh[Out::off(1) + l] = pm;
        sh[Out::off(2) + l] = kk;
    }
    if (lane == 0) *sh_status = ok ? 0 : 1;
}

__device__ __noinline__ void svc_correct_wave(double *sh, double *sx, int32_t *sh_status) {
    const int lane = threadIdx.x, l = lane & 15, i = l >> 2, j = l & 3;
    using In = OpCorrect::In;  // mag, acc, z, P, K, acc0, mag0
    using Out = OpCorrect::Out;
    double mag[3], acc[3], z[4], a0[3], m0[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mag[k] = sh[svc_at(In::off(0) + k)];
        acc[k] = sh[svc_at(In::off(1) + k)];
        a0[k] = sh[svc_at(In::off(5) + k)];
        m0[k] = sh[svc_at(In::off(6) + k)];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = sh[svc_at(In::off(2) + k)];
    double *P = sx, *K = sx + 16;
    if (lane < 16) {
        P[l] = sh[svc_at(In::off(3) + l)];
        K[l] = sh[svc_at(In::off(4) + l)];
    }
    __syncthreads();
    // d_correct_cov: P - K P, one entry per lane
    const double pout = P[l] - dot_row_col(K + 4 * i, 1, P + j, 4, 4);
    // d_correct_measure + d_correct_state on every lane (the same values on each)
    double y[4], kr[16], X[4];
    int32_t st = 0;
    d_correct_measure(mag, acc, z, a0, m0, y, &st);
#pragma unroll
    for (int k = 0; k < 16; ++k) kr[k] = K[k];
    d_correct_state(y, z, kr, X);
    __syncthreads();
    // outputs: X, P
    if (lane < 4) sh[Out::off(0) + lane] = pick4(X, lane);
    if (lane < 16) sh[Out::off(1) + l] = pout;
    if (lane == 0) *sh_status = st;
}

__global__ __launch_bounds__(64) void k_service(char *box, unsigned long long idle_ticks) {
    __shared__ double sh[64];
    __shared__ double sx[kSvcScratch];
    __shared__ int32_t sh_status;
    const int lane = threadIdx.x;
    const uint64_t *req = reinterpret_cast<const uint64_t *>(box);
    double *resp = reinterpret_cast<double *>(box + kSvcRespOff);
    int32_t *resp_status = reinterpret_cast<int32_t *>(box + kSvcStatusOff);
    uint32_t *resp_seq = reinterpret_cast<uint32_t *>(box + kSvcSeqOff);
    uint32_t done = __hip_atomic_load(resp_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    unsigned long long t0 = wall_clock64();
    for (;;) {
        const uint64_t w = __hip_atomic_load(req + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
        const uint32_t tag = __builtin_amdgcn_readlane(lo, 7);
        const uint32_t seq = tag & 0xFFFFu, op = tag >> 16;
        bool wait = seq == done || __any((lane & 7) == 7 && lo != tag);
        if (!wait) {
            // Every line's stamp carries a hash of that line's 7 payload words (svc_mix): a line
            // whose payload words predate its stamp -- the memory model does not promise a 64 B
            // line to be read as one snapshot -- fails it and is read again at the next poll.  (A
            // seqlock re-read behind an acquire fence would cost one more PCIe round trip per
            // call: measured +1.2 us.)
            const uint32_t h = xor8((lane & 7) == 7 ? 0u : svc_mix(w, (uint32_t)lane));
            wait = __any((lane & 7) == 7 && h != hi);
        }
        if (wait) {
            if (wall_clock64() - t0 > idle_ticks) break;  // uniform
            __builtin_amdgcn_s_sleep(2);
            continue;
        }
        if (op == kSvcStop) {
            if (lane == 0) __hip_atomic_store(resp_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        sh[lane] = __longlong_as_double((long long)w);
        __syncthreads();
        const int n_out = Ops::outputs((int)op);
        if (op == Ops::code<OpPredict>())
            svc_predict_wave(sh, sx, &sh_status);  // op is wave-uniform: every lane takes part
        else if (op == Ops::code<OpCorrect>())
            svc_correct_wave(sh, sx, &sh_status);
        else if (lane == 0)
            svc_run(op, sh, &sh_status);
        __syncthreads();
        if (lane < n_out) __hip_atomic_store(resp + lane, sh[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (lane == 0) __hip_atomic_store(resp_status, sh_status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __threadfence_system();
        __syncthreads();
        if (lane == 0) __hip_atomic_store(resp_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        done = seq;
        t0 = wall_clock64();
    }
}

// Host side: one service per device, shared by the process's threads (calls serialise on a mutex).
class Service {
  public:
    static std::atomic<int> &mode() {
        static std::atomic<int> m{[] {
            const char *e = std::getenv("PEKF_PERCALL");
            return e && std::strcmp(e, "launch") == 0 ? PEKF_PERCALL_LAUNCH : PEKF_PERCALL_SERVICE;
        }()};
        return m;
    }

    static Service *get() {  // nullptr: launch mode, or the service is unavailable
        if (mode().load() != PEKF_PERCALL_SERVICE) return nullptr;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
        Service &s = instances()[dev];  // instance dev serves device dev (set once, at construction)
        return s.broken_.load() ? nullptr : &s;
    }

    // One request: n_in doubles in, n_out doubles out.  Returns PEKF_OK, or an error (the caller
    // then falls back to a launch).
    int call(uint32_t op, const double *in, size_t n_in, double *out, int n_out, int32_t *status) {
        std::lock_guard<std::mutex> g(m_);
        if (int st = ensure_running()) return st;
        post(op, in, n_in);
        if (int st = await(true)) return st;
        const double *r = reinterpret_cast<const double *>(box_ + kSvcRespOff);
        std::memcpy(out, r, (size_t)n_out * sizeof(double));
        *status = *reinterpret_cast<volatile int32_t *>(box_ + kSvcStatusOff);
        last_ = std::chrono::steady_clock::now();
        return PEKF_OK;
    }

    // Stop the resident kernel (before a device-wide synchronisation, at exit).
    void quiesce() {
        std::lock_guard<std::mutex> g(m_);
        stop_locked();
    }

    static void quiesce_all();

  private:
    static constexpr int kMaxDevices = 16;
    static Service *instances() {
        static Service *per_device = [] {
            static Service all[kMaxDevices];
            for (int i = 0; i < kMaxDevices; ++i) all[i].dev_ = i;  // its wall-clock rate sets the idle limit
            return all;
        }();
        return per_device;
    }

    int ensure_running() {
        if (!box_) {
            if (hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess ||
                hipHostMalloc(reinterpret_cast<void **>(&box_), kSvcBytes, hipHostMallocMapped | hipHostMallocCoherent) !=
                    hipSuccess ||
                hipHostGetDevicePointer(reinterpret_cast<void **>(&box_dev_), box_, 0) != hipSuccess) {
                broken_ = true;
                return set_error(PEKF_ERR_HIP, "per-call service: setup failed");
            }
            std::memset(box_, 0, kSvcBytes);
            int khz = 0;
            if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev_) != hipSuccess || khz <= 0) khz = 100000;
            idle_ticks_ = (unsigned long long)khz * kSvcIdleMs;
            static std::once_flag once;
            std::call_once(once, [] { std::atexit(Service::quiesce_all); });
        }
        // past half the idle period the kernel may be about to leave: restart it deliberately
        if (running_ && std::chrono::steady_clock::now() - last_ > std::chrono::microseconds(kSvcIdleMs * 500)) stop_locked();
        if (!running_) return launch();
        return PEKF_OK;
    }

    int launch() {
        hipLaunchKernelGGL(k_service, dim3(1), dim3(64), 0, stream_, box_dev_, idle_ticks_);
        if (launched("k_service") != PEKF_OK) {  // its message is replaced below
            broken_ = true;
            return set_error(PEKF_ERR_HIP, "per-call service: launch failed");
        }
        running_ = true;
        last_ = std::chrono::steady_clock::now();
        return PEKF_OK;
    }

    void post(uint32_t op, const double *in, size_t n_in) {
        seq_ = (seq_ + 1) & 0xFFFFu;  // 16-bit sequence number: the stamp's low half is op << 16 | seq
        const uint32_t tag = (op << 16) | seq_;
        for (int k = 0; k < 8; ++k) {
            double *line = reinterpret_cast<double *>(box_ + 64 * k);
            uint32_t h = 0;
            for (int j = 0; j < kSvcLinePayload; ++j) {
                const size_t i = (size_t)k * kSvcLinePayload + j;
                line[j] = i < n_in ? in[i] : 0.0;
                uint64_t bits;
                std::memcpy(&bits, &line[j], sizeof bits);
                h ^= svc_mix(bits, (uint32_t)(8 * k + j));
            }
            __atomic_store_n(reinterpret_cast<uint64_t *>(line + 7), ((uint64_t)h << 32) | tag, __ATOMIC_RELEASE);
        }
    }

    // Wait for the answer to seq_.  If the kernel ended without answering (it reached its idle
    // limit as the request was posted), restart it: the new kernel picks the request up.
    int await(bool restart) {
        volatile uint32_t *rs = reinterpret_cast<volatile uint32_t *>(box_ + kSvcSeqOff);
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned it = 0;; ++it) {
            if (__atomic_load_n(rs, __ATOMIC_ACQUIRE) == seq_) return PEKF_OK;
            if ((it & 255u) != 255u) continue;
            const auto dt = std::chrono::steady_clock::now() - t0;
            if (dt < std::chrono::microseconds(200)) continue;
            if (hipStreamQuery(stream_) == hipSuccess) {  // the kernel has ended
                running_ = false;
                if (__atomic_load_n(rs, __ATOMIC_ACQUIRE) == seq_) return PEKF_OK;
                if (!restart) {
                    __atomic_store_n(const_cast<uint32_t *>(rs), seq_, __ATOMIC_RELEASE);
                    return PEKF_OK;
                }
                if (int st = launch()) return st;
                restart = false;  // at most one restart per request
            } else if (dt > std::chrono::seconds(2)) {
                broken_ = true;
                return set_error(PEKF_ERR_HIP, "per-call service: no answer within 2 s");
            }
        }
    }

    void stop_locked() {
        if (!running_) return;
        if (hipStreamQuery(stream_) == hipSuccess) {  // already left at its idle limit
            running_ = false;
            return;
        }
        post(kSvcStop, nullptr, 0);
        (void)await(false);
        (void)hipStreamSynchronize(stream_);
        running_ = false;
    }

    std::mutex m_;
    hipStream_t stream_ = nullptr;
    char *box_ = nullptr, *box_dev_ = nullptr;
    unsigned long long idle_ticks_ = 0;
    int dev_ = 0;
    uint32_t seq_ = 0;
    std::atomic<bool> running_{false};  // read without the lock by quiesce_all
    std::atomic<bool> broken_{false};  // read without the lock by get()
    std::chrono::steady_clock::time_point last_;
};

// only devices whose service kernel is running are touched (no context is created elsewhere)
void Service::quiesce_all() {
    Service *all = instances();
    int cur = -1;
    for (int d = 0; d < kMaxDevices; ++d) {
        if (!all[d].running_.load()) continue;
        if (cur < 0 && hipGetDevice(&cur) != hipSuccess) return;
        if (hipSetDevice(d) != hipSuccess) continue;
        all[d].quiesce();
    }
    if (cur >= 0) (void)hipSetDevice(cur);
}

void service_quiesce_all() { Service::quiesce_all(); }

#define PEKF_GRID(n) dim3(grid_for((n), kBlock)), dim3(kBlock)

// Host side of k_call1: packs the inputs (in order) into the Blob, runs the call with zero-copy
// outputs and returns them (in order) plus the status word.
template <class Op>
static int call1(const OpPtrs<Op> &a, int32_t *status) {
    using In = typename Op::In;
    using Out = typename Op::Out;
    Blob b;
    for (int k = 0; k < In::count; ++k) std::memcpy(b.v + In::off(k), a.in[k], In::w(k) * sizeof(double));
    double tmp[kBlobDoubles];
    auto deliver = [&] {
        for (int k = 0; k < Out::count; ++k) std::memcpy(a.out[k], tmp + Out::off(k), Out::w(k) * sizeof(double));
        return PEKF_OK;
    };
    // the resident service when it is available, a launch of k_call1 otherwise (same bodies)
    Service *svc = Service::get();
    if (svc && svc->call(Ops::code<Op>(), b.v, In::total, tmp, Out::total, status) == PEKF_OK) return deliver();
    Staging &s = Staging::get();
    constexpr size_t ob = Out::total * sizeof(double);
    void *out[2];
    if (int st = s.stage_in({}, {ob, sizeof(int32_t)}, nullptr, out)) return st;
    hipLaunchKernelGGL(k_call1<Op>, dim3(1), dim3(64), 0, s.stream(), b, static_cast<double *>(out[0]),
                       static_cast<int32_t *>(out[1]), s.done(1));
    if (int st = launched("k_call1")) return st;
    if (int st = s.stage_out({{tmp, ob}, {status, sizeof(int32_t)}}, out)) return st;
    return deliver();
}

// The checks of every entry point of a table operator, over exactly its operands (an empty batch passes:
// the caller returns before touching a pointer).
template <class Op>
static int op_args(int64_t n, const OpPtrs<Op> &a) {
    PEKF_CHECK_ARG(n >= 0, "n < 0");
    bool null = false;
    for (const double *p : a.in) null |= !p;
    for (const double *p : a.out) null |= !p;
    PEKF_CHECK_ARG(n == 0 || !null, "null pointer");
    return PEKF_OK;
}

// The host-pointer route: staged operands, the n = 1 route for one item, the status plane mapped to the
// operator's error.
template <class Op>
static int host_op(int64_t n, const OpPtrs<Op> &a) {
    if (int st = op_args(n, a)) return st;
    if (n == 0) return PEKF_OK;
    return staged_call<Op, kBlock, call1<Op>>(k_op<Op>, n, a);
}

// The device-pointer route: the launch alone, on the caller's stream; status may be NULL.
template <class Op>
static int dev_op(int64_t n, const OpPtrs<Op> &a, int32_t *status, void *stream) {
    if (int st = op_args(n, a)) return st;
    if (n == 0) return PEKF_OK;
    hipLaunchKernelGGL(k_op<Op>, PEKF_GRID(n), 0, as_stream(stream), n, a, status, kNoSignal);
    return launched(Op::kName);
}

}  // namespace pekf

using namespace pekf;

extern "C" {

int pekf_set_percall_mode(int mode) {
    PEKF_CHECK_ARG(mode == PEKF_PERCALL_SERVICE || mode == PEKF_PERCALL_LAUNCH, "unknown per-call mode");
    if (mode == PEKF_PERCALL_LAUNCH) service_quiesce_all();
    Service::mode().store(mode);
    return PEKF_OK;
}

int pekf_get_percall_mode(int *mode) {
    PEKF_CHECK_ARG(mode, "mode is NULL");
    *mode = Service::mode().load();
    return PEKF_OK;
}

// Every operator entry below states its pointers in ABI order; widths, checks and routes come from the table.

int pekf_rk4_dev(int64_t n, const double *q0, const double *dt_ns, const double *w, double *q_out,
                 void *stream) {
    return dev_op<OpRk4>(n, {{q0, dt_ns, w}, {q_out}}, nullptr, stream);
}

int pekf_predict_dev(int64_t n, const double *gyro, const double *dt_ns, const double *X,
                     const double *P, const double *Q, const double *R, double *z, double *Pm,
                     double *K, int32_t *status, void *stream) {
    return dev_op<OpPredict>(n, {{gyro, dt_ns, X, P, Q, R}, {z, Pm, K}}, status, stream);
}

int pekf_correct_dev(int64_t n, const double *mag, const double *acc, const double *z,
                     const double *P, const double *K, const double *acc0, const double *mag0,
                     double *X, double *P_out, void *stream) {
    return dev_op<OpCorrect>(n, {{mag, acc, z, P, K, acc0, mag0}, {X, P_out}}, nullptr, stream);
}

int pekf_rk4(int64_t n, const double *q0, const double *dt_ns, const double *w, double *q_out) {
    return host_op<OpRk4>(n, {{q0, dt_ns, w}, {q_out}});
}

// written out: k_norm takes len as well, and has no n = 1 route
int pekf_norm(int64_t n, int64_t len, const double *a, double *res) {
    PEKF_CHECK_ARG(n >= 0 && len >= 0, "negative size");
    if (n == 0) return PEKF_OK;
    PEKF_CHECK_ARG(a && res, "null pointer");
    if (int st = require_device()) return st;
    Staging &s = Staging::get();
    const size_t b = (size_t)n * sizeof(double);
    void *in[1], *out[1];
    if (int st = s.stage_in({{a, (size_t)len * b}}, {b}, in, out)) return st;
    hipLaunchKernelGGL(k_norm, PEKF_GRID(n), 0, s.stream(), n, len, static_cast<const double *>(in[0]),
                       static_cast<double *>(out[0]), s.done(grid_for(n, kBlock)));
    if (int st = launched("k_norm")) return st;
    return s.stage_out({{res, b}}, out);
}

int pekf_jacobian_a(int64_t n, const double *w, double *A) { return host_op<OpJacA>(n, {{w}, {A}}); }

int pekf_jacobian_b(int64_t n, const double *q, double *Jb) { return host_op<OpJacB>(n, {{q}, {Jb}}); }

int pekf_comparator(int64_t n, const double *q1, const double *q2, double *res) {
    return host_op<OpComparator>(n, {{q1, q2}, {res}});
}

int pekf_predict(int64_t n, const double *gyro, const double *dt_ns, const double *X,
                 const double *P, const double *Q, const double *R, double *z, double *Pm,
                 double *K) {
    return host_op<OpPredict>(n, {{gyro, dt_ns, X, P, Q, R}, {z, Pm, K}});
}

int pekf_correct(int64_t n, const double *mag, const double *acc, const double *z,
                 const double *P, const double *K, const double *acc0, const double *mag0,
                 double *X, double *P_out) {
    return host_op<OpCorrect>(n, {{mag, acc, z, P, K, acc0, mag0}, {X, P_out}});
}

int pekf_wahba_rotation(int64_t n, const double *acc0, const double *mag0, const double *acc,
                        const double *mag, const double *k_acc, const double *k_mag, double *R) {
    return host_op<OpWahba<false>>(n, {{acc0, mag0, acc, mag, k_acc, k_mag}, {R}});
}

int pekf_wahba_quaternion(int64_t n, const double *acc0, const double *mag0, const double *acc,
                          const double *mag, const double *k_acc, const double *k_mag, double *q) {
    return host_op<OpWahba<true>>(n, {{acc0, mag0, acc, mag, k_acc, k_mag}, {q}});
}

int pekf_wahba_rotation_dev(int64_t n, const double *acc0, const double *mag0, const double *acc,
                            const double *mag, const double *k_acc, const double *k_mag, double *R,
                            int32_t *status, void *stream) {
    return dev_op<OpWahba<false>>(n, {{acc0, mag0, acc, mag, k_acc, k_mag}, {R}}, status, stream);
}

int pekf_wahba_quaternion_dev(int64_t n, const double *acc0, const double *mag0, const double *acc,
                              const double *mag, const double *k_acc, const double *k_mag, double *q,
                              int32_t *status, void *stream) {
    return dev_op<OpWahba<true>>(n, {{acc0, mag0, acc, mag, k_acc, k_mag}, {q}}, status, stream);
}

int pekf_rotmat_to_quat(int64_t n, const double *M, double *q) { return host_op<OpR2q>(n, {{M}, {q}}); }

}  // extern "C"
