// pekf_side.hip -- side outputs beside the fused filter: what main_file.py
// plots next to the filter quaternion.
//   k_gyro_chain   pure-gyro attitude: the RK4 chain of the gyro record alone, same dt as the
//                  filter (KFS/KalmanFilter.cpp:149 RungeKuttaEval(Quarternion_Gyro_pure, ...),
//                  logged as "q_gyro"; the step is ExtendedKalmanFilter.py:25-41)
//   k_wahba_stream pure-Wahba attitude per record with fixed weights (main_file.py:40,
//                  Wahba.getQuarternion(acc, mag, 0.5, 0.5), Wahba.py:49-50)
//   k_rpy          UtilityFunctions.Quart2RPY (UtilityFunctions.py:3-14), degrees
// Each reads the same resident planes as pekf_run_dev (one lane per filter, coalesced).
#include "pekf_internal.hpp"
#include "pekf_math.hpp"

namespace pekf {

constexpr int kSideBlock = 256;

__device__ __forceinline__ float4 ld_nt(const float4 *p) {
    typedef float v4 __attribute__((ext_vector_type(4)));
    const v4 v = __builtin_nontemporal_load((const v4 *)p);
    return make_float4(v.x, v.y, v.z, v.w);
}
template <bool NT, typename V>
__device__ __forceinline__ V ld(const V *p) {
    if constexpr (NT)
        return ld_nt(p);
    else
        return *p;
}

// Both stream kernels run over either record type R (pekf_internal.hpp): Rec, the 40 B stream record, or
// Rec64, pekf_run_rec64_dev's planes (gd double4 {gyro xyz, dt_ns}, am double4 {acc xyz, mag x}, my double2
// {mag yz}), so a log replayed in FP64 gets its q_gyro / Wahba attitudes from the values as parsed.  The
// arithmetic is one body for both (on f32-representable values the results are bit-identical).  What
// differs per record type, each choice measured:
template <typename R>
struct SideRec;
template <>
struct SideRec<Rec> {
    // Both kernels are HBM-bound (a few dozen FP64 ops per 16-24 B record), so each lane keeps kDepth
    // records in flight (row_ring)
    static constexpr int kDepth = 8;
    // The gyro chain's record loads carry the non-temporal hint (each record is read once): 28.9 -> 26.7 ms
    // at 1M x 10,000 records; the Wahba stream's do not (+1 % with it) (profiles/r4/ntload/).
    static constexpr bool kGyroNt = true;
    // dt is the masked dt word of gd.w, or, for a word of PEKF_DT_ESCAPE in a LONGDT launch, the entry of
    // the window's dt side plane
    static constexpr bool kDtWord = true;
};
template <>
struct SideRec<Rec64> {
    static constexpr int kDepth = 4;         // shallower rings: a record is 32-48 B of registers here
    static constexpr bool kGyroNt = false;
    static constexpr bool kDtWord = false;   // dt is the float64 gd.w itself
};

// 32-bit row and step counters (window, n_steps < 2^31: checked on the host), so the wave-uniform
// tests are scalar compares.
__device__ __forceinline__ int32_t next_row(int32_t r, int32_t window) { return r + 1 == window ? 0 : r + 1; }

// The time loop of a stream kernel: one(record, t) for t = 0 .. n - 1 over the rows row0, row0 + 1, ... of
// a window of W rows (cyclic), the records in a register ring of D filled D rows ahead by load(row), the
// loop unrolled by D so every ring index is static.  The prefetch row wraps inside the resident window, so
// the loads past the last step read valid (unused) records and need no predicate.  The loop runs whole
// blocks of D records with no exit inside the unrolled body (an exit per record made the compiler copy the
// ring on the back edge, behind a wait for the loads just issued), then the last n % D records.
template <int D, typename Load, typename One>
__device__ __forceinline__ void row_ring(int32_t n, int32_t W, int32_t row0, Load &&load, One &&one) {
    decltype(load(row0)) ring[D];
    int32_t pf = row0;  // next row to prefetch
#pragma unroll
    for (int k = 0; k < D; ++k) {
        ring[k] = load(pf);
        pf = next_row(pf, W);
    }
    auto step = [&](int k, int32_t t) {
        const auto r = ring[k];
        ring[k] = load(pf);
        pf = next_row(pf, W);
        one(r, t);
    };
    const int32_t n_full = n - n % D;
    int32_t t0 = 0;
    for (; t0 < n_full; t0 += D) {
#pragma unroll
        for (int k = 0; k < D; ++k) step(k, t0 + k);
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        if (t0 + k >= n) break;  // uniform
        step(k, t0 + k);
    }
}

// a quaternion to row t of a [n_steps][batch][4] output
__device__ __forceinline__ void store_quat(double *out, int32_t t, int64_t batch, uint32_t lane, const double (&v)[4]) {
    double2 *o = reinterpret_cast<double2 *>(out + (int64_t)t * batch * 4) + 2 * (int64_t)lane;
    o[0] = make_double2(v[0], v[1]);
    o[1] = make_double2(v[2], v[3]);
}

// LONGDT (R = Rec): the window has a dt side plane dtx[window][batch] (float64 ns); a record whose dt word
// is PEKF_DT_ESCAPE takes its dt from there, exactly as the filter does (k_run<..., LONGDT>).
template <typename R, bool LONGDT>
__global__ __launch_bounds__(kSideBlock) void k_gyro_chain(int64_t batch, int64_t n_steps, int64_t window,
                                                           int64_t step0, const decltype(R::gd) *__restrict__ gd,
                                                           const double *__restrict__ dtx,
                                                           double *__restrict__ q, double *__restrict__ traj) {
    using T = SideRec<R>;
    static_assert(T::kDtWord || !LONGDT, "only a dt word escapes");
    const int64_t b = (int64_t)blockIdx.x * kSideBlock + threadIdx.x;
    if (b >= batch) return;
    const uint32_t lane = (uint32_t)b;
    double x[4] = {q[4 * b], q[4 * b + 1], q[4 * b + 2], q[4 * b + 3]};
    row_ring<T::kDepth>(
        (int32_t)n_steps, (int32_t)window, (int32_t)(step0 % window),
        [&](int32_t row) { return ld<T::kGyroNt>(gd + (int64_t)row * batch + lane); },
        [&](const auto &r, int32_t t) {
            const double hw[3] = {0.5 * (double)r.x, 0.5 * (double)r.y, 0.5 * (double)r.z};
            double dt_ns;
            if constexpr (T::kDtWord) {
                const uint32_t word = __float_as_uint(r.w) & PEKF_DT_MASK;
                dt_ns = (double)word;
                if constexpr (LONGDT) {  // off the fast path: the escaped record's row, (step0 + t) % window
                    if (word == PEKF_DT_ESCAPE) dt_ns = dtx[((step0 + t) % window) * batch + b];
                }
            } else {
                dt_ns = r.w;
            }
            // |h_w|^2 and |x|^2 with their fmas explicit: which product of a sum of squares the compiler
            // fuses is its choice and moves with the code around it; these are the ones the chain has
            // always had, so its results keep their bits
            const double th2 = __builtin_fma(hw[2], hw[2], __builtin_fma(hw[0], hw[0], hw[1] * hw[1]));
            const double n2 =
                __builtin_fma(x[3], x[3], __builtin_fma(x[2], x[2], __builtin_fma(x[1], x[1], x[0] * x[0])));
            double z[4];
            rk4_closed(x, n2, dt_ns, hw, th2, z);
            x[0] = z[0]; x[1] = z[1]; x[2] = z[2]; x[3] = z[3];
            if (traj) store_quat(traj, t, batch, lane, x);
        });
    q[4 * b] = x[0]; q[4 * b + 1] = x[1]; q[4 * b + 2] = x[2]; q[4 * b + 3] = x[3];
}

template <typename R>
__global__ __launch_bounds__(kSideBlock) void k_wahba_stream(int64_t batch, int64_t n_steps, int64_t window,
                                                             int64_t step0, const decltype(R::am) *__restrict__ am,
                                                             const decltype(R::my) *__restrict__ my,
                                                             const double *__restrict__ refs, double ka,
                                                             double km, double *__restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * kSideBlock + threadIdx.x;
    if (b >= batch) return;
    const uint32_t lane = (uint32_t)b;
    Frame Wf;
    {
        const double a0[3] = {refs[6 * b + 0], refs[6 * b + 1], refs[6 * b + 2]};
        const double m0[3] = {refs[6 * b + 3], refs[6 * b + 4], refs[6 * b + 5]};
        make_frame<true>(a0, m0, Wf);
    }
    const double sg = wahba_sign(ka, km);
    struct AccMag {
        decltype(R::am) a;
        decltype(R::my) m;
    };
    row_ring<SideRec<R>::kDepth>(
        (int32_t)n_steps, (int32_t)window, (int32_t)(step0 % window),
        [&](int32_t row) { return AccMag{(am + (int64_t)row * batch)[lane], (my + (int64_t)row * batch)[lane]}; },
        [&](const AccMag &r, int32_t t) {
            const auto &a = r.a;
            const auto &m = r.m;
            const double acc[3] = {a.x, a.y, a.z}, mag[3] = {a.w, m.x, m.y};
            Frame Vf;
            make_frame<true>(acc, mag, Vf, sg);
            double R9[9], y[4];
            wahba_rotation<true>(Wf, Vf, ka, km, R9);
            if (frame_degenerate<1>(Vf)) {  // a zero sample or acc parallel to mag: B has rank 1 (pekf_math.hpp)
                const double sa[3] = {a.x, a.y, a.z}, sm[3] = {a.w, m.x, m.y};  // from the record again
                double a0[3], m0[3];
                frame_pair(Wf, a0, m0);
                wahba_current_rank1<1>(a0, m0, sa, sm, ka, km, R9);
            }
            rotm_to_quat_fast(R9, y);  // keeps the reference's branch / sign convention
            store_quat(out, t, batch, lane, y);
        });
}

// UtilityFunctions.Quart2RPY: roll = atan2(2(q0q1+q2q3), 1-2(q1^2+q2^2)), pitch = asin(2(q0q2-q3q1)),
// yaw = atan2(2(q0q3+q1q2), 1-2(q2^2+q3^2)), times 180/pi
__device__ __forceinline__ void d_rpy(int64_t i, const double *__restrict__ q, double *__restrict__ rpy) {
#pragma clang fp contract(off)  // round like NumPy: at gimbal lock sinp may round past 1 -> NaN there too
    const double *p = q + 4 * i;
    const double sinr = 2 * (p[0] * p[1] + p[2] * p[3]);
    const double cosr = 1 - 2 * (p[1] * p[1] + p[2] * p[2]);
    const double sinp = 2 * (p[0] * p[2] - p[3] * p[1]);
    const double siny = 2 * (p[0] * p[3] + p[1] * p[2]);
    const double cosy = 1 - 2 * (p[2] * p[2] + p[3] * p[3]);
    const double k = 180.0 / 3.141592653589793;
    rpy[3 * i + 0] = atan2(sinr, cosr) * k;
    rpy[3 * i + 1] = asin(sinp) * k;
    rpy[3 * i + 2] = atan2(siny, cosy) * k;
}

// its entry in the form of the per-call operator table (pekf_percall.hip): no status plane, no n = 1 route
struct OpRpy {
    using In = Widths<4>;   // q
    using Out = Widths<3>;  // roll, pitch, yaw
    static constexpr int kErr = PEKF_OK;
    static constexpr const char *kMsg = nullptr, *kName = "k_rpy";
};

__global__ __launch_bounds__(kSideBlock) void k_rpy(int64_t n, OpPtrs<OpRpy> p, int32_t *, Done done) {
    const int64_t i = (int64_t)blockIdx.x * kSideBlock + threadIdx.x;
    if (i < n) d_rpy(i, p.in[0], p.out[0]);
    done.signal();
}

}  // namespace pekf

using namespace pekf;

// The argument checks of the four stream entry points, in their order (an empty launch passes: the caller
// returns before launching).  misaligned: null, or the message of an FP64-record entry whose plane or
// output pointers miss their alignment (the 40 B-record entries do not check any).
static int side_args(int64_t batch, int64_t n_steps, int64_t window, int64_t step0, bool pointers,
                     const char *misaligned) {
    PEKF_CHECK_ARG(batch >= 0 && n_steps >= 0, "negative size");
    if (batch == 0 || n_steps == 0) return PEKF_OK;
    PEKF_CHECK_ARG(window > 0 && step0 >= 0, "window must be > 0 and step0 >= 0");
    PEKF_CHECK_ARG(batch < ((int64_t)1 << 28), "batch must be < 2^28 filters per launch");
    PEKF_CHECK_ARG(pointers, "null pointer");
    PEKF_CHECK_ARG(!misaligned, misaligned);
    PEKF_CHECK_ARG(n_steps < ((int64_t)1 << 31) && window < ((int64_t)1 << 31), "n_steps and window must be < 2^31");
    return PEKF_OK;
}
static dim3 side_grid(int64_t batch) { return dim3(grid_for(batch, kSideBlock)); }

extern "C" {

int pekf_gyro_chain_ext_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0, const void *plane_gd,
                            const double *dt_ext, double *q_gyro, double *traj, void *stream) {
    if (int st = side_args(batch, n_steps, window, step0, plane_gd && q_gyro, nullptr)) return st;
    if (batch == 0 || n_steps == 0) return PEKF_OK;
    dispatch_bools(
        [&](auto longdt) {
            hipLaunchKernelGGL((k_gyro_chain<Rec, longdt.value>), side_grid(batch), dim3(kSideBlock), 0,
                               as_stream(stream), batch, n_steps, window, step0,
                               static_cast<const float4 *>(plane_gd), dt_ext, q_gyro, traj);
        },
        dt_ext != nullptr);
    return launched("k_gyro_chain");
}

int pekf_gyro_chain_rec64_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0, const void *plane_gd,
                              double *q_gyro, double *traj, void *stream) {
    const bool aligned = (uintptr_t)plane_gd % 32 == 0 && (uintptr_t)traj % 16 == 0;
    if (int st = side_args(batch, n_steps, window, step0, plane_gd && q_gyro,
                           aligned ? nullptr : "misaligned plane / traj pointer"))
        return st;
    if (batch == 0 || n_steps == 0) return PEKF_OK;
    hipLaunchKernelGGL((k_gyro_chain<Rec64, false>), side_grid(batch), dim3(kSideBlock), 0, as_stream(stream), batch,
                       n_steps, window, step0, static_cast<const double4 *>(plane_gd), nullptr, q_gyro, traj);
    return launched("k_gyro_chain<Rec64>");
}

int pekf_wahba_stream_rec64_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0, const void *plane_am,
                                const void *plane_my, const double *refs, double k_acc, double k_mag, double *out,
                                void *stream) {
    const bool aligned = (uintptr_t)plane_am % 32 == 0 && (uintptr_t)plane_my % 16 == 0 && (uintptr_t)out % 16 == 0;
    if (int st = side_args(batch, n_steps, window, step0, plane_am && plane_my && refs && out,
                           aligned ? nullptr : "misaligned plane / out pointer"))
        return st;
    if (batch == 0 || n_steps == 0) return PEKF_OK;
    hipLaunchKernelGGL(k_wahba_stream<Rec64>, side_grid(batch), dim3(kSideBlock), 0, as_stream(stream), batch, n_steps,
                       window, step0, static_cast<const double4 *>(plane_am), static_cast<const double2 *>(plane_my),
                       refs, k_acc, k_mag, out);
    return launched("k_wahba_stream<Rec64>");
}

int pekf_gyro_chain_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0,
                        const void *plane_gd, double *q_gyro, double *traj, void *stream) {
    return pekf_gyro_chain_ext_dev(batch, n_steps, window, step0, plane_gd, nullptr, q_gyro, traj, stream);
}

int pekf_wahba_stream_dev(int64_t batch, int64_t n_steps, int64_t window, int64_t step0,
                          const void *plane_am, const void *plane_my, const double *refs, double k_acc,
                          double k_mag, double *out, void *stream) {
    if (int st = side_args(batch, n_steps, window, step0, plane_am && plane_my && refs && out, nullptr)) return st;
    if (batch == 0 || n_steps == 0) return PEKF_OK;
    hipLaunchKernelGGL(k_wahba_stream<Rec>, side_grid(batch), dim3(kSideBlock), 0, as_stream(stream), batch, n_steps,
                       window, step0, static_cast<const float4 *>(plane_am), static_cast<const float2 *>(plane_my),
                       refs, k_acc, k_mag, out);
    return launched("k_wahba_stream");
}

int pekf_quat_to_rpy_dev(int64_t n, const double *q, double *rpy, void *stream) {
    PEKF_CHECK_ARG(n >= 0, "n < 0");
    if (n == 0) return PEKF_OK;
    PEKF_CHECK_ARG(q && rpy, "null pointer");
    hipLaunchKernelGGL(k_rpy, dim3(grid_for(n, kSideBlock)), dim3(kSideBlock), 0, as_stream(stream), n,
                       OpPtrs<OpRpy>{{q}, {rpy}}, nullptr, kNoSignal);
    return launched("k_rpy");
}

int pekf_quat_to_rpy(int64_t n, const double *q, double *rpy) {
    PEKF_CHECK_ARG(n >= 0, "n < 0");
    if (n == 0) return PEKF_OK;
    PEKF_CHECK_ARG(q && rpy, "null pointer");
    return staged_call<OpRpy, kSideBlock>(k_rpy, n, {{q}, {rpy}});
}

}  // extern "C"
