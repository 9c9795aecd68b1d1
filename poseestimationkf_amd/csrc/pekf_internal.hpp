// pekf_internal.hpp -- shared host-side plumbing of libpekf.so (error state, HIP checks,
// the pinned/device staging workspace used by the host-pointer entry points).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/pekf.h"

namespace pekf {

int set_error(int code, const char *fmt, ...);
int hip_fail(hipError_t e, const char *what);
int require_device();

#define PEKF_HIP(call)                                                   \
    do {                                                                 \
        hipError_t e_ = (call);                                          \
        if (e_ != hipSuccess) return ::pekf::hip_fail(e_, #call);        \
    } while (0)

#define PEKF_CHECK_ARG(cond, msg)                                        \
    do {                                                                 \
        if (!(cond)) return ::pekf::set_error(PEKF_ERR_INVALID, "%s", msg); \
    } while (0)

// After hipLaunchKernelGGL: the launch's error, if any, reported under the kernel's name.
// (static, like staged_call below: the library's exported symbols stay those of the C ABI and its plumbing)
static inline int launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return PEKF_OK;
}

// Run-time flags to template flags: calls f(std::bool_constant<b>{}...), so a generic lambda states a
// launch once and picks the kernel variant with <a.value, b.value, ...>.  Every combination is instantiated.
template <class F> inline void dispatch_bools(F &&f) { f(); }
template <class F, class... Bs> inline void dispatch_bools(F &&f, bool b, Bs... rest) {
    if (b) dispatch_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else   dispatch_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

inline unsigned grid_for(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// One record of the stream as it sits in the three planes (include/pekf.h, pekf_run_dev)
struct Rec {
    float4 gd;  // gx, gy, gz, bits(dt word)
    float4 am;  // ax, ay, az, mx
    float2 my;  // my, mz
};
// The FP64 record (pekf_run_rec64_dev's planes; pekf_frontend_ext_dev's output with FP64 events)
struct Rec64 {
    double4 gd;  // gx, gy, gz, dt_ns
    double4 am;  // ax, ay, az, mx
    double2 my;  // my, mz
};

// Host-pointer calls: inputs are packed into one coherent, mapped pinned buffer.  Small calls
// (<= kZeroCopyMaxBytes of inputs + outputs, e.g. the n = 1 calls of main_file.py) run
// zero-copy: the kernel reads and writes that buffer over PCIe, so a call is one launch and one
// synchronisation.  Larger calls copy it to device memory once each way.
constexpr size_t kZeroCopyMaxBytes = (size_t)1 << 16;
struct HostArg {
    const void *ptr;
    size_t bytes;
};
struct HostOut {
    void *ptr;
    size_t bytes;
};

// Completion signal of a one-block per-call launch (the zero-copy calls): every thread makes its
// writes visible system-wide, then one thread stores `seq` into a host-visible flag that the
// host polls instead of calling hipStreamSynchronize (measured on MI355X: 7.8 vs 12.4 us per
// round trip, scripts/sync_probe.hip).  flag == nullptr: no signal (device-pointer calls).
struct Done {
    unsigned *flag;
    unsigned seq;
    __device__ __forceinline__ void signal() const {
        if (!flag) return;  // uniform: a kernel argument
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
};
constexpr Done kNoSignal = {nullptr, 0u};

class Staging {
  public:
    // Packs `ins` into device memory; returns device addresses for ins and outs.
    // The caller enqueues its kernel on stream() between stage_in() and stage_out(), passing
    // done(grid blocks) to it so that a zero-copy one-block launch signals its completion.
    int stage_in(std::initializer_list<HostArg> ins, std::initializer_list<size_t> out_bytes,
                 void **dev_in, void **dev_out);
    int stage_out(std::initializer_list<HostOut> outs, void *const *dev_out);
    Done done(unsigned blocks);
    hipStream_t stream() const { return stream_; }
    ~Staging();

    static Staging &get();  // per calling thread, per current device
  private:
    int reserve(size_t bytes);
    int wait();
    hipStream_t stream_ = nullptr;
    char *dev_ = nullptr;
    char *host_ = nullptr;
    char *host_dev_ = nullptr;  // device address of host_
    unsigned *flag_ = nullptr;      // coherent pinned completion flag (host address)
    unsigned *flag_dev_ = nullptr;  // its device address
    unsigned seq_ = 0;
    bool signalled_ = false;        // the launch since stage_in() signals through flag_
    size_t cap_ = 0;
    size_t in_bytes_ = 0;
    bool zero_copy_ = false;
    int device_ = -1;
};

// A per-call operator is one table entry Op (pekf_percall.hip holds the table and states the form): Op::In and
// Op::Out are Widths<...>, the doubles per item of each operand in ABI order; everything else about the layout
// -- offsets, totals, the widest operand -- is derived from them here.
template <int... W>
struct Widths {
    static constexpr int count = sizeof...(W);
    static constexpr int total = (W + ... + 0);
    static constexpr int widest = std::max({W...});
    static constexpr int w(int k) {
        const int a[] = {W...};
        return a[k];
    }
    static constexpr int off(int k) {  // operand k's first double within an item's concatenated operands
        int s = 0;
        for (int j = 0; j < k; ++j) s += w(j);
        return s;
    }
};

// An operator's operand pointers (host or device), as its entry points take them.
template <class Op>
struct OpPtrs {
    const double *in[Op::In::count];
    double *out[Op::Out::count];
};
template <class Op>
using OpKernel = void (*)(int64_t, OpPtrs<Op>, int32_t *, Done);
template <class Op>
using Call1Fn = int (*)(const OpPtrs<Op> &, int32_t *);

// One host-pointer operator call: kernel(n, device operands, status plane, Done) over n items.  ONE is the
// operator's n = 1 route (call1<Op> of pekf_percall.hip) or nullptr; Op::kErr is the code a non-zero entry of the
// status plane maps to, with Op::kMsg, or PEKF_OK for a kernel without one.  The caller has checked its arguments.
template <class Op, int BLOCK, Call1Fn<Op> ONE, size_t... I, size_t... O>
static int staged_call(OpKernel<Op> kernel, int64_t n, const OpPtrs<Op> &a, std::index_sequence<I...>,
                       std::index_sequence<O...>) {
    using In = typename Op::In;
    using Out = typename Op::Out;
    constexpr bool kStatus = Op::kErr != PEKF_OK;
    if (int st = require_device()) return st;
    if constexpr (ONE != nullptr) {
        if (n == 1) {
            int32_t st1 = 0;
            if (int st = ONE(a, &st1)) return st;
            return kStatus && st1 ? set_error(Op::kErr, "%s", Op::kMsg) : PEKF_OK;
        }
    }
    const size_t b = (size_t)n * sizeof(double);
    Staging &s = Staging::get();
    // the status plane follows the outputs; without one it is an empty plane that nothing reads or writes
    std::vector<int32_t> status(kStatus ? (size_t)n : 0);
    const size_t sb = status.size() * sizeof(int32_t);
    void *din[In::count], *dout[Out::count + 1];
    if (int st = s.stage_in({{a.in[I], In::w(I) * b}...}, {Out::w(O) * b..., sb}, din, dout)) return st;
    const OpPtrs<Op> d = {{static_cast<const double *>(din[I])...}, {static_cast<double *>(dout[O])...}};
    hipLaunchKernelGGL(kernel, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, s.stream(), n, d,
                       kStatus ? static_cast<int32_t *>(dout[Out::count]) : nullptr, s.done(grid_for(n, BLOCK)));
    if (int st = launched(Op::kName)) return st;
    if (int st = s.stage_out({{a.out[O], Out::w(O) * b}..., {status.data(), sb}}, dout)) return st;
    for (int32_t v : status)
        if (v) return set_error(Op::kErr, "%s", Op::kMsg);
    return PEKF_OK;
}

template <class Op, int BLOCK, Call1Fn<Op> ONE = nullptr>
static int staged_call(OpKernel<Op> kernel, int64_t n, const OpPtrs<Op> &a) {
    return staged_call<Op, BLOCK, ONE>(kernel, n, a, std::make_index_sequence<Op::In::count>{},
                                       std::make_index_sequence<Op::Out::count>{});
}

// Stops the resident per-call service kernel (pekf_percall.hip) of every device, e.g. before a
// device-wide synchronisation, which would otherwise wait for its idle limit.
void service_quiesce_all();

// Filter-handle update kernel launcher (pekf_run.hip): one FP64 record per filter.
int launch_update(int64_t batch, const double *gyro, const int64_t *t_ns, const double *acc, const double *mag,
                  const uint8_t *missing, const double *refs, int64_t *prev_t, double *X, double *P, double q,
                  double r, double *x_out, uint32_t flags, hipStream_t stream);

// Multi-record fused launches over 40 B records (pekf_run_multi.hip, compiled with the max-ILP
// scheduler): every k_run<Rec, TRAJ, MIXED, SOA, COUNTS, ...> variant; arguments checked by
// pekf_run_ext_dev, which launches k_run_one itself for n_steps = 1.  (The k_run<Rec64, ...> variants
// are launched by pekf_run_rec64_dev in the same file.)
int launch_run_multi(int64_t batch, int64_t n_steps, int64_t window, int64_t step0, const float4 *gd,
                     const float4 *am, const float2 *my, const double *dtx, const double *refs, double *X,
                     double *P, double q, double r, double *traj, const int32_t *counts, bool mixed, bool soa,
                     hipStream_t stream);

}  // namespace pekf
