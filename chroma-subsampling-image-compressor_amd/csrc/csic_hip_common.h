// csic_hip_common.h -- shared by the HIP translation units (csic_kernels.hip, csic_planar.hip, csic_planar_bits.hip,
// csic_decode.hip, csic_distortion.hip, csic_ssim.hip, csic_pipeline.hip, csic_files.hip, csic_multi.hip, csic_graph.hip): error
// macro, the HIP instantiation of the device guard, the plan, the launch descriptor that csic_kernels.hip prepares for the other
// units, the device staging of the synchronous *_host wrappers, the run-time-value -> template-argument helper and the launch
// shell of the units' entry points (ilog2, for_frame_batches, launch, reconstruct_device).  Which kernel a plane unit takes and with
// what grid and block is csic_select.cpp's (plan_planar, plan_planar_bits, plan_reconstruct, plan_decode).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "csic_device_guard.h"
#include "csic_internal.h"
#include "csic_select.h"

// The plan behind the opaque handle of csic.h.  `sel` / `name` are what select_kernel / kernel_name give for (p, g, tune) with
// no launch constraints (the planar formats: FAM_PLANAR and the name of their own kernel); refreshed by csic_plan_tune.
struct csic_plan {
    csic_params p;
    csic::Geometry g;
    int device;
    csic::Tune tune;
    csic::Selection sel;
    char name[96];
    // host path staging
    void *d_in, *d_out;
    unsigned long long *d_sum;
};

namespace csic {

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return ::csic::set_error(CSIC_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

struct HipDeviceApi {
    static int get(int *d) { return (int)hipGetDevice(d); }
    static int set(int d) { return (int)hipSetDevice(d); }
};
using DeviceGuard = BasicDeviceGuard<HipDeviceApi>;

// `CSIC_DEVICE_SCOPE(dev);` at the top of an entry point: `dev` is current until the scope ends, then the
// caller's device is current again.  Returns CSIC_EHIP from the enclosing function if the switch fails.
#define CSIC_DEVICE_SCOPE(dev)                                                                              \
    ::csic::DeviceGuard csic_device_guard_(dev);                                                            \
    if (csic_device_guard_.status() != 0)                                                                   \
        return ::csic::set_error(CSIC_EHIP, "cannot make device %d current: %s", (int)(dev),                \
                                 hipGetErrorString((hipError_t)csic_device_guard_.status()))

// Device staging of a synchronous *_host wrapper (csic_decode_host, csic_distortion_host, csic_ssim_host): buffers that live
// until the scope ends and copies on the null stream.  The first HIP error is kept and turns every later call into a no-op, so a
// wrapper runs its sequence straight through and looks at error() once.
class DeviceStaging {
public:
    DeviceStaging() = default;
    DeviceStaging(const DeviceStaging &) = delete;
    DeviceStaging &operator=(const DeviceStaging &) = delete;
    ~DeviceStaging() { for (int i = 0; i < n_; ++i) (void)hipFree(buf_[i]); }
    void *alloc(size_t bytes)                       // nullptr after an error
    {
        void *p = nullptr;
        if (ok()) keep(n_ < MAX_BUFFERS ? hipMalloc(&p, bytes) : hipErrorInvalidValue);   // (more than MAX_BUFFERS: a bug here, not a full device)
        if (p) buf_[n_++] = p;
        return p;
    }
    void to_device(void *dst, const void *src, size_t bytes) { if (ok()) keep(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, nullptr)); }
    void to_host(void *dst, const void *src, size_t bytes) { if (ok()) keep(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, nullptr)); }
    void sync() { if (ok()) keep(hipStreamSynchronize(nullptr)); }
    bool ok() const { return err_ == hipSuccess; }
    hipError_t error() const { return err_; }
private:
    static constexpr int MAX_BUFFERS = 4;           // csic_ssim_host takes all four: raise it with the next buffer
    void keep(hipError_t e) { if (err_ == hipSuccess) err_ = e; }
    void *buf_[MAX_BUFFERS] = {};
    int n_ = 0;
    hipError_t err_ = hipSuccess;
};

using KernelFn = void (*)(KArgs);

// One fully resolved launch of the fused kernel: what hipLaunchKernel / hipGraphAddKernelNode need.
struct LaunchDesc {
    KernelFn fn;
    dim3 grid, block;
    KArgs args;
};

// csic_kernels.hip: validates the call, resolves kernel + geometry for `nframes` frames (<= 65535, the grid z
// limit) and fills *d.  Does not touch the device.
int prepare_launch(const csic_plan *pl, const void *d_in, void *d_out, int nframes, int32_t in_pitch, int32_t out_pitch,
                   LaunchDesc *d);
// The same for `nframes` frames in SEPARATE buffers named by device-resident pointer tables (one launch, frame index on
// grid z): `align_bits` is the bitwise OR of every frame pointer in the tables (the vector kernels need all of them 16-byte aligned).
int prepare_launch_table(const csic_plan *pl, const void *const *d_in_tab, void *const *d_out_tab, uintptr_t align_bits, int nframes,
                         LaunchDesc *d);
int enqueue(const LaunchDesc &d, hipStream_t stream);
int launch_on_stream(csic_plan *pl, const void *d_in, void *d_out, int nframes, hipStream_t stream);
// csic_planar.hip: out_format = CSIC_FMT_PLANAR (forward: packed input -> planar frame buffers; name of the kernel a plan takes)
// csic_planar.hip: the second kernel argument of the planar kernels, and a prepared planar launch (as LaunchDesc for the packed ones)
struct PExtra {
    uint8_t *planar;              // forward: destination frame buffers, frame_bytes apart; reconstruct: source
    const uint64_t *planar_tab;   // forward, frame-table mode: device-resident table of the frames' planar buffers (else NULL)
    uint32_t *packed;             // reconstruct: destination (n pixels per frame, back to back)
    int64_t cb_off, cr_off, frame_bytes, n;
    int32_t Wm, Wc, lhe, lve, replay_last;      // module width, samples per chroma row, log2 hold_h / hold_v
    uint32_t mWm, kWm;                          // exact j / Wm (magic_div)
    int32_t T;                                  // threads per block
};
struct PlanarLaunchDesc {
    void (*fn)(KArgs, PExtra);
    dim3 grid, block;
    KArgs args;
    PExtra extra;
};
int planar_forward(const csic_plan *pl, const void *d_in, void *d_planar, int nframes, hipStream_t stream);
// `nframes` (<= 65535) frames in SEPARATE buffers named by device-resident pointer tables: resolves kernel + geometry (no device work)
int planar_prepare_table(const csic_plan *pl, const void *const *d_in_tab, void *const *d_planar_tab, uintptr_t align_bits, int nframes,
                         PlanarLaunchDesc *d);
int planar_enqueue(const PlanarLaunchDesc &d, hipStream_t stream);
// csic_planar_bits.hip: out_format = CSIC_FMT_PLANAR_BITS (forward: packed input -> bit-packed planar frame buffers)
int planar_bits_forward(const csic_plan *pl, const void *d_in, void *d_bits, int nframes, hipStream_t stream);
void plan_sizes(const csic_plan *pl, size_t *in_px, size_t *out_px);
int64_t plan_algorithmic_bytes(const csic_plan *pl);          // per frame (csic_algorithmic_bytes of the plan's parameters)


// with_const<V0, V1, ...>(v, fn): calls fn with v as a compile-time constant -- std::integral_constant<.., Vi> for the Vi equal
// to v, the last one listed if none is (the callers' values are validated long before).  The one place a run-time value turns
// into a template argument: only the listed values are ever instantiated.
template <auto V0, auto... Vs, class T, class Fn>
auto with_const(T v, Fn &&fn)
{
    if constexpr (sizeof...(Vs) == 0) return fn(std::integral_constant<decltype(V0), V0>{});
    else return v == (T)V0 ? fn(std::integral_constant<decltype(V0), V0>{}) : with_const<Vs...>(v, fn);
}
#define CSIC_CONST(x) decltype(x)::value     // the value of a with_const argument, usable as a template argument inside nested lambdas

// ------------------------------------------------------------------------------------------------
// the launch shell of the units' entry points
// ------------------------------------------------------------------------------------------------
inline int ilog2(int x) { int l = 0; while ((1 << l) < x) ++l; return l; }

// fn(f0, nz) for every batch of at most 65535 frames (the grid z limit): frames f0 .. f0 + nz - 1.  Stops at the first status
// that is not CSIC_OK and returns it.
template <class Fn> int for_frame_batches(int nframes, Fn &&fn)
{
    for (int f0 = 0; f0 < nframes; f0 += 65535) {
        const int st = fn(f0, nframes - f0 < 65535 ? nframes - f0 : 65535);
        if (st != CSIC_OK) return st;
    }
    return CSIC_OK;
}

// One kernel launch: the arguments are converted to the kernel's parameter types and copied, as <<< >>> would.
template <class... P>
int launch(void (*fn)(P...), dim3 grid, dim3 block, hipStream_t stream, std::common_type_t<P>... args)
{
    void *params[] = {static_cast<void *>(&args)...};
    HIP_TRY(hipLaunchKernel(reinterpret_cast<const void *>(fn), grid, block, params, 0, stream));
    return CSIC_OK;
}

// csic_reconstruct_device / csic_reconstruct_bits_device: the refusals, the kernel for (out_format, fast, nontemporal) and one launch
// per batch of frames as plan_reconstruct lays it out -- K groups of 4 positions per lane.  Extra is the kernels' second argument (PExtra, BExtra: frame_bytes, n, Wm,
// T, packed and the source pointer *src); fill(plan, &e) fills it from the plan's layout, pick(fmt, fast, nt) names the kernel.
template <class Extra, class Fill, class Pick>
int reconstruct_device(csic_plan *plan, const void *d_src, uint8_t *Extra::*src, void *d_out, int32_t nframes, int32_t out_format,
                       void *hip_stream, const char *entry, const char *align_msg, int K, Fill fill, Pick pick)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!d_src || !d_out) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    if (nframes <= 0) return set_error(CSIC_EINVAL_SIZE, "nframes must be positive. Got %d", nframes);
    if (out_format != CSIC_FMT_ARGB8888 && out_format != CSIC_FMT_YCBCR888X)
        return set_error(CSIC_EINVAL_FORMAT, "%s writes ARGB8888(0) or YCBCR888X(1). Got %d", entry, out_format);
    if (((uintptr_t)d_src & 255u) || ((uintptr_t)d_out & 15u)) return set_error(CSIC_EINVAL_SIZE, "%s", align_msg);
    using Fn = void (*)(KArgs, Extra);
    KArgs a;
    fill_base_args(plan->g, plan->g.W, plan->g.Wo, &a);
    Extra e;
    fill(plan, &e);
    CSIC_DEVICE_SCOPE(plan->device);
    ReconPlan rp;
    plan_reconstruct(plan->g, plan->tune, e.Wm, K, nframes, &rp);
    const Fn fn = with_const<(int)CSIC_FMT_ARGB8888, (int)CSIC_FMT_YCBCR888X>(out_format, [&](auto fmt) {
        return with_const<true, false>(rp.fast, [&](auto fa) {
            return with_const<true, false>(!plan->tune.no_nt, [&](auto nt) -> Fn { return pick(fmt, fa, nt); });
        });
    });
    e.T = rp.T;
    const int st = for_frame_batches(nframes, [&](int f0, int nz) {
        e.*src = const_cast<uint8_t *>(static_cast<const uint8_t *>(d_src)) + (int64_t)f0 * e.frame_bytes;
        e.packed = static_cast<uint32_t *>(d_out) + (int64_t)f0 * e.n;
        return launch(fn, dim3(rp.grid.x, 1, (unsigned)nz), dim3(rp.block.x, 1, 1), static_cast<hipStream_t>(hip_stream), a, e);
    });
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

} // namespace csic
