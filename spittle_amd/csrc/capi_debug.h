// capi_debug.h -- what the context-free test hooks share (capi_sample.cpp: spt_debug_sample_*,
// capi_attn.cpp: spt_debug_attn_*, capi_gemm.cpp: spt_debug_gemm, spt_debug_layernorm): the error
// message, the device check, a stream with the buffers of one call, the host rounding of f32 inputs to
// an engine dtype and the copies between host f32 and device storage of a dtype.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

#include "../../include/spittle_hip.h"
#include "capi_err.h"
#include "common.h"
#include "kernels.h"

namespace spt {
namespace dbg {

using spt::set_err;

// the calling thread's device and a stream on it, with every buffer the call allocates
struct Scope {
    hipStream_t st = nullptr;
    std::vector<void*> bufs;
    explicit Scope(int device) {
        HIP_CHECK(hipSetDevice(device));
        HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    }
    ~Scope() {
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
        for (void* p : bufs) (void)hipFree(p);
    }
    template <typename T> T* alloc(size_t n) {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, (n ? n : 1) * sizeof(T)));
        bufs.push_back(p);
        return (T*)p;
    }
    template <typename T> T* up(const T* h, size_t n) {
        T* p = alloc<T>(n);
        HIP_CHECK(hipMemcpyAsync(p, h, n * sizeof(T), hipMemcpyHostToDevice, st));
        return p;
    }
    // an output buffer the kernels must write: every byte 0xFF (a NaN in f32, bf16 and f16)
    template <typename T> T* out(size_t n) {
        T* p = alloc<T>(n);
        HIP_CHECK(hipMemsetAsync(p, 0xFF, (n ? n : 1) * sizeof(T), st));
        return p;
    }
    template <typename T> void down(T* h, const T* dev, size_t n) {
        HIP_CHECK(hipMemcpyAsync(h, dev, n * sizeof(T), hipMemcpyDeviceToHost, st));
    }
    void sync() { HIP_CHECK(hipStreamSynchronize(st)); }
};

inline spt_status device_ok(int32_t device, char* err, size_t errlen) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_err(err, errlen, "no HIP device available");
        return SPT_ERR_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        set_err(err, errlen, "device ordinal out of range");
        return SPT_ERR_INVALID_ARG;
    }
    return SPT_OK;
}

// f32 -> the storage of an engine dtype, on the host (round-to-nearest-even, the device's conversion)
inline std::vector<uint16_t> to_half_storage(int dtype, const float* v, size_t n) {
    std::vector<uint16_t> o(n);
    for (size_t i = 0; i < n; ++i) o[i] = dtype == DT_BF16 ? f2bf(v[i]) : f2h_bits(v[i]);
    return o;
}

// host f32 -> device storage of dtype (h16 keeps the rounded copy alive until the stream has read it)
inline const void* up_as(Scope& sc, int dtype, const float* v, size_t n, std::vector<uint16_t>& h16) {
    if (dtype == DT_F32) return sc.up(v, n);
    h16 = to_half_storage(dtype, v, n);
    return sc.up(h16.data(), n);
}

// device storage of dtype -> host f32
inline void down_f32(Scope& sc, int dtype, const void* dev, float* h, size_t n) {
    if (dtype == DT_F32) {
        sc.down(h, (const float*)dev, n);
        return;
    }
    float* f = sc.alloc<float>(n);
    to_f32(dtype, dev, f, (int64_t)n, sc.st);
    SPT_LAUNCH_CHECK();
    sc.down(h, (const float*)f, n);
}

}  // namespace dbg
}  // namespace spt
