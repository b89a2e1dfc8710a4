// Host side of the extern "C" wrappers: operand checks, per-kernel launch attributes, grid limits and the launch status.
// Host code only; common.h holds what kernels need.
//
// One process, one device.  The statics below (a kernel's dynamic-LDS attribute, the CU count) are set for the device that is
// current at the first call and never again: the library serves one device per process (one rank per device; several streams of
// that device are fine).
#pragma once
#include <initializer_list>

#include "common.h"

namespace rdetr {

// ---- operands -----------------------------------------------------------------------------------------------------------------
// A NULL pointer counts as aligned.  Whether an operand may be NULL is the wrapper's own question, asked first and answered with
// RDETR_ERR_INVALID_ARG; an optional operand that is absent then needs no guard here.
inline bool aligned_to(const void *p, unsigned a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

template <typename... P> inline bool all_aligned(unsigned a, P... p) { return (aligned_to(p, a) && ...); }

// The row contract of the vector kernels: [rows, C] elements of elem_bytes each, row stride ld elements, read and written in 16-byte
// pieces -- ld >= C (else RDETR_ERR_INVALID_ARG), ld a multiple of 16 bytes and the base 16-byte aligned (else
// RDETR_ERR_UNSUPPORTED).  Over several operands an invalid stride is reported before an unsupported one, whichever operand has it.
struct Rows {
    const void *p;
    long long ld, C;
    int elem_bytes;
};

inline int rows_status(std::initializer_list<Rows> operands)
{
    for (const Rows &r : operands)
        if (r.ld < r.C) return RDETR_ERR_INVALID_ARG;
    for (const Rows &r : operands)
        if (r.ld % (16 / r.elem_bytes) != 0 || !aligned_to(r.p, 16)) return RDETR_ERR_UNSUPPORTED;
    return RDETR_OK;
}

inline bool rows_ok(const void *p, long long ld, long long C, int elem_bytes) { return rows_status({{p, ld, C, elem_bytes}}) == RDETR_OK; }

// ---- launch -------------------------------------------------------------------------------------------------------------------
// Allows Kernel up to `bytes` of dynamic LDS (above the 64 KiB every kernel may use).  One function-local static per kernel, so every
// instantiation of a kernel template sets its own attribute, once, thread-safely; `bytes` is the most the kernel is ever launched
// with (the first call's value is the one that is set).
template <auto Kernel> inline int ensure_dynamic_lds(int bytes)
{
    static const hipError_t set =
        hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return set == hipSuccess ? RDETR_OK : RDETR_ERR_LAUNCH;
}

// CUs of the current device, asked once; kCus where the runtime does not say
inline int device_cu_count()
{
    static const int cus = [] {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return kCus;
        return prop.multiProcessorCount > 0 ? prop.multiProcessorCount : kCus;
    }();
    return cus;
}

// a one-dimensional grid of nblk workgroups can be launched
inline bool grid_fits(long long nblk) { return nblk <= 0x7fffffffll; }

inline int launch_status()
{
    return hipGetLastError() == hipSuccess ? RDETR_OK : RDETR_ERR_LAUNCH;
}

}  // namespace rdetr
