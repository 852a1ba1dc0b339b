// Host-side pieces shared by the two SAG handles (ls_sag_api.cpp: decoder, ls_sag_enc_api.cpp: encoder): a device buffer that only
// grows, and the error text / HIP-status check both ABIs report through their ls_*_last_error.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "ls_hip.h"

namespace ls {

struct DeviceBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; bytes = 0; }
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    float* f() const { return static_cast<float*>(p); }
};

// stores the formatted message in the handle's `err` (or, without a handle, in `create_error`) and returns `code`
template <class Handle>
int sag_fail(Handle* h, std::string& create_error, int code, const char* fmt, va_list ap) {
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    (h ? h->err : create_error) = buf;
    return code;
}

}  // namespace ls

// `fail` is the file's own variadic wrapper of ls::sag_fail: fail(handle, code, fmt, ...)
#define LS_SAG_CHK(fail, h, expr)                                                                              \
    do {                                                                                                       \
        hipError_t e__ = (expr);                                                                               \
        if (e__ != hipSuccess)                                                                                 \
            return fail((h), LS_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)
