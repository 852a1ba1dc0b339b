// Host-only plumbing shared by the seven handles behind include/ls_hip.h (ls_handle, ls_sag, ls_sag_enc, ls_clip_text, ls_trainer, ls_eval, ls_post_stream): the
// device buffer every handle owns its memory through, the one error path (message formatter, HIP-status check, *_last_error) and
// the sinusoidal position table.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "ls_hip.h"

namespace ls {

// a device allocation that only grows; freed with its owner (the handle's device must be current)
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
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

// message of this thread's last failed create of a Handle (handles may be created from several threads)
template <class Handle>
std::string& create_error() {
    thread_local std::string msg;
    return msg;
}

// records the formatted message in the handle's `err` (h == nullptr: as this thread's create error of that handle type), returns code
template <class Handle>
int fail(Handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    (h ? h->err : create_error<Handle>()) = buf;
    return code;
}

// what every *_last_error returns
template <class Handle>
const char* last_error(const Handle* h) { return (h ? h->err : create_error<Handle>()).c_str(); }

// the failure exit of a *_create that already holds a handle: `code` comes from a fail<Handle>(nullptr, ...) that recorded the
// message; the handle goes through its own *_destroy, so streams, events and buffers made so far are released
template <class Handle>
int abandon(Handle* h, void (*destroy)(Handle*), int code) {
    destroy(h);
    return code;
}

#define HIPCHK(h, expr)                                                                         \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return ::ls::fail((h), LS_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

// PositionalEncoding.pe rows 0 .. rows-1 (mlp_module.py:104-116, motionclip_module.py:11-28), fp32 like the torch buffer
inline std::vector<float> pe_table(int rows, int D) {
    std::vector<float> pe((size_t)rows * D);
    const float cexp = (float)(-std::log(10000.0) / D);
    for (int i = 0; i < D / 2; ++i) {
        const float div = expf((float)(2 * i) * cexp);
        for (int p = 0; p < rows; ++p) {
            pe[(size_t)p * D + 2 * i] = sinf((float)p * div);
            pe[(size_t)p * D + 2 * i + 1] = cosf((float)p * div);
        }
    }
    return pe;
}

}  // namespace ls
