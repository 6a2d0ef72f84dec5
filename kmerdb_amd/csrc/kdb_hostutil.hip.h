// kdb_hostutil.hip.h -- what every host file of libkdbhip.so reports errors and selects a device with: the thread's last error message
// (kdb_last_error reads it), fail(), HIP_TRY and DeviceGuard, and the owners of device memory, pinned memory, events and streams
// (DevBuf, PinnedBuf, Event, Stream).  One translation unit includes it, so the unnamed namespace is the library's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/kdbhip.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail(KDB_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),   \
                        __FILE__, __LINE__);                                                  \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; (void)hipSetDevice(dev); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// What owns device memory, pinned memory, an event or a stream frees it when it goes (the engine's members, a call's scratch).
struct NoCopy { NoCopy() = default; NoCopy(const NoCopy &) = delete; NoCopy &operator=(const NoCopy &) = delete; };

template <class T>
struct DevBuf : NoCopy {
    T *p = nullptr;
    size_t cap = 0;                                      // bytes
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    T *operator->() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // exactly nbytes, for a buffer that holds nothing yet; the caller reports the error
    hipError_t alloc(size_t nbytes)
    {
        const hipError_t err = hipMalloc((void **)&p, nbytes);
        if (err != hipSuccess) p = nullptr; else cap = nbytes;
        return err;
    }
    // grow-only scratch: room for need_bytes and a quarter more.  The old array is freed first (nothing may still read it), and where the
    // new one does not fit none is held.
    int grow(size_t need_bytes)
    {
        if (cap >= need_bytes) return KDB_OK;
        release();
        const size_t want = need_bytes + need_bytes / 4 + 256;
        const hipError_t err = alloc(want);
        if (err != hipSuccess) { (void)hipGetLastError(); return fail(KDB_ERR_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(err)); }
        return KDB_OK;
    }
};

template <class T>
struct PinnedBuf : NoCopy {
    T *p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    operator T *() const { return p; }
    hipError_t alloc(size_t nbytes) { return hipHostMalloc((void **)&p, nbytes, hipHostMallocDefault); }
};

struct Event : NoCopy {                                  // (no timing: an order between streams, or something for the host to wait for)
    hipEvent_t ev = nullptr;
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    operator hipEvent_t() const { return ev; }
    hipError_t create() { return hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
};

struct Stream : NoCopy {
    hipStream_t s = nullptr;
    ~Stream() { (void)destroy(); }
    operator hipStream_t() const { return s; }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    hipError_t destroy() { const hipError_t err = s ? hipStreamDestroy(s) : hipSuccess; s = nullptr; return err; }
};

}  // namespace
