// host-side helpers shared by the C-ABI translation units of libsdrx.so
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include <cstdio>
#include "../../include/sdrx.h"

namespace sdrx {

void set_error(const std::string& s);
int  hip_fail(hipError_t e, const char* what, const char* file, int line);
int  check_device(int device);           // SDRX_OK or SDRX_ENODEV (sets error)
int  device_cu_count(int device);

#define SDRX_HIP(call)                                                                 \
    do { hipError_t e_ = (call);                                                       \
         if (e_ != hipSuccess) return ::sdrx::hip_fail(e_, #call, __FILE__, __LINE__); \
    } while (0)

// the same for a create function past its `new`: `cleanup` (a destroy call, or `delete h`) runs before the return
#define SDRX_HIP_ELSE(call, cleanup)                                                   \
    do { hipError_t e_ = (call);                                                       \
         if (e_ != hipSuccess) { int r_ = ::sdrx::hip_fail(e_, #call, __FILE__, __LINE__); cleanup; return r_; } \
    } while (0)

// grow-only device buffer
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes);           // SDRX_OK / SDRX_ENOMEM
    void release();
};

// pairs of HIP events bracketing kernel launches on a stream
struct EventTimer {
    bool enabled = false;
    std::vector<hipEvent_t> ev;          // start0, stop0, start1, stop1, ...
    size_t used = 0;
    double total_ms = 0; long count = 0;
    int begin(hipStream_t s);            // records a start event (no-op when disabled)
    int end(hipStream_t s);
    int collect(hipStream_t s);          // sync + fold the recorded pairs into total_ms / count
    void release();
};

// what every handle that owns a stream embeds (as `core`): the device, the launch stream (its own unless the caller lent
// one), the feed timer and the record of the last launch.  The sdrx_*_{sync,set_stream,get_stream,set_timing,get_timing,
// last_launch} entry points check their handle and forward here.
struct HandleCore {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    EventTimer timer;
    struct { char name[96] = ""; int grid = 0, block = 0, lds = 0; } last;

    int open(int dev);                   // check_device, hipSetDevice, a non-blocking stream of its own
    void close();                        // waits for own_stream, releases the timer's events, destroys own_stream
    int sync();
    int set_stream(void* hip_stream);    // waits for the current stream first; nullptr: back to own_stream
    int get_stream(void** hip_stream) const;
    int set_timing(int enabled);
    int get_timing(double* total_ms, int64_t* count, int reset);
    void note_launch(const char* name, int grid, int block, int lds);
    int last_launch(char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) const;
};

} // namespace sdrx
