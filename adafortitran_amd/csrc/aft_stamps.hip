// aft_stamps.hip -- the diagnostic build's host facility (-DAFT_DIAG_STAMPS, switch AFT_STAMPS): StampRun (aft_internal.h), the one
// stamp buffer per device (one stamped launch at a time uses it) and the "first N reports of a kind" counters.  Empty in the product build.
#ifdef AFT_DIAG_STAMPS
#include <cstdio>
#include <mutex>

#include "aft_internal.h"
#include "stamp_report.h"

namespace aft {

namespace {
constexpr size_t kRowBytes = sizeof(unsigned long long) * kStampSlots;
std::mutex g_mu;
unsigned long long *g_buf[kMaxDevices];        // kStampRows rows each, allocated on the device's first stamped launch
// reports each kind still gets: the first 2 launches of each chain variant and of attention, 4 of either conv kernel, 3 of the training chain
int g_left[kStampKinds] = {2, 2, 2, 2, 4, 4, 3};
}  // namespace

StampRun::StampRun(Switch sw, StampKind kind, long long rows, hipStream_t st) : kind_(kind), rows_(rows), st_(st) {
    if (!switch_on(sw) || rows <= 0) return;   // (no rows: a launch the caller does not want stamped)
    if (!stamp_rows_fit(rows)) {
        printf("stamps: a launch of %lld rows does not fit the buffer's %d rows: not stamped\n", rows, kStampRows);
        fflush(stdout);
        return;
    }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return;
    std::lock_guard<std::mutex> lock(g_mu);
    unsigned long long *&buf = g_buf[current_device()];
    if (!buf && hipMalloc(&buf, kRowBytes * kStampRows) != hipSuccess) { buf = nullptr; (void)hipGetLastError(); return; }
    if (hipMemsetAsync(buf, 0, kRowBytes * (size_t)rows, st) == hipSuccess) dev_ = buf;
}

const unsigned long long *StampRun::collect() {
    if (!dev_) return nullptr;
    if (!host_.empty()) return host_.data();
    {
        std::lock_guard<std::mutex> lock(g_mu);
        if (g_left[kind_] <= 0) return nullptr;   // stamped, but this kind has had its reports
        --g_left[kind_];
    }
    host_.resize((size_t)rows_ * kStampSlots);
    if (hipStreamSynchronize(st_) == hipSuccess && hipMemcpy(host_.data(), dev_, kRowBytes * (size_t)rows_, hipMemcpyDeviceToHost) == hipSuccess)
        return host_.data();
    host_.clear();
    return nullptr;
}

}  // namespace aft
#endif
