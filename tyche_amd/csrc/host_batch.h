// host_batch.h -- internal interface between the C-ABI layer (engine.hip) and the host batch
// pipeline (host_batch.hip): run_host and what goes with it, and the few things the pipeline
// and the shared-dictionary layer (dict.hip) need from engine.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tyche_codec.h"

namespace tyche {

// ---- from engine.hip
constexpr int kMaxDevices = 64;

// set the calling thread's error text (tyche_last_error) and return TYCHE_E_DEVICE
int fail(const char *what, hipError_t e);
int fail_msg(const std::string &m);
const std::string &thread_error();
void set_thread_error(const std::string &m);
// TYCHE_LOG_ERRORS=1: the line a failure leaves on stderr (fail and fail_msg write it themselves)
void log_error(const std::string &m);

uint64_t now_ns();

// The devices the host API uses when the thread is not pinned: the visible
// gfx950 devices, the first TYCHE_DEVICES of them when that is set.
struct DeviceSet {
    std::vector<int> ids;
    std::string why;   // empty when ids is non-empty
};
const DeviceSet &device_set();
// -1: the host API spreads work over every usable device (the default);
// >= 0: tyche_set_device pinned the calling thread to that device
int pinned_device();
// makes `dev` current on this thread after checking it (cached per device)
int ensure_device(int dev);
// the device for a thread's device-side work: its pinned one, the rank's, else the first of the set
int current_device(int *dev);
// makes the device of stream s (when it has one) current for a device-resident call
int stream_device(hipStream_t s);

// the encoder kernel for a codec id; compress_launch_fails is the FAIL_COMPRESS_EVERY test hook,
// asked once per encode launch (launch_encode asks it itself)
hipError_t launch_encode(int id, const tyche_batch_t &b, uint32_t in_cap, hipStream_t s);
bool compress_launch_fails();

// Restores the calling thread's current device when it goes out of scope: the
// host entry points switch devices to run a batch, and a caller (a torch rank
// after set_device, say) must find its own device current afterwards.
struct DeviceGuard {
    int saved = -1;
    DeviceGuard() {
        if (hipGetDevice(&saved) != hipSuccess) saved = -1;
    }
    ~DeviceGuard() {
        int now = -1;
        if (saved >= 0 && hipGetDevice(&now) == hipSuccess && now != saved) (void)hipSetDevice(saved);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// ---- from host_batch.hip
// run_host's direct_out modes (see run_host_batch)
enum { kDirectNone = 0, kDirectAlways = 1, kDirectLz4Decode = 2 };

// A chunk's launch, hipError_t(const tyche_batch_t &, hipStream_t, bool host_dst), by reference: the
// callable lives in the caller's frame for the whole run_host call, so nothing is allocated or copied
// per call (the restore path runs one per page).
class LaunchRef {
  public:
    template <typename F, typename = std::enable_if_t<!std::is_same<std::decay_t<F>, LaunchRef>::value>>
    LaunchRef(F &&f)
        : obj_((void *)&f), call_([](void *o, const tyche_batch_t &b, hipStream_t s, bool host_dst) -> hipError_t {
              return (*(std::remove_reference_t<F> *)o)(b, s, host_dst);
          }) {}
    hipError_t operator()(const tyche_batch_t &b, hipStream_t s, bool host_dst) const { return call_(obj_, b, s, host_dst); }

  private:
    void *obj_;
    hipError_t (*call_)(void *, const tyche_batch_t &, hipStream_t, bool);
};

// Host batch over the calling thread's devices (host_batch.hip)
int run_host(size_t n, const void *const *src, const uint32_t *src_len, void *const *dst, const uint32_t *dst_cap,
             int32_t *results, LaunchRef launch, bool zc_ok = false, int direct_out = kDirectNone);

// the host path's stage clocks since the last read, for tyche_host_profile: up to n values, returns how many
int host_profile_read(uint64_t *out, int n);

// the device of a process launched one per GPU (LOCAL_RANK), -1 when not pinned that way
int rank_device();

}  // namespace tyche
