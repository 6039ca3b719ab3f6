// runtime.hip -- what the library keeps besides kernels: the tile-scheduling slots of the persistent kernels, the ABI
// version, event / launch timing and the error strings.
#include <ds_device.h>
#include <unistd.h>
#include "ds_common.h"
#include <map>
#include <mutex>
#include <utility>
#include <vector>
#include <stdlib.h>

// Scheduling slots of the persistent kernels (ds_device.h): tile counters that must be private to whatever can be in
// flight at the same time.
//   * Eager launches take the next of DS_SCHED_RING slots of their own (device, stream): launches of one stream run in
//     order, so the only launches that can ever share a slot are ones the stream itself serialises -- whatever other
//     streams, graphs or processes' worth of persistent launches are enqueued in between (a process-wide round-robin,
//     as before round 4, handed the slot of a kernel still queued on stream A to the 65th launch enqueued on stream B).
//   * A launch that is being CAPTURED into a graph keeps a slot of its own for good: the node carries the pointer and
//     can replay on any stream next to anything.
// THE MEMORY IS THE CALLER'S (round 6, SURVEY 8(b): "the library never hipMallocs ... no synchronise"): slots are carved
// from zeroed device buffers the caller hands over with ds_sched_set_workspace (the Python wrapper: one torch.zeros of
// ds_sched_workspace_bytes() per device, allocated when a model is moved to the device or on the first launch there);
// a kernel leaves its slot zeroed.  Without a workspace -- or with every slot of it taken by captured launches -- a
// persistent launch returns DS_ERR_NO_WORKSPACE and the caller hands over another buffer.  Host side is serialised by a
// mutex; the only state the library keeps is the table of what has been carved.
namespace {
struct SchedPool {
    std::mutex mu;
    struct Chunk { unsigned *base; size_t slots, used; };
    std::map<int, std::vector<Chunk>> chunks;                               // device -> the caller's buffers
    std::map<std::pair<int, void *>, std::pair<unsigned *, unsigned>> rings;  // (device, stream) -> (ring base, next)

    unsigned *carve(int dev, size_t n_slots) {
        for (auto &c : chunks[dev])
            if (c.used + n_slots <= c.slots) {
                unsigned *r = c.base + c.used * DS_SCHED_WORDS;
                c.used += n_slots;
                return r;
            }
        return nullptr;
    }
    size_t free_slots(int dev) {
        size_t n = 0;
        for (auto &c : chunks[dev]) n += c.slots - c.used;
        return n;
    }
};
SchedPool &sched_pool() { static SchedPool p; return p; }
}  // namespace

unsigned *ds_sched_slot(void *stream) {
    SchedPool &P = sched_pool();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    bool capturing = false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing((hipStream_t)stream, &cs) == hipSuccess) capturing = cs == hipStreamCaptureStatusActive;
    else (void)hipGetLastError();
    std::lock_guard<std::mutex> lock(P.mu);
    if (capturing) return P.carve(dev, 1);
    auto key = std::make_pair(dev, stream);
    auto it = P.rings.find(key);
    if (it == P.rings.end()) {
        unsigned *base = P.carve(dev, DS_SCHED_RING);
        if (!base) return nullptr;
        it = P.rings.emplace(key, std::make_pair(base, 0u)).first;
    }
    const unsigned k = it->second.second++ % DS_SCHED_RING;
    return it->second.first + (size_t)k * DS_SCHED_WORDS;
}

// bytes of one scheduler workspace: 1024 slots of 64 bytes (a ring of 8 per stream that launches persistent kernels,
// one per persistent launch captured into a graph)
extern "C" size_t ds_sched_workspace_bytes(void) { return (size_t)1024 * DS_SCHED_WORDS * sizeof(unsigned); }

// Hands `bytes` of ZEROED device memory on the CURRENT device to the persistent kernels' tile scheduler.  The buffer
// must stay allocated for as long as the library may launch (the wrapper keeps the tensor alive for the life of the
// process); it may be called again to add a buffer when DS_ERR_NO_WORKSPACE says the previous ones are used up.
extern "C" int ds_sched_set_workspace(void *zeroed_device_memory, size_t bytes) {
    DS_REQUIRE(zeroed_device_memory != nullptr, DS_ERR_NULL);
    DS_REQUIRE(DS_ALIGNED16(zeroed_device_memory), DS_ERR_ALIGNMENT);
    const size_t slots = bytes / (DS_SCHED_WORDS * sizeof(unsigned));
    DS_REQUIRE(slots >= 2 * DS_SCHED_RING, DS_ERR_BAD_SHAPE);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return DS_ERR_UNSUPPORTED; }
    SchedPool &P = sched_pool();
    std::lock_guard<std::mutex> lock(P.mu);
    P.chunks[dev].push_back({(unsigned *)zeroed_device_memory, slots, 0});
    return DS_OK;
}

// slots of the current device's workspaces that have not been handed out yet (0: ds_sched_set_workspace is due)
extern "C" long long ds_sched_free_slots(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return -1; }
    SchedPool &P = sched_pool();
    std::lock_guard<std::mutex> lock(P.mu);
    return (long long)P.free_slots(dev);
}

/* ds_version history:
 *   1300  waveform augmentation: reverberation, noise at an SNR, level (augment.hip)
 *   1200  score normalisation: cohort statistics by radix select (score_norm.hip)
 *   1100  angular-margin softmax head (margin_head.hip)
 *   1000  energy VAD (vad.hip)
 *    900  polyphase resampler (resample.hip)
 *    800  speaker identification (identify.hip)
 *    700  log-mel filterbank front end (ds_fbank_*)
 *    600  round 6 (caller-owned scheduler workspace, ds_mfma_rate_probe_data)
 *    500  round 5
 *    400  round 4 (fp16 training step, refinement probes, launch-bound timing)
 *    301  + ds_conv_dgrad_bnbwd_bf16, ds_bn_bwd_group_finish_f32
 *    300  round-3 ABI: split grouped BatchNorm backward for data parallelism, grouped f64 sums
 */
extern "C" int ds_version(void) { return 1300; }

// ---- launch timing (see DS_LAUNCH_BIG_LDS in ds_device.h) ----
extern "C" int ds_event_create(void **out_event) {
    DS_REQUIRE(out_event != nullptr, DS_ERR_NULL);
    hipEvent_t e = nullptr;
    const hipError_t rc = hipEventCreate(&e);
    if (rc != hipSuccess) return (int)rc;
    *out_event = (void *)e;
    return DS_OK;
}

extern "C" int ds_event_destroy(void *event) {
    DS_REQUIRE(event != nullptr, DS_ERR_NULL);
    return (int)hipEventDestroy((hipEvent_t)event);
}

// milliseconds between two events (waits for `stop` first, at most 2 s)
extern "C" int ds_event_elapsed_ms(void *start, void *stop, float *ms) {
    DS_REQUIRE(start && stop && ms, DS_ERR_NULL);
    // bounded wait (2 s): an event that was armed but never bound to a launch must not hang the caller
    hipError_t rc = hipEventQuery((hipEvent_t)stop);
    for (int i = 0; rc == hipErrorNotReady && i < 20000; ++i) {
        usleep(100);
        rc = hipEventQuery((hipEvent_t)stop);
    }
    if (rc != hipSuccess) {
        (void)hipGetLastError();
        return (int)rc;
    }
    rc = hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
    if (rc != hipSuccess) (void)hipGetLastError();
    return (int)rc;
}

// The NEXT big-LDS kernel launch of this thread (the MFMA convolution / filter-gradient kernels) records its own
// execution into (start, stop).  ds_launch_timing_end() disarms and returns the number of such launches since arming
// (the caller expects 1: a call that launched several kernels timed only its first).
extern "C" int ds_launch_timing_arm(void *start, void *stop) {
    DS_REQUIRE(start && stop, DS_ERR_NULL);
    ds_timing_arm_state = {(hipEvent_t)start, (hipEvent_t)stop, 1, 0};
    return DS_OK;
}

extern "C" int ds_launch_timing_end(void) {
    const int n = ds_timing_arm_state.launches;
    ds_timing_arm_state = {nullptr, nullptr, 0, 0};
    return n;
}

extern "C" const char *ds_error_string(int code) {
    switch (code) {
        case DS_OK: return "ok";
        case DS_ERR_BAD_SHAPE: return "bad shape";
        case DS_ERR_ALIGNMENT: return "pointer not 16-byte aligned";
        case DS_ERR_NULL: return "null pointer";
        case DS_ERR_UNSUPPORTED: return "unsupported configuration";
        case DS_ERR_NO_WORKSPACE: return "no free tile-scheduling slot on this device: hand over zeroed device memory with ds_sched_set_workspace";
        default: return code > 0 ? "HIP runtime error (hipError_t)" : "unknown error";
    }
}
