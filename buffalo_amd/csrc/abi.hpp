// The C boundary every handle kind shares: one create, one guarded call, one lifecycle.  Included by the files that define `extern "C"` entry points.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace bfh {

// the handle behind the `void*` of the C ABI
template <typename H>
static inline H* as(void* h) { return static_cast<H*>(h); }

static inline int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) throw Error(BFH_ERR_HIP, "no HIP device available (libbuffalo_hip has no CPU fallback)");
    return dev;
}

// bfh_*_create: a handle on the current HIP device, or NULL with the reason in bfh_last_error(NULL)
template <typename H>
static inline void* create_handle() {
    try {
        const int dev = current_device();
        H* h = new H();
        h->device = dev;
        return h;
    } catch (const std::exception& e) {
        g_create_error = e.what();
        return nullptr;
    }
}

// Selects the handle's device, runs `fn(handle)` and maps exceptions onto the status codes of buffalo_hip.h.  A body that returns nothing yields
// BFH_OK, a bool yields 1 / 0 (the `*_init` contract), an int is passed on.
template <typename H, typename F>
static inline int guarded(void* h, F&& fn) {
    if (!h) {
        g_create_error = "null handle";
        return BFH_ERR_INVALID;
    }
    H& x = *as<H>(h);
    try {
        BFH_HIP(hipSetDevice(x.device));
        if constexpr (std::is_void_v<decltype(fn(x))>) {
            fn(x);
            return BFH_OK;
        } else {
            return static_cast<int>(fn(x));
        }
    } catch (const Error& e) {
        x.last_error = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        x.last_error = "out of host memory";
        return BFH_ERR_NOMEM;
    } catch (const std::exception& e) {
        x.last_error = e.what();
        return BFH_ERR_INVALID;
    }
}

// bfh_*_stream
static inline void* stream_of(void* h) {
    if (!h) {
        g_create_error = "null handle";
        return nullptr;
    }
    return as<HandleBase>(h)->stream;
}

static inline int get_stats(void* h, bfh_stats* out) {
    return guarded<HandleBase>(h, [&](HandleBase& x) {
        BFH_REQUIRE(out, "get_stats: null output");
        x.refresh_stats();
        *out = x.stats;
    });
}
static inline int reset_stats(void* h) {
    return guarded<HandleBase>(h, [](HandleBase& x) {
        x.refresh_stats();   // what the timers still hold belongs to the interval that ends here
        x.stats = bfh_stats{};
        x.clear_accumulators();
    });
}

}  // namespace bfh

// create, destroy and get_stats of one handle kind (all that sppmi has) ...
#define BFH_ABI_CREATE_DESTROY_STATS(kind, Handle)                                                  \
    void* bfh_##kind##_create(void) { return ::bfh::create_handle<Handle>(); }                      \
    void bfh_##kind##_destroy(void* h) { delete ::bfh::as<Handle>(h); }                             \
    int bfh_##kind##_get_stats(void* h, bfh_stats* out) { return ::bfh::get_stats(h, out); }
// ... and the whole lifecycle of every other kind
#define BFH_ABI_LIFECYCLE(kind, Handle)                                                             \
    BFH_ABI_CREATE_DESTROY_STATS(kind, Handle)                                                      \
    int bfh_##kind##_set_device(void* h, int device) {                                              \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) { x.set_device(device); });                 \
    }                                                                                               \
    int bfh_##kind##_reset_stats(void* h) { return ::bfh::reset_stats(h); }
