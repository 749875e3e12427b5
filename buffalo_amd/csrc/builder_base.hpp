// What the three database builders (sppmi.hip, stream.hip, mm.hip) share on the host side: a handle with a stream of its own, the padded
// upload of a text, the way results reach the caller's arrays, and the fetch of one sorted group.
#pragma once
#include "common.hpp"
#include "text_tiles.hpp"

namespace bfh {

class BuilderHandle : public HandleBase {
 public:
    ~BuilderHandle() override {
        if (stream) (void)hipStreamDestroy(stream);
    }
    void ensure() {
        BFH_HIP(hipSetDevice(device));
        if (!stream) BFH_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    }
    // device -> the caller's array through the library's pinned ring (HostStager): the caller's arrays are pageable numpy memory
    void to_host(void* dst, const void* src, size_t bytes) {
        if (bytes == 0) return;
        BFH_REQUIRE(dst != nullptr, std::string(kind_) + ": an output array is missing");
        stager_.d2h(dst, src, bytes, stream, device);
        stats.d2h_bytes += static_cast<double>(bytes);
    }

 protected:
    explicit BuilderHandle(const char* kind) : kind_(kind) {}   // `kind` = the prefix of the handle's messages

    // fetches of a builder with a `built_` state
    void need_build() {
        BFH_REQUIRE(built_, std::string(kind_) + ": fetch before a successful build");
        ensure();
    }
    // bytes -> device, padded with zeros to whole tiles + 16 so that every 16-byte load of a tile is inside the buffer
    void upload_text(const char* text, int64_t bytes, DevBuf<char>& d) {
        const size_t padded = static_cast<size_t>(text_tiles_of(bytes)) * kTextTile + 16;
        grow(d, padded);
        if (bytes) BFH_HIP(hipMemcpyAsync(d.get(), text, static_cast<size_t>(bytes), hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemsetAsync(d.get() + bytes, 0, padded - static_cast<size_t>(bytes), stream));
    }

    bool built_ = false;

 private:
    const char* kind_;
    HostStager stager_;
};

// One group of a builder: a device COO sorted by (major, minor) into compressed rows (csr_from_device_coo) and handed to the caller.  The
// buffers are kept from fetch to fetch.
struct GroupFetch {
    DevBuf<int64_t> indptr;
    DevBuf<int32_t> minor;
    DevBuf<float> vals;
    DevBuf<uint64_t> kin, kout;

    // the n > 0 records (d_major, d_minor, d_vals) of a matrix with num_major > 0 major ids; the device work counts into `timer`
    void fetch(BuilderHandle& h, EventTimer& timer, DevBuf<char>& tmp, const int32_t* d_major, const int32_t* d_minor, const float* d_vals, int64_t n,
               int num_major, int64_t* indptr_out, int32_t* keys_out, float* vals_out) {
        grow(indptr, static_cast<size_t>(num_major)); grow(minor, static_cast<size_t>(n)); grow(vals, static_cast<size_t>(n));
        timer.timed(h.stream, [&] {
            BFH_HIP(hipMemcpyAsync(minor.get(), d_minor, 4 * static_cast<size_t>(n), hipMemcpyDeviceToDevice, h.stream));   // the sort overwrites it
            csr_from_device_coo(d_major, minor.get(), d_vals, vals.get(), n, num_major, indptr.get(), kin, kout, tmp, h.stream);
        });
        h.to_host(indptr_out, indptr.get(), 8 * static_cast<size_t>(num_major));
        h.to_host(keys_out, minor.get(), 4 * static_cast<size_t>(n));
        h.to_host(vals_out, vals.get(), 4 * static_cast<size_t>(n));
    }
};

}  // namespace bfh
