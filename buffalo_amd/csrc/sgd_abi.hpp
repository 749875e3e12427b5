// The entry points BPRMF and WARP share (buffalo_hip.h declares them once per kind), written once: bpr.hip and warp.hip instantiate them for
// their handle inside `extern "C"`.
#pragma once
#include "abi.hpp"
#include "comm.hpp"
#include "sgd_base.hpp"

#define BFH_ABI_SGD(kind, Handle)                                                                                                                       \
    BFH_ABI_LIFECYCLE(kind, Handle)                                                                                                                     \
    int bfh_##kind##_init(void* h, const char* opt_json_path) {                                                                                         \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) { return x.init(opt_json_path); });                                                             \
    }                                                                                                                                                   \
    int bfh_##kind##_get_vdim(void* h) {                                                                                                                \
        return ::bfh::guarded<Handle>(h, [](Handle& x) { return x.get_vdim(); });                                                                       \
    }                                                                                                                                                   \
    int bfh_##kind##_initialize_model(void* h, float* P, int P_rows, float* Q, float* Qb, int Q_rows, int64_t num_nnz, int set_gpu) {                   \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) { x.initialize_model(P, P_rows, Q, Qb, Q_rows, num_nnz, set_gpu != 0); });                      \
    }                                                                                                                                                   \
    int bfh_##kind##_set_placeholder(void* h, const int64_t* indptr, size_t batch_size) {                                                               \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) { x.set_placeholder(indptr, batch_size); });                                                    \
    }                                                                                                                                                   \
    int bfh_##kind##_set_cumulative_table(void* h, const int64_t* table) {                                                                              \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) { x.set_cumulative_table(table); });                                                            \
    }                                                                                                                                                   \
    int bfh_##kind##_partial_update(void* h, int start_x, int next_x, const int64_t* indptr, const int32_t* keys, double* loss_sum,                     \
                                    double* n_samples) {                                                                                                \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) {                                                                                               \
            double l = 0, n = 0;                                                                                                                        \
            x.partial_update(start_x, next_x, indptr, keys, &l, &n);                                                                                    \
            if (loss_sum) *loss_sum = l;                                                                                                                \
            if (n_samples) *n_samples = n;                                                                                                              \
        });                                                                                                                                             \
    }                                                                                                                                                   \
    int bfh_##kind##_update_parameters(void* h) {                                                                                                       \
        return ::bfh::guarded<Handle>(h, [](Handle& x) { x.update_parameters(); });                                                                     \
    }                                                                                                                                                   \
    int bfh_##kind##_synchronize(void* h, int device_to_host) {                                                                                         \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) { x.synchronize(device_to_host != 0, device_to_host == 2); });                                  \
    }                                                                                                                                                   \
    int bfh_##kind##_compute_loss(void* h, int n, const int32_t* users, const int32_t* positives, const int32_t* negatives, double* loss) {             \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) { *loss = x.compute_loss(n, users, positives, negatives); });                                   \
    }                                                                                                                                                   \
    int bfh_##kind##_set_resident_csr(void* h, const int64_t* indptr, const int32_t* keys, int64_t nnz) {                                               \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) { x.set_resident_csr(indptr, keys, nnz); });                                                    \
    }                                                                                                                                                   \
    int bfh_##kind##_set_mode(void* h, const char* name, int64_t value) {                                                                               \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) { x.set_mode(name ? name : "", value); });                                                      \
    }                                                                                                                                                   \
    int bfh_##kind##_set_shard(void* h, int64_t nnz_offset, int num_shards) {                                                                           \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) { x.set_shard(nnz_offset, num_shards); });                                                      \
    }                                                                                                                                                   \
    int bfh_##kind##_device_buffer(void* h, const char* name, void** dptr, size_t* bytes) {                                                             \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) { x.device_buffer(name ? name : "", dptr, bytes); });                                           \
    }                                                                                                                                                   \
    void* bfh_##kind##_stream(void* h) { return ::bfh::stream_of(h); }                                                                                  \
    int bfh_##kind##_set_comm(void* h, void* comm) {                                                                                                    \
        return ::bfh::guarded<Handle>(h, [&](Handle& x) { x.set_comm(::bfh::as<::bfh::Comm>(comm)); });                                                 \
    }                                                                                                                                                   \
    int bfh_##kind##_comm_flush(void* h) {                                                                                                              \
        return ::bfh::guarded<Handle>(h, [](Handle& x) {                                                                                                \
            x.exchange_finish();                                                                                                                        \
            x.sync_stream();                                                                                                                            \
        });                                                                                                                                             \
    }
