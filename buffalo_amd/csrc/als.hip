// ALS on gfx950 -- C ABI.  The handle lives in als_handle.hpp, the kernels in als_kernels.hpp; CFR in cfr_impl.hpp, eALS in eals_handle.hpp / eals_kernels.hpp.
// The three handles are siblings: each derives from AlsCore (als_core.hpp) and this file calls only their public entry points.
//
// Reference semantics: CALS (/root/reference/lib/algo_impl/als/als.cc:30-358) + Algorithm::_leastsquare
// (/root/reference/lib/algo.cc:39-82) behind CuALS's object surface
// (/root/reference/include/buffalo/cuda/als/als.hpp:20-35).
#include "abi.hpp"
#include "als_handle.hpp"
#include "cfr_impl.hpp"
#include "eals_handle.hpp"

using bfh::AlsHandle;
using bfh::CfrHandle;
using bfh::EalsHandle;
using bfh::guarded;

extern "C" {

BFH_ABI_LIFECYCLE(als, AlsHandle)

int bfh_als_init(void* h, const char* opt_json_path) {
    return guarded<AlsHandle>(h, [&](AlsHandle& a) { return a.init(opt_json_path); });
}
int bfh_als_get_vdim(void* h) {
    return guarded<AlsHandle>(h, [](AlsHandle& a) { return a.vdim(); });
}
int bfh_als_initialize_model(void* h, float* P, int P_rows, float* Q, int Q_rows) {
    return guarded<AlsHandle>(h, [&](AlsHandle& a) { a.initialize_model(P, P_rows, Q, Q_rows); });
}
int bfh_als_set_placeholder(void* h, const int64_t* lindptr, const int64_t* rindptr, size_t batch_size) {
    return guarded<AlsHandle>(h, [&](AlsHandle& a) { a.set_placeholder(lindptr, rindptr, batch_size); });
}
int bfh_als_precompute(void* h, int axis) {
    return guarded<AlsHandle>(h, [&](AlsHandle& a) { a.precompute(axis); });
}
int bfh_als_partial_update(void* h, int start_x, int next_x, const int64_t* indptr, const int32_t* keys, const float* vals,
                           int axis, double* loss_nume, double* loss_deno) {
    return guarded<AlsHandle>(h, [&](AlsHandle& a) {
        double nume = 0, deno = 0;
        a.partial_update(start_x, next_x, indptr, keys, vals, axis, &nume, &deno);
        if (loss_nume) *loss_nume = nume;
        if (loss_deno) *loss_deno = deno;
    });
}
int bfh_als_set_resident_csr(void* h, int axis, const int64_t* indptr, const int32_t* keys, const float* vals, int64_t nnz) {
    return guarded<AlsHandle>(h, [&](AlsHandle& a) { a.set_resident_csr(axis, indptr, keys, vals, nnz); });
}
int bfh_als_fold_in(void* h, int axis, int n_rows, const int64_t* indptr, const int32_t* keys, const float* vals, int64_t nnz, float* out) {
    return guarded<AlsHandle>(h, [&](AlsHandle& a) { a.fold_in(axis, n_rows, indptr, keys, vals, nnz, out); });
}
int bfh_als_synchronize(void* h, int device_to_host) {
    return guarded<AlsHandle>(h, [&](AlsHandle& a) { a.synchronize(device_to_host != 0); });
}
int bfh_als_set_mode(void* h, const char* name, int64_t value) {
    return guarded<AlsHandle>(h, [&](AlsHandle& a) { a.set_mode(name ? name : "", value); });
}
int bfh_als_device_buffer(void* h, const char* name, void** dptr, size_t* bytes) {
    return guarded<AlsHandle>(h, [&](AlsHandle& a) { a.device_buffer(name ? name : "", dptr, bytes); });
}
void* bfh_als_stream(void* h) { return bfh::stream_of(h); }
int bfh_als_set_comm(void* h, void* comm) {
    return guarded<AlsHandle>(h, [&](AlsHandle& a) { a.set_comm(bfh::as<bfh::Comm>(comm)); });
}
int bfh_als_publish_rows(void* h, int axis, const int* bounds, int n_bounds) {
    return guarded<AlsHandle>(h, [&](AlsHandle& a) { a.publish_rows(axis, bounds, n_bounds); });
}

// ------------------------------------------------------------------------------------------------
// CFR -- CCFR (/root/reference/lib/algo_impl/cfr/cfr.cc) behind CyCFR's surface (buffalo/algo/_cfr.pyx:25-71)
// ------------------------------------------------------------------------------------------------
BFH_ABI_LIFECYCLE(cfr, CfrHandle)

int bfh_cfr_init(void* h, const char* opt_json_path) {
    return guarded<CfrHandle>(h, [&](CfrHandle& c) { return c.init(opt_json_path); });
}
int bfh_cfr_set_embedding(void* h, float* data, int size, const char* obj_type) {
    return guarded<CfrHandle>(h, [&](CfrHandle& c) { c.set_embedding(data, size, obj_type ? obj_type : ""); });
}
int bfh_cfr_precompute(void* h, const char* obj_type) {
    return guarded<CfrHandle>(h, [&](CfrHandle& c) { c.precompute(obj_type ? obj_type : ""); });
}
int bfh_cfr_partial_update_user(void* h, int start_x, int next_x, const int64_t* indptr, const int32_t* keys, const float* vals, double* loss) {
    return guarded<CfrHandle>(h, [&](CfrHandle& c) {
        const double v = c.partial_update_user(start_x, next_x, indptr, keys, vals);
        if (loss) *loss = v;
    });
}
int bfh_cfr_partial_update_item(void* h, int start_x, int next_x, const int64_t* indptr_u, const int32_t* keys_u, const float* vals_u,
                                const int64_t* indptr_c, const int32_t* keys_c, const float* vals_c, double* loss) {
    return guarded<CfrHandle>(h, [&](CfrHandle& c) {
        const double v = c.partial_update_item(start_x, next_x, indptr_u, keys_u, vals_u, indptr_c, keys_c, vals_c);
        if (loss) *loss = v;
    });
}
int bfh_cfr_partial_update_context(void* h, int start_x, int next_x, const int64_t* indptr, const int32_t* keys, const float* vals, double* loss) {
    return guarded<CfrHandle>(h, [&](CfrHandle& c) {
        const double v = c.partial_update_context(start_x, next_x, indptr, keys, vals);
        if (loss) *loss = v;
    });
}

// ------------------------------------------------------------------------------------------------
// eALS -- CEALS (/root/reference/lib/algo_impl/eals/eals.cc) behind CyEALS's surface (buffalo/algo/_eals.pyx:23-67)
// ------------------------------------------------------------------------------------------------
BFH_ABI_LIFECYCLE(eals, EalsHandle)

int bfh_eals_init(void* h, const char* opt_json_path) {
    return guarded<EalsHandle>(h, [&](EalsHandle& e) { return e.init(opt_json_path); });
}
int bfh_eals_initialize_model(void* h, float* P, float* Q, float* C, int P_rows, int Q_rows) {
    return guarded<EalsHandle>(h, [&](EalsHandle& e) { e.initialize_model(P, Q, C, P_rows, Q_rows); });
}
int bfh_eals_precompute_cache(void* h, int nnz, const int64_t* indptr, const int32_t* keys, int axis) {
    return guarded<EalsHandle>(h, [&](EalsHandle& e) { e.precompute_cache(nnz, indptr, keys, axis); });
}
int bfh_eals_update(void* h, const int64_t* indptr, const int32_t* keys, const float* vals, int axis) {
    return guarded<EalsHandle>(h, [&](EalsHandle& e) { return e.update(indptr, keys, vals, axis); });
}
int bfh_eals_estimate_loss(void* h, int nnz, const int64_t* indptr, const int32_t* keys, const float* vals, int axis, float* rmse, float* loss) {
    return guarded<EalsHandle>(h, [&](EalsHandle& e) {
        float r = 0.f, l = 0.f;
        e.estimate_loss(nnz, indptr, keys, vals, axis, &r, &l);
        if (rmse) *rmse = r;
        if (loss) *loss = l;
    });
}

}  // extern "C"
