// pLSI (probabilistic latent semantic indexing, EM) on gfx950 -- kernels, handle and C ABI (bfh_plsi_*).
//
// Reference semantics: plsi::CPLSI (/root/reference/lib/algo_impl/plsi/plsi.cc) behind CyPLSI's surface
// (/root/reference/buffalo/algo/_plsi.pyx).  For every stored entry (x, c, v), plsi.cc:91-101:
//     latent_k = max(P_[x,k] * Q_[c,k], 1e-10f);  norm = sum_k latent_k;  loss -= log(norm) * v;
//     P[x,:] += latent / norm * v;  Q[c,:] += latent / norm * v
// then normalize (:107-125) and swap (:127-130).  One EM epoch reads only the OLD factors and writes only sums.
//
// Device formulation.  Both sums are one computation on the two orientations of the matrix: the new row of an "owner" is the sum over
// its entries of max(own_old * other_old[key], 1e-10) / norm * v.  `plsi_half_step_kernel` runs over the rowwise matrix for P (that
// pass also gives the loss) and over the colwise matrix for Q; the colwise matrix is the transpose of the epoch's batches, made on
// the device by the COO -> CSR path of ingest.hip.  The owner's old row and its new row live in registers, the other side is gathered
// with 16-byte loads, the new row is stored once: there is no atomic on a factor matrix and every sum has a fixed order, so an
// epoch is bit-reproducible -- run to run, for any split into batches, resident or batched.
//
// Layout: [rows, vdim] float32, vdim = ceil(d / 32) * 32.  A row is handled by a LANE GROUP of G lanes (G = 8 .. 64, a power of two with
// 4 * G * C >= vdim; lane l of the group holds columns (c * G + l) * 4 .. + 3 of chunk c < C), so a wave works on 64 / G entries per
// instruction (8 at the default d = 20).  Columns >= d are MASKED, not zero-padded: max(0, 1e-10) would put them into `norm`.
//
// Work decomposition (host-built list, a function of the row lengths only):
//   * an owner of at most 2 * (64 / G) entries is a SHORT item: one lane group walks it front to back, 64 / G owners per wave;
//   * any other owner is cut into segments of kPlsiSeg entries; a wave takes one segment, its 64 / G groups take the entries
//     round-robin and are combined by an xor butterfly (commutative at every stage, so every lane holds the same bits);
//   * an owner of more than one segment writes its partial rows into slabs that `plsi_slab_sum_kernel` adds in segment order.
//   Empty owners keep the zero that reset() wrote.
// Loss: one double per lane group, combined per wave, one double per wave in a buffer that a single block adds in a fixed order.
//
// The steps on one row (entry walk, butterfly, row normalisation) are functions of plsi_fold_kernels.hpp, shared with the fold-in kernel there
// (bfh_plsi_fold_in: rows for histories that are not in the model, Q held fixed), which therefore gives the trainer's bits.
#include <random>

#include "abi.hpp"
#include "plsi_fold_kernels.hpp"

namespace bfh {

struct PlsiLong {
    int32_t owner, slab0, count, pad;
};
struct PlsiArgs {
    const float* own_old;
    const float* other_old;
    float* own_new;
    float* slabs;
    const int32_t* keys;
    const float* vals;
    const PlsiItem* items;
    int n_short, n_seg, d, vdim;
    double* loss_part;   // one per wave (LOSS builds)
};

template <int G, int C, bool LOSS>
__global__ __launch_bounds__(256) void plsi_half_step_kernel(const PlsiArgs a) {
    constexpr int NG = 64 / G;
    const int lane = threadIdx.x & 63, lig = lane & (G - 1), grp = lane / G;
    const int w = static_cast<int>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int n_short_waves = (a.n_short + NG - 1) / NG;
    if (w >= n_short_waves + a.n_seg) return;   // wave-uniform
    const bool team = w >= n_short_waves;
    int idx, stride;
    int64_t off;
    bool active = true;
    if (team) {
        idx = a.n_short + (w - n_short_waves); off = grp; stride = NG;
    } else {
        idx = w * NG + grp; off = 0; stride = 1;
        active = idx < a.n_short;
    }
    PlsiItem it{0, -1, 0, 0};
    if (active) it = a.items[idx];

    bool in_row[C];
    float own[C][4], acc[C][4];
    bool valid[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int col = (c * G + lig) * 4;
        in_row[c] = col < a.vdim;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in_row[c]) o = *reinterpret_cast<const float4*>(a.own_old + static_cast<size_t>(it.owner) * a.vdim + col);
        own[c][0] = o.x; own[c][1] = o.y; own[c][2] = o.z; own[c][3] = o.w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            valid[c][e] = col + e < a.d;
            acc[c][e] = 0.f;
        }
    }
    double lacc = 0.0;

    plsi_walk_entries<G, C, LOSS>(own, valid, in_row, acc, lacc, a.other_old, a.keys, a.vals, it.beg + off, it.end, stride, a.vdim, lig);
    if (team) plsi_team_sum<G, C>(acc);   // the NG groups of the wave hold disjoint entries of one segment
    if (active && (!team || grp == 0)) {
        float* out = it.dest < 0 ? a.own_new + static_cast<size_t>(it.owner) * a.vdim : a.slabs + static_cast<size_t>(it.dest) * a.vdim;
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (in_row[c]) *reinterpret_cast<float4*>(out + (c * G + lig) * 4) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
    }
    if (LOSS) {   // every lane of a group holds the group's sum; groups without an item hold 0
#pragma unroll
        for (int m = G; m < 64; m <<= 1) lacc += __shfl_xor(lacc, m, 64);
        if (lane == 0) a.loss_part[w] = lacc;
    }
}

// own_new[owner] = slab[slab0] + slab[slab0 + 1] + ... in segment order; one block per split owner
__global__ __launch_bounds__(256) void plsi_slab_sum_kernel(const PlsiLong* __restrict__ longs, const float* __restrict__ slabs, float* __restrict__ own_new, int vdim) {
    const PlsiLong L = longs[blockIdx.x];
    for (int c = threadIdx.x; c < vdim; c += 256) {
        float s = slabs[static_cast<size_t>(L.slab0) * vdim + c];
        for (int k = 1; k < L.count; ++k) s += slabs[static_cast<size_t>(L.slab0 + k) * vdim + c];
        own_new[static_cast<size_t>(L.owner) * vdim + c] = s;
    }
}

// out[0] = sum of part[0, n) in a fixed order (thread t adds t, t + 256, ...; then a tree over the 256 threads); one block
__global__ __launch_bounds__(256) void plsi_loss_sum_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
        if (static_cast<int>(threadIdx.x) < m) sh[threadIdx.x] += sh[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

// rows[g] = the row that owns entry g of [e0, e1) (first x in [x0, x1) with indptr[x] > g); *bad = 1 when a key is outside [0, num_keys)
__global__ __launch_bounds__(256) void plsi_expand_rows_kernel(const int64_t* __restrict__ indptr, int x0, int x1, int64_t e0, int64_t e1,
                                                               const int32_t* __restrict__ keys, int num_keys, int32_t* __restrict__ rows, int* __restrict__ bad) {
    const int64_t g = e0 + static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (g >= e1) return;
    int lo = x0, hi = x1 - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (indptr[mid] > g) hi = mid;
        else lo = mid + 1;
    }
    rows[g] = lo;
    const int32_t k = keys[g];
    if (k < 0 || k >= num_keys) *bad = 1;
}

// plsi.cc:113-116: P[i,:] += alpha1 / d; P[i,:] /= sum(P[i,:]) -- one lane group per row
template <int G, int C>
__global__ __launch_bounds__(256) void plsi_normalize_rows_kernel(float* __restrict__ P, int rows, int d, int vdim, float add) {
    const int lig = threadIdx.x & (G - 1);
    const int64_t row = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) / G;
    if (row >= rows) return;   // uniform over the lane group
    float x[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int col = (c * G + lig) * 4;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < vdim) t = *reinterpret_cast<const float4*>(P + row * vdim + col);
        x[c][0] = t.x; x[c][1] = t.y; x[c][2] = t.z; x[c][3] = t.w;
    }
    plsi_normalize_row<G, C>(x, d, lig, add);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int col = (c * G + lig) * 4;
        if (col < vdim) *reinterpret_cast<float4*>(P + row * vdim + col) = make_float4(x[c][0], x[c][1], x[c][2], x[c][3]);
    }
}

// plsi.cc:119-122, stage 1: part[chunk][k] = sum over the chunk's rows of (Q[i,k] + add), rows i = r, r + 4, ... per thread, then the 4 threads of
// a column in a fixed order.  grid (chunks, ceil(vdim / 64)), block 256 = 4 row lanes x 64 columns.
constexpr int kPlsiColChunk = 1024;
__global__ __launch_bounds__(256) void plsi_colsum_partial_kernel(const float* __restrict__ Q, int rows, int vdim, float add, double* __restrict__ part) {
    __shared__ double sh[4][64];
    const int c = blockIdx.y * 64 + (threadIdx.x & 63), r = threadIdx.x >> 6;
    const int r0 = blockIdx.x * kPlsiColChunk, r1 = min(rows, r0 + kPlsiColChunk);
    double s = 0.0;
    if (c < vdim)
        for (int i = r0 + r; i < r1; i += 4) s += static_cast<double>(Q[static_cast<size_t>(i) * vdim + c] + add);
    sh[r][threadIdx.x & 63] = s;
    __syncthreads();
    if (r == 0 && c < vdim) part[static_cast<size_t>(blockIdx.x) * vdim + c] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}
// stage 2: colsum[k] = part[0][k] + part[1][k] + ... in chunk order
__global__ __launch_bounds__(256) void plsi_colsum_final_kernel(const double* __restrict__ part, int chunks, int vdim, double* __restrict__ colsum) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= vdim) return;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += part[static_cast<size_t>(k) * vdim + c];
    colsum[c] = s;
}
// Q[i,k] = (Q[i,k] + add) / colsum[k] for k < d
__global__ __launch_bounds__(256) void plsi_scale_cols_kernel(float* __restrict__ Q, int64_t n, int d, int vdim, float add, const double* __restrict__ colsum) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = static_cast<int>(i % vdim);
    if (c < d) Q[i] = (Q[i] + add) / static_cast<float>(colsum[c]);
}

class PlsiHandle : public HandleBase {
 public:
    ~PlsiHandle() override {
        if (stream) (void)hipStreamDestroy(stream);
    }
    bool init(const char* opt_path) {
        std::string err;
        if (!opt_.load(opt_path ? opt_path : "", &err)) {
            last_error = err;
            return false;
        }
        d_ = opt_.integer("d");
        BFH_REQUIRE(d_ >= 1, "option d must be at least 1");
        BFH_REQUIRE(d_ <= 1024, "pLSI: d > 1024 is not supported by the gfx950 kernels");
        seed_ = static_cast<uint32_t>(static_cast<int64_t>(opt_.num_or("random_seed", 0)));
        vdim_ = vdim_of(d_);
        // lane group: the smallest power of two >= vdim / 4, at least 8; beyond 64 lanes a lane holds C chunks
        G_ = lane_group_of(vdim_);
        C_ = 1;
        while (G_ * 4 * C_ < vdim_) C_ *= 2;
        BFH_HIP(hipSetDevice(device));
        if (!stream) BFH_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        loss_dev_.resize(1, true, stream);
        bad_.resize(1, true, stream);
        BFH_HIP(hipStreamSynchronize(stream));
        inited_ = true;
        model_ = false;
        return true;
    }

    // plsi.cc:42-70.  The reference's stream is not defined (one mt19937 shared by an OpenMP loop); the distribution is: |N(0, 1/d)|, rows of P and
    // columns of Q scaled to sum 1.  Here: one mt19937(seed), P row by row, then Q column by column.
    void initialize_model(float* P, int P_rows, float* Q, int Q_rows) {
        BFH_REQUIRE(inited_, "initialize_model called before init");
        BFH_REQUIRE(P && Q && P_rows > 0 && Q_rows > 0, "initialize_model: null array or empty shape");
        P_host_ = P; Q_host_ = Q; P_rows_ = P_rows; Q_rows_ = Q_rows;
        if (!keep_init_) {
            std::mt19937 rng(seed_);
            std::normal_distribution<float> dist(0.f, 1.0f / static_cast<float>(d_));
            for (int u = 0; u < P_rows; ++u) {
                float* row = P + static_cast<size_t>(u) * d_;
                float s = 0.f;
                for (int k = 0; k < d_; ++k) s += (row[k] = std::fabs(dist(rng)));
                for (int k = 0; k < d_; ++k) row[k] /= s;
            }
            std::vector<double> colsum(d_, 0.0);
            for (int k = 0; k < d_; ++k)
                for (int i = 0; i < Q_rows; ++i) colsum[k] += (Q[static_cast<size_t>(i) * d_ + k] = std::fabs(dist(rng)));
            for (int i = 0; i < Q_rows; ++i)
                for (int k = 0; k < d_; ++k) Q[static_cast<size_t>(i) * d_ + k] /= static_cast<float>(colsum[k]);
        }
        for (int s = 0; s < 2; ++s) {
            Pd_[s].resize(static_cast<size_t>(P_rows) * vdim_, true, stream);
            Qd_[s].resize(static_cast<size_t>(Q_rows) * vdim_, true, stream);
        }
        old_ = 0;
        indptr_.resize(P_rows);
        colparts_.resize(static_cast<size_t>((Q_rows + kPlsiColChunk - 1) / kPlsiColChunk) * vdim_);
        colsum_.resize(vdim_);
        tindptr_.resize(Q_rows);
        model_ = true;
        fold_.rows = 0;   // the rows of an earlier fold_in belong to the model they were folded against
        drop_resident();
        upload_model();
        clean_ = false;
    }

    void upload_model() {
        BFH_REQUIRE(model_, "synchronize before initialize_model");
        // [rows, d] -> [rows, vdim]; the pad columns stay zero
        stats.h2d_bytes += rows_to_device(Pd_[old_].get(), vdim_, P_host_, d_, 0, P_rows_, stream);
        stats.h2d_bytes += rows_to_device(Qd_[old_].get(), vdim_, Q_host_, d_, 0, Q_rows_, stream);
        BFH_HIP(hipStreamSynchronize(stream));
    }
    void download_model() {
        BFH_REQUIRE(model_, "synchronize before initialize_model");
        const int slot = t_copy_.begin(stream);
        stats.d2h_bytes += rows_to_host(P_host_, d_, Pd_[old_].get(), vdim_, 0, P_rows_, stream);
        stats.d2h_bytes += rows_to_host(Q_host_, d_, Qd_[old_].get(), vdim_, 0, Q_rows_, stream);
        t_copy_.end(slot, stream);
        BFH_HIP(hipStreamSynchronize(stream));
        copy_ms_ += t_copy_.drain();
    }

    // plsi.cc:38-40; the epoch's batch list goes with the accumulators
    void reset() {
        BFH_REQUIRE(model_, "reset before initialize_model");
        BFH_HIP(hipMemsetAsync(Pd_[1 - old_].get(), 0, Pd_[1 - old_].bytes(), stream));
        BFH_HIP(hipMemsetAsync(Qd_[1 - old_].get(), 0, Qd_[1 - old_].bytes(), stream));
        BFH_HIP(hipStreamSynchronize(stream));
        have_batches_ = false;
        updated_ = false;
        transposed_ = false;
        clean_ = true;
    }

    // plsi.cc:72-105 -- the P half-step over rows [start_x, next_x); the batch stays on the device for the Q half-step at normalize()
    float partial_update(int start_x, int next_x, const int64_t* indptr, const int32_t* keys, const float* vals) {
        BFH_REQUIRE(model_, "partial_update before initialize_model");
        BFH_REQUIRE(!resident_, "partial_update with a resident matrix set: call update_resident (set_mode(\"resident\", 0) drops the matrix)");
        BFH_REQUIRE(clean_, "partial_update: reset() has not been called since the last swap / initialize_model");
        BFH_REQUIRE(indptr, "partial_update: null indptr");
        BFH_REQUIRE(0 <= start_x && start_x <= next_x && next_x <= P_rows_, "partial_update: bad row range (next_x beyond the rows of P?)");
        BFH_REQUIRE(!have_batches_ || start_x == x1_, "partial_update: the batches of an epoch must be consecutive row ranges");
        if (next_x == start_x) return 0.f;
        const int64_t total = indptr[P_rows_ - 1];
        const int64_t e0 = start_x == 0 ? 0 : indptr[start_x - 1], e1 = indptr[next_x - 1];
        BFH_REQUIRE(0 <= e0 && e0 <= e1 && e1 <= total, "partial_update: indptr is not a non-decreasing list of END offsets");
        BFH_REQUIRE(e1 == e0 || (keys && vals), "partial_update: null keys / vals");
        reserve_entries(total);
        BFH_HIP(hipMemcpyAsync(indptr_.get() + start_x, indptr + start_x, sizeof(int64_t) * (next_x - start_x), hipMemcpyHostToDevice, stream));
        if (e1 > e0) {
            BFH_HIP(hipMemcpyAsync(keys_.get() + e0, keys, sizeof(int32_t) * (e1 - e0), hipMemcpyHostToDevice, stream));
            BFH_HIP(hipMemcpyAsync(vals_.get() + e0, vals, sizeof(float) * (e1 - e0), hipMemcpyHostToDevice, stream));
        }
        stats.h2d_bytes += 8.0 * (next_x - start_x) + 8.0 * (e1 - e0);
        expand_and_check(start_x, next_x, e0, e1);
        build_items(indptr, start_x, next_x, wl_p_);
        upload_items(wl_p_);
        const float loss = half_step(true, wl_p_, keys_.get(), vals_.get());
        if (!have_batches_) { x0_ = start_x; e0_ = e0; }
        x1_ = next_x; e1_ = e1;
        have_batches_ = true;
        transposed_ = false;
        return loss;
    }

    // the whole rowwise matrix stays in HBM, with its transpose and both work lists: built once, used every epoch
    void set_resident_csr(const int64_t* indptr, const int32_t* keys, const float* vals, int64_t nnz) {
        BFH_REQUIRE(model_, "set_resident_csr before initialize_model");
        BFH_REQUIRE(indptr && keys && vals && nnz > 0, "set_resident_csr: null array or empty matrix");
        BFH_REQUIRE(indptr[P_rows_ - 1] == nnz, "set_resident_csr: indptr[rows - 1] differs from nnz");
        drop_resident();
        reserve_entries(nnz);
        BFH_HIP(hipMemcpyAsync(indptr_.get(), indptr, sizeof(int64_t) * P_rows_, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(keys_.get(), keys, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(vals_.get(), vals, sizeof(float) * nnz, hipMemcpyHostToDevice, stream));
        stats.h2d_bytes += 8.0 * P_rows_ + 8.0 * nnz;
        expand_and_check(0, P_rows_, 0, nnz);
        build_items(indptr, 0, P_rows_, wl_p_);
        upload_items(wl_p_);
        x0_ = 0; x1_ = P_rows_; e0_ = 0; e1_ = nnz;
        transpose();
        resident_ = true;
    }
    float update_resident() {
        BFH_REQUIRE(model_, "update_resident before initialize_model");
        BFH_REQUIRE(resident_, "update_resident before set_resident_csr");
        BFH_REQUIRE(clean_, "update_resident: reset() has not been called since the last swap / initialize_model");
        const float loss = half_step(true, wl_p_, keys_.get(), vals_.get());
        updated_ = true;
        return loss;
    }

    // the Q half-step over the transpose of what the epoch has seen, then plsi.cc:107-125
    void normalize(float alpha1, float alpha2) {
        BFH_REQUIRE(model_, "normalize before initialize_model");
        BFH_REQUIRE(resident_ ? updated_ : have_batches_, "normalize: no batch seen since reset() (partial_update / update_resident first)");
        if (e1_ > e0_) {
            if (!resident_ && !transposed_) transpose();   // a second normalize() of an epoch (after "raw_accumulators") reuses it
            half_step(false, wl_q_, tkeys_, tvals_.get());
        }
        if (raw_) {   // tests read the accumulators before the normalisation
            BFH_HIP(hipStreamSynchronize(stream));
            return;
        }
        const int slot = t_norm_.begin(stream);
        float* Pn = Pd_[1 - old_].get();
        float* Qn = Qd_[1 - old_].get();
        const float a1 = alpha1 / static_cast<float>(d_), a2 = alpha2 / static_cast<float>(Q_rows_);
        const unsigned pblocks = static_cast<unsigned>((static_cast<int64_t>(P_rows_) * G_ + 255) / 256);
#define BFH_PN(GG, CC) hipLaunchKernelGGL((plsi_normalize_rows_kernel<GG, CC>), dim3(pblocks), dim3(256), 0, stream, Pn, P_rows_, d_, vdim_, a1)
        dispatch_gc([&] { BFH_PN(8, 1); }, [&] { BFH_PN(16, 1); }, [&] { BFH_PN(32, 1); }, [&] { BFH_PN(64, 1); }, [&] { BFH_PN(64, 2); }, [&] { BFH_PN(64, 4); });
#undef BFH_PN
        const int chunks = (Q_rows_ + kPlsiColChunk - 1) / kPlsiColChunk;
        hipLaunchKernelGGL(plsi_colsum_partial_kernel, dim3(chunks, (vdim_ + 63) / 64), dim3(256), 0, stream, Qn, Q_rows_, vdim_, a2, colparts_.get());
        hipLaunchKernelGGL(plsi_colsum_final_kernel, dim3((vdim_ + 255) / 256), dim3(256), 0, stream, colparts_.get(), chunks, vdim_, colsum_.get());
        const int64_t n = static_cast<int64_t>(Q_rows_) * vdim_;
        hipLaunchKernelGGL(plsi_scale_cols_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, Qn, n, d_, vdim_, a2, colsum_.get());
        BFH_HIP(hipGetLastError());
        t_norm_.end(slot, stream);
        BFH_HIP(hipStreamSynchronize(stream));
        norm_ms_ += t_norm_.drain();
    }

    // plsi.cc:127-130: old <- new; the caller's arrays hold the new model when this returns
    void swap() {
        BFH_REQUIRE(model_, "swap before initialize_model");
        old_ = 1 - old_;
        clean_ = false;
        download_model();
    }

    // ---- fold-in: topic rows for histories that are not in the model (bfh_plsi_fold_in) ------------------------------------------------
    // out[b] = the row after `iters` EM steps over history b with the old Q held fixed, from init[b] (or 1 / d): bit for bit what `iters`
    // epochs of the trainer give that row when Q is put back after each (plsi_fold_kernels.hpp).  Steps: refuse bad input on the host ->
    // work items from the row lengths -> upload -> one launch -> copy out.  Everything it writes is its own (FoldState); of the training
    // state it reads Qd_[old_] and d_ / vdim_ / G_ / C_, so it may be called anywhere in an epoch.
    void fold_in(int n_rows, const int64_t* indptr, const int32_t* keys, const float* vals, int64_t nnz, int iters, float alpha1, const float* init,
                 float* out, double* loss, double* kernel_ms) {
        BFH_REQUIRE(model_, "fold_in before initialize_model");
        fold_check(n_rows, indptr, keys, vals, nnz, iters, alpha1);
        FoldState& f = fold_;
        f.rows = n_rows;
        if (kernel_ms) *kernel_ms = 0.0;
        if (n_rows == 0) return;
        const int n_short = fold_items(n_rows, indptr);
        const int NG = 64 / G_;
        const int waves = (n_short + NG - 1) / NG + (n_rows - n_short);
        const size_t nout = static_cast<size_t>(n_rows) * vdim_;
        grow(f.out, nout);
        grow(f.items, static_cast<size_t>(n_rows));
        grow(f.keys, static_cast<size_t>(std::max<int64_t>(nnz, 1)));
        grow(f.vals, static_cast<size_t>(std::max<int64_t>(nnz, 1)));
        BFH_HIP(hipMemcpyAsync(f.items.get(), f.host_items.data(), n_rows * sizeof(PlsiItem), hipMemcpyHostToDevice, stream));
        stats.h2d_bytes += static_cast<double>(n_rows * sizeof(PlsiItem));
        if (nnz) {
            BFH_HIP(hipMemcpyAsync(f.keys.get(), keys, nnz * sizeof(int32_t), hipMemcpyHostToDevice, stream));
            BFH_HIP(hipMemcpyAsync(f.vals.get(), vals, nnz * sizeof(float), hipMemcpyHostToDevice, stream));
            stats.h2d_bytes += 8.0 * nnz;
        }
        if (init) {
            grow(f.init, nout);
            stats.h2d_bytes += rows_to_device(f.init.get(), vdim_, init, d_, 0, n_rows, stream);   // the pad columns are never read
        }
        if (loss) grow(f.loss, static_cast<size_t>(n_rows));
        PlsiFoldArgs a{};
        a.Q = Qd_[old_].get();
        a.init = init ? f.init.get() : nullptr;
        a.out = f.out.get();
        a.loss = loss ? f.loss.get() : nullptr;
        a.keys = f.keys.get(); a.vals = f.vals.get(); a.items = f.items.get();
        a.n_short = n_short; a.n_team = n_rows - n_short; a.d = d_; a.vdim = vdim_; a.iters = iters;
        a.a1 = alpha1 / static_cast<float>(d_);
        a.uniform = 1.0f / static_cast<float>(d_);
        const dim3 grid(static_cast<unsigned>((waves + 3) / 4));
        const int slot = f.t_fold.begin(stream);
#define BFH_FOLD(GG, CC)                                                                                         \
    do {                                                                                                         \
        if (loss) hipLaunchKernelGGL((plsi_fold_kernel<GG, CC, true>), grid, dim3(256), 0, stream, a);           \
        else hipLaunchKernelGGL((plsi_fold_kernel<GG, CC, false>), grid, dim3(256), 0, stream, a);               \
    } while (0)
        dispatch_gc([&] { BFH_FOLD(8, 1); }, [&] { BFH_FOLD(16, 1); }, [&] { BFH_FOLD(32, 1); }, [&] { BFH_FOLD(64, 1); }, [&] { BFH_FOLD(64, 2); },
                    [&] { BFH_FOLD(64, 4); });
#undef BFH_FOLD
        BFH_HIP(hipGetLastError());
        f.t_fold.end(slot, stream);
        if (out) stats.d2h_bytes += rows_to_host(out, d_, f.out.get(), vdim_, 0, n_rows, stream);
        if (loss) {
            BFH_HIP(hipMemcpyAsync(loss, f.loss.get(), n_rows * sizeof(double), hipMemcpyDeviceToHost, stream));
            stats.d2h_bytes += 8.0 * n_rows;
        }
        BFH_HIP(hipStreamSynchronize(stream));
        const double ms = f.t_fold.drain();
        if (kernel_ms) *kernel_ms = ms;
        stats.launches += 1;
        stats.exchanges += 1;
        stats.accepted += n_rows;
        stats.loaded_rows += nnz * iters;
    }

    void set_mode(const std::string& name, int64_t value) {
        if (name == "keep_init") keep_init_ = value != 0;          // initialize_model uploads the caller's arrays as they are
        else if (name == "raw_accumulators") raw_ = value != 0;    // normalize() stops after the Q half-step
        else if (name == "resident") {
            BFH_REQUIRE(value == 0, "resident: only 0 (drop the resident matrix) can be set; set_resident_csr makes one");
            drop_resident();
        } else if (name == "timing") timing = value != 0;
        else throw Error(BFH_ERR_INVALID, "unknown mode '" + name + "' (keep_init, raw_accumulators, resident, timing)");
    }

    void device_buffer(const std::string& name, void** ptr, size_t* bytes) {
        DevBuf<float>* b = nullptr;
        if (name == "fold") {   // the rows of the last fold_in (which returned with the stream drained)
            *ptr = fold_.rows ? fold_.out.get() : nullptr;
            *bytes = static_cast<size_t>(fold_.rows) * vdim_ * sizeof(float);
            return;
        }
        if (name == "P") b = &Pd_[old_];
        else if (name == "Q") b = &Qd_[old_];
        else if (name == "P_new") b = &Pd_[1 - old_];
        else if (name == "Q_new") b = &Qd_[1 - old_];
        else throw Error(BFH_ERR_INVALID, "unknown device buffer '" + name + "' (P, Q: the old model; P_new, Q_new: the accumulators; fold: the rows of the last fold_in)");
        *ptr = b->get();
        *bytes = b->bytes();
    }

    // the phases of an epoch in the fields of bfh_stats (buffalo_hip.h lists the mapping)
    void refresh_stats() override {
        stats.kernel_ms = p_ms_; stats.optimizer_ms = q_ms_; stats.aux_ms = tr_ms_; stats.exchange_kernel_ms = norm_ms_; stats.allreduce_ms = copy_ms_;
    }
    void clear_accumulators() override { p_ms_ = q_ms_ = tr_ms_ = norm_ms_ = copy_ms_ = 0.0; }
    int vdim() const { return vdim_; }

 private:
    struct WorkList {
        std::vector<PlsiItem> items;   // short items first
        std::vector<PlsiLong> longs;
        int n_short = 0, n_seg = 0, n_slabs = 0;
        DevBuf<PlsiItem> d_items;
        DevBuf<PlsiLong> d_longs;
    };

    template <typename F0, typename F1, typename F2, typename F3, typename F4, typename F5>
    void dispatch_gc(F0 f0, F1 f1, F2 f2, F3 f3, F4 f4, F5 f5) {
        if (G_ == 8) f0();
        else if (G_ == 16) f1();
        else if (G_ == 32) f2();
        else if (C_ == 1) f3();
        else if (C_ == 2) f4();
        else f5();
    }

    void drop_resident() {
        resident_ = false;
        have_batches_ = false;
        updated_ = false;
    }
    void reserve_entries(int64_t total) {
        const size_t need = static_cast<size_t>(std::max<int64_t>(total, 1));
        if (keys_.size() < need) {
            BFH_REQUIRE(!have_batches_, "partial_update: indptr[rows - 1] grew inside an epoch");
            keys_.resize(need); vals_.resize(need); trows_.resize(need); tvals_.resize(need);
        }
    }
    void expand_and_check(int x0, int x1, int64_t e0, int64_t e1) {
        if (e1 == e0) return;
        BFH_HIP(hipMemsetAsync(bad_.get(), 0, sizeof(int), stream));
        hipLaunchKernelGGL(plsi_expand_rows_kernel, dim3(static_cast<unsigned>((e1 - e0 + 255) / 256)), dim3(256), 0, stream, indptr_.get(), x0, x1, e0, e1,
                           keys_.get(), Q_rows_, trows_.get(), bad_.get());
        BFH_HIP(hipGetLastError());
        int bad = 0;
        BFH_HIP(hipMemcpyAsync(&bad, bad_.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        BFH_REQUIRE(!bad, "keys outside [0, rows of Q): the matrix has more columns than the model has items");
    }

    // owners [x0, x1) of a matrix given by END offsets -> items.  Depends on the owners' lengths alone.
    void build_items(const int64_t* ends, int x0, int x1, WorkList& wl) {
        const int NG = 64 / G_;
        const int64_t short_max = NG > 1 ? 2 * NG : 0;
        wl.items.clear(); wl.longs.clear();
        std::vector<PlsiItem> segs;
        int slabs = 0;
        for (int x = x0; x < x1; ++x) {
            const int64_t beg = x == 0 ? 0 : ends[x - 1], end = ends[x];
            BFH_REQUIRE(end >= beg, "indptr is not a non-decreasing list of END offsets");
            const int64_t n = end - beg;
            if (n == 0) continue;
            if (n <= short_max) wl.items.push_back({x, -1, beg, end});
            else if (n <= kPlsiSeg) segs.push_back({x, -1, beg, end});
            else {
                const int cnt = static_cast<int>((n + kPlsiSeg - 1) / kPlsiSeg);
                wl.longs.push_back({x, slabs, cnt, 0});
                for (int k = 0; k < cnt; ++k) segs.push_back({x, slabs + k, beg + static_cast<int64_t>(k) * kPlsiSeg, std::min(end, beg + static_cast<int64_t>(k + 1) * kPlsiSeg)});
                slabs += cnt;
            }
        }
        wl.n_short = static_cast<int>(wl.items.size());
        wl.n_seg = static_cast<int>(segs.size());
        wl.n_slabs = slabs;
        wl.items.insert(wl.items.end(), segs.begin(), segs.end());
    }
    void upload_items(WorkList& wl) {
        if (wl.d_items.size() < wl.items.size()) wl.d_items.resize(wl.items.size());
        if (wl.d_longs.size() < wl.longs.size()) wl.d_longs.resize(wl.longs.size());
        if (!wl.items.empty()) BFH_HIP(hipMemcpyAsync(wl.d_items.get(), wl.items.data(), wl.items.size() * sizeof(PlsiItem), hipMemcpyHostToDevice, stream));
        if (!wl.longs.empty()) BFH_HIP(hipMemcpyAsync(wl.d_longs.get(), wl.longs.data(), wl.longs.size() * sizeof(PlsiLong), hipMemcpyHostToDevice, stream));
        BFH_HIP(hipStreamSynchronize(stream));   // the vectors may change after this
        stats.h2d_bytes += static_cast<double>(wl.items.size() * sizeof(PlsiItem) + wl.longs.size() * sizeof(PlsiLong));
    }

    // colwise matrix of entries [e0_, e1_): tindptr_ (END offsets, 0-based), tkeys_ (rows, ascending inside a column), tvals_
    void transpose() {
        const int64_t n = e1_ - e0_;
        const int slot = t_tr_.begin(stream);
        tkeys_ = trows_.get() + e0_;
        csr_from_device_coo(keys_.get() + e0_, tkeys_, vals_.get() + e0_, tvals_.get(), n, Q_rows_, tindptr_.get(), sort_in_, sort_out_, sort_tmp_, stream);
        t_tr_.end(slot, stream);
        tindptr_host_.resize(Q_rows_);
        BFH_HIP(hipMemcpyAsync(tindptr_host_.data(), tindptr_.get(), sizeof(int64_t) * Q_rows_, hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        tr_ms_ += t_tr_.drain();
        stats.d2h_bytes += 8.0 * Q_rows_;
        build_items(tindptr_host_.data(), 0, Q_rows_, wl_q_);
        upload_items(wl_q_);
        transposed_ = true;
    }

    // one half-step over a work list; `p_side`: own = P, other = Q, with the loss
    float half_step(bool p_side, WorkList& wl, const int32_t* keys, const float* vals) {
        const int total = wl.n_short + wl.n_seg;
        if (total == 0) return 0.f;
        const int NG = 64 / G_;
        const int waves = (wl.n_short + NG - 1) / NG + wl.n_seg;
        if (slabs_.size() < static_cast<size_t>(wl.n_slabs) * vdim_) slabs_.resize(static_cast<size_t>(wl.n_slabs) * vdim_);
        if (p_side && loss_part_.size() < static_cast<size_t>(waves)) loss_part_.resize(waves);
        PlsiArgs a{};
        a.own_old = (p_side ? Pd_ : Qd_)[old_].get();
        a.other_old = (p_side ? Qd_ : Pd_)[old_].get();
        a.own_new = (p_side ? Pd_ : Qd_)[1 - old_].get();
        a.slabs = slabs_.get();
        a.keys = keys; a.vals = vals; a.items = wl.d_items.get();
        a.n_short = wl.n_short; a.n_seg = wl.n_seg; a.d = d_; a.vdim = vdim_;
        a.loss_part = loss_part_.get();
        EventTimer& t = p_side ? t_p_ : t_q_;
        const int slot = t.begin(stream);
        const dim3 grid(static_cast<unsigned>((waves + 3) / 4));
#define BFH_HS(GG, CC)                                                                                                  \
    do {                                                                                                                \
        if (p_side) hipLaunchKernelGGL((plsi_half_step_kernel<GG, CC, true>), grid, dim3(256), 0, stream, a);           \
        else hipLaunchKernelGGL((plsi_half_step_kernel<GG, CC, false>), grid, dim3(256), 0, stream, a);                 \
    } while (0)
        dispatch_gc([&] { BFH_HS(8, 1); }, [&] { BFH_HS(16, 1); }, [&] { BFH_HS(32, 1); }, [&] { BFH_HS(64, 1); }, [&] { BFH_HS(64, 2); }, [&] { BFH_HS(64, 4); });
#undef BFH_HS
        BFH_HIP(hipGetLastError());
        if (!wl.longs.empty()) {
            hipLaunchKernelGGL(plsi_slab_sum_kernel, dim3(static_cast<unsigned>(wl.longs.size())), dim3(256), 0, stream, wl.d_longs.get(), slabs_.get(), a.own_new, vdim_);
            BFH_HIP(hipGetLastError());
        }
        double loss = 0.0;
        if (p_side) {
            hipLaunchKernelGGL(plsi_loss_sum_kernel, dim3(1), dim3(256), 0, stream, loss_part_.get(), waves, loss_dev_.get());
            BFH_HIP(hipGetLastError());
        }
        t.end(slot, stream);
        if (p_side) BFH_HIP(hipMemcpyAsync(&loss, loss_dev_.get(), sizeof(double), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        (p_side ? p_ms_ : q_ms_) += t.drain();
        stats.launches += 1;
        stats.samples += p_side ? wl_entries(wl) : 0;
        stats.loaded_rows += wl_entries(wl);
        stats.merges += static_cast<int64_t>(wl.longs.size());
        return static_cast<float>(loss);
    }
    static int64_t wl_entries(const WorkList& wl) {
        int64_t n = 0;
        for (const PlsiItem& it : wl.items) n += it.end - it.beg;
        return n;
    }

    // Everything bfh_plsi_fold_in refuses, before anything is uploaded or launched.  The key check is a host scan of all nnz keys: serving
    // input is not trusted, and an out-of-range key must never reach a gather.
    void fold_check(int n_rows, const int64_t* indptr, const int32_t* keys, const float* vals, int64_t nnz, int iters, float alpha1) const {
        BFH_REQUIRE(n_rows >= 0, "fold_in: n_rows is negative");
        BFH_REQUIRE(nnz >= 0, "fold_in: nnz is negative");
        BFH_REQUIRE(iters >= 1 && iters <= 10000, "fold_in: iters must be in [1, 10000]");
        BFH_REQUIRE(std::isfinite(alpha1) && alpha1 >= 0.f, "fold_in: alpha1 must be finite and not negative");
        BFH_REQUIRE(n_rows == 0 || indptr, "fold_in: null indptr");
        BFH_REQUIRE(nnz == 0 || (keys && vals), "fold_in: null keys / vals with nnz > 0");
        int64_t prev = 0;
        for (int b = 0; b < n_rows; ++b) {
            BFH_REQUIRE(indptr[b] >= prev, "fold_in: indptr decreases at row " + std::to_string(b));
            prev = indptr[b];
        }
        BFH_REQUIRE(prev == nnz, "fold_in: indptr[n_rows - 1] != nnz");
        for (int64_t i = 0; i < nnz; ++i)
            if (keys[i] < 0 || keys[i] >= Q_rows_)
                throw Error(BFH_ERR_INVALID, "fold_in: key " + std::to_string(keys[i]) + " at position " + std::to_string(i) + " is outside [0, " +
                                                 std::to_string(Q_rows_) + ")");
    }

    // The call's rows as work items in fold_.host_items -> the number of short ones, which come first.  A row's class follows from its length by
    // build_items' rule (at most 2 * (64 / G) entries, or none: one lane group; otherwise a wave, which walks the segments in order); the rows
    // of a wave each come longest first, which shortens the tail of the launch and changes no bit.
    int fold_items(int n_rows, const int64_t* ends) {
        const int NG = 64 / G_;
        const int64_t short_max = NG > 1 ? 2 * NG : 0;
        std::vector<PlsiItem>& items = fold_.host_items;
        items.clear();
        std::vector<PlsiItem> teams;
        for (int b = 0; b < n_rows; ++b) {
            const int64_t beg = b == 0 ? 0 : ends[b - 1], end = ends[b];
            (end - beg <= short_max ? items : teams).push_back({b, -1, beg, end});
        }
        const int n_short = static_cast<int>(items.size());
        std::stable_sort(teams.begin(), teams.end(), [](const PlsiItem& x, const PlsiItem& y) { return x.end - x.beg > y.end - y.beg; });
        items.insert(items.end(), teams.begin(), teams.end());
        return n_short;
    }

    Options opt_;
    int d_ = 0, vdim_ = 0, G_ = 8, C_ = 1;
    uint32_t seed_ = 0;
    bool inited_ = false, model_ = false, keep_init_ = false, raw_ = false;
    bool clean_ = false, have_batches_ = false, resident_ = false, updated_ = false, transposed_ = false;
    float* P_host_ = nullptr;
    float* Q_host_ = nullptr;
    int P_rows_ = 0, Q_rows_ = 0, old_ = 0;
    DevBuf<float> Pd_[2], Qd_[2];   // [old_]: the old model, [1 - old_]: the accumulators / new model
    int x0_ = 0, x1_ = 0;           // rows and entries the epoch has seen
    int64_t e0_ = 0, e1_ = 0;
    DevBuf<int64_t> indptr_, tindptr_;
    DevBuf<int32_t> keys_, trows_;
    DevBuf<float> vals_, tvals_, slabs_;
    int32_t* tkeys_ = nullptr;
    std::vector<int64_t> tindptr_host_;
    DevBuf<uint64_t> sort_in_, sort_out_;
    DevBuf<char> sort_tmp_;
    DevBuf<double> loss_part_, loss_dev_, colparts_, colsum_;
    DevBuf<int> bad_;
    WorkList wl_p_, wl_q_;
    // fold_in's own state: nothing here is read or written by a training call, nothing of the training state above is written by fold_in
    struct FoldState {
        int rows = 0;                      // rows of the last call: what device buffer "fold" holds
        DevBuf<float> out;                 // [rows, vdim]: device buffer "fold"
        DevBuf<float> init;                // [rows, vdim]: the caller's start rows
        DevBuf<int32_t> keys;
        DevBuf<float> vals;
        DevBuf<double> loss;               // [rows]
        DevBuf<PlsiItem> items;
        std::vector<PlsiItem> host_items;
        EventTimer t_fold;
    };
    FoldState fold_;
    EventTimer t_p_, t_q_, t_tr_, t_norm_, t_copy_;
    double p_ms_ = 0, q_ms_ = 0, tr_ms_ = 0, norm_ms_ = 0, copy_ms_ = 0;
};

}  // namespace bfh

using bfh::guarded;
using bfh::PlsiHandle;

extern "C" {

BFH_ABI_LIFECYCLE(plsi, PlsiHandle)

int bfh_plsi_init(void* h, const char* opt_json_path) {
    return guarded<PlsiHandle>(h, [&](PlsiHandle& p) { return p.init(opt_json_path); });
}
int bfh_plsi_get_vdim(void* h) {
    return guarded<PlsiHandle>(h, [](PlsiHandle& p) { return p.vdim(); });
}
int bfh_plsi_initialize_model(void* h, float* P, int P_rows, float* Q, int Q_rows) {
    return guarded<PlsiHandle>(h, [&](PlsiHandle& p) { p.initialize_model(P, P_rows, Q, Q_rows); });
}
int bfh_plsi_synchronize(void* h, int device_to_host) {
    return guarded<PlsiHandle>(h, [&](PlsiHandle& p) {
        if (device_to_host) p.download_model();
        else p.upload_model();
    });
}
int bfh_plsi_reset(void* h) {
    return guarded<PlsiHandle>(h, [](PlsiHandle& p) { p.reset(); });
}
int bfh_plsi_partial_update(void* h, int start_x, int next_x, const int64_t* indptr, const int32_t* keys, const float* vals, float* loss) {
    return guarded<PlsiHandle>(h, [&](PlsiHandle& p) {
        const float v = p.partial_update(start_x, next_x, indptr, keys, vals);
        if (loss) *loss = v;
    });
}
int bfh_plsi_set_resident_csr(void* h, const int64_t* indptr, const int32_t* keys, const float* vals, int64_t nnz) {
    return guarded<PlsiHandle>(h, [&](PlsiHandle& p) { p.set_resident_csr(indptr, keys, vals, nnz); });
}
int bfh_plsi_update_resident(void* h, float* loss) {
    return guarded<PlsiHandle>(h, [&](PlsiHandle& p) {
        const float v = p.update_resident();
        if (loss) *loss = v;
    });
}
int bfh_plsi_normalize(void* h, float alpha1, float alpha2) {
    return guarded<PlsiHandle>(h, [&](PlsiHandle& p) { p.normalize(alpha1, alpha2); });
}
int bfh_plsi_swap(void* h) {
    return guarded<PlsiHandle>(h, [](PlsiHandle& p) { p.swap(); });
}
int bfh_plsi_fold_in(void* h, int n_rows, const int64_t* indptr, const int32_t* keys, const float* vals, int64_t nnz, int iters, float alpha1,
                     const float* init, float* out, double* loss, double* kernel_ms) {
    return guarded<PlsiHandle>(h, [&](PlsiHandle& p) { p.fold_in(n_rows, indptr, keys, vals, nnz, iters, alpha1, init, out, loss, kernel_ms); });
}
int bfh_plsi_set_mode(void* h, const char* name, int64_t value) {
    return guarded<PlsiHandle>(h, [&](PlsiHandle& p) { p.set_mode(name ? name : "", value); });
}
int bfh_plsi_device_buffer(void* h, const char* name, void** ptr, size_t* bytes) {
    return guarded<PlsiHandle>(h, [&](PlsiHandle& p) { p.device_buffer(name ? name : "", ptr, bytes); });
}

}  // extern "C"
