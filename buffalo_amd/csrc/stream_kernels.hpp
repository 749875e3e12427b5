// Kernels of the Stream database builder (stream.hip): the name table, the token lookup, the validation splits, distinct (user, item) records
// in file order, item counts.  Line ends and token starts are text_tiles.hpp's kernels, the pair keys and the END offsets csr_kernels.hpp's.
// Integer atomics only, vector stores only.
#pragma once
#include "common.hpp"
#include "csr_kernels.hpp"
#include "text_tiles.hpp"

namespace bfh {

// FNV-1a over the bytes, then a 64-bit finalizer: the low bits pick the slot, the high word is the fingerprint kept beside the name index
constexpr uint64_t kStreamHashSeed = 0xcbf29ce484222325ull;
__host__ __device__ __forceinline__ uint64_t stream_hash_step(uint64_t h, unsigned b) { return (h ^ b) * 0x100000001b3ull; }
__host__ __device__ __forceinline__ uint64_t stream_hash_finish(uint64_t h) {
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    return h;
}

#if defined(__HIPCC__)

// the first 8 bytes of a name or token as one word (byte k in bits 8k..8k+7, zeros behind a shorter one): with equal lengths, equal words
// are equal bytes, so names of up to 8 bytes -- ordinary catalogues -- are compared by one 8-byte gather
__host__ __device__ __forceinline__ uint64_t stream_head_step(uint64_t w, unsigned b, int64_t k) { return k < 8 ? w | (static_cast<uint64_t>(b) << (8 * k)) : w; }

// name i = line i of the id file with the white space at both ends removed (str.strip(): stream.py:120-122)
__global__ __launch_bounds__(256) void stream_names_kernel(const char* __restrict__ names, int64_t bytes, const int64_t* __restrict__ eol, int64_t n_eol,
                                                           int num_names, int64_t* __restrict__ beg, int32_t* __restrict__ len,
                                                           uint64_t* __restrict__ head) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= num_names) return;
    int64_t b = i ? eol[i - 1] + 1 : 0, e = i < n_eol ? eol[i] : bytes;
    while (b < e && stream_space(static_cast<unsigned char>(names[b]))) ++b;
    while (e > b && stream_space(static_cast<unsigned char>(names[e - 1]))) --e;
    beg[i] = b;
    len[i] = static_cast<int32_t>(e - b);
    uint64_t w = 0;
    for (int64_t k = 0; k < 8 && b + k < e; ++k) w = stream_head_step(w, static_cast<unsigned char>(names[b + k]), k);
    head[i] = w;
}

__device__ __forceinline__ bool stream_same_bytes(const char* __restrict__ a, const char* __restrict__ b, int64_t n) {
    for (int64_t k = 0; k < n; ++k)
        if (a[k] != b[k]) return false;
    return true;
}

// Open addressing, linear probing; a slot holds (fingerprint << 32) | (name index + 1), 0 = empty.  One thread per name claims the first empty
// slot of its probe sequence by compare-and-swap.  Equal names walk the same sequence, so the later one meets the earlier one's slot before any
// empty slot: `dup` takes the smallest index of a name that met its equal.
__global__ __launch_bounds__(256) void stream_insert_kernel(const char* __restrict__ names, const int64_t* __restrict__ beg, const int32_t* __restrict__ len,
                                                            int num_names, unsigned long long* __restrict__ table, uint64_t mask, int* __restrict__ dup) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= num_names) return;
    const char* mine = names + beg[i];
    const int32_t n = len[i];
    uint64_t h = kStreamHashSeed;
    for (int32_t k = 0; k < n; ++k) h = stream_hash_step(h, static_cast<unsigned char>(mine[k]));
    h = stream_hash_finish(h);
    const unsigned long long fp = h >> 32, entry = (fp << 32) | static_cast<unsigned>(i + 1);
    for (uint64_t slot = h & mask;; slot = (slot + 1) & mask) {
        const unsigned long long old = atomicCAS(&table[slot], 0ull, entry);
        if (old == 0ull) return;
        if ((old >> 32) != fp) continue;
        const int j = static_cast<int>(old & 0xffffffffull) - 1;
        if (len[j] == n && stream_same_bytes(names + beg[j], mine, n)) {
            atomicMin(dup, i > j ? i : j);
            return;
        }
    }
}

// the probe counter is kStreamProbeSlots words on cache lines of their own: a wave adds to the slot of its block, the host sums them
// (one word for all waves is one serial chain of same-address atomics, longer than the rest of the kernel)
constexpr int kStreamProbeSlots = 64, kStreamProbeStride = 8;

// One thread per token: hash its bytes from its start (wherever the token ends: the next tile, the next megabyte), walk the table, write the
// 0-based item id.  A token that is no name: item -1 and `err_tok` takes the smallest such token index.
__global__ __launch_bounds__(256) void stream_lookup_kernel(const char* __restrict__ text, int64_t bytes, const int64_t* __restrict__ tok_pos, int64_t n_tok,
                                                            const char* __restrict__ names,
                                                            const int64_t* __restrict__ nbeg, const int32_t* __restrict__ nlen,
                                                            const uint64_t* __restrict__ nhead, const unsigned long long* __restrict__ table,
                                                            uint64_t mask, int32_t* __restrict__ item, unsigned long long* __restrict__ err_tok,
                                                            unsigned long long* __restrict__ probes) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    int extra = 0;
    if (t < n_tok) {
        const int64_t p = tok_pos[t];
        int64_t e = p;
        uint64_t h = kStreamHashSeed, head = 0;
        for (; e < bytes; ++e) {
            const unsigned b = static_cast<unsigned char>(text[e]);
            if (stream_space(b)) break;
            h = stream_hash_step(h, b);
            head = stream_head_step(head, b, e - p);
        }
        h = stream_hash_finish(h);
        const unsigned long long fp = h >> 32;
        int found = -1;
        for (uint64_t slot = h & mask;; slot = (slot + 1) & mask) {
            const unsigned long long ent = table[slot];
            if (ent == 0ull) break;
            if ((ent >> 32) == fp) {
                const int j = static_cast<int>(ent & 0xffffffffull) - 1;
                if (nlen[j] == e - p && nhead[j] == head && (e - p <= 8 || stream_same_bytes(names + nbeg[j] + 8, text + p + 8, e - p - 8))) {
                    found = j;
                    break;
                }
            }
            ++extra;
        }
        item[t] = found;
        if (found < 0) atomicMin(err_tok, static_cast<unsigned long long>(t));
    }
    const int total = wave_sum_i32(extra);
    if (lane_id() == 0 && total) atomicAdd(probes + (blockIdx.x % kStreamProbeSlots) * kStreamProbeStride, static_cast<unsigned long long>(total));
}

__global__ __launch_bounds__(256) void stream_fill_kernel(int64_t* __restrict__ a, int64_t n, int64_t v) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) a[i] = v;
}

// `newest` (stream.py:224-228): the last min(vali_n, max(len - 1, 0)) events of a user are held out
__global__ __launch_bounds__(256) void stream_hold_newest_kernel(const int32_t* __restrict__ user, const int64_t* __restrict__ ends, int64_t n, int vali_n,
                                                                 int64_t* __restrict__ keep) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n) return;
    const int u = user[t];
    const int64_t beg = u ? ends[u - 1] : 0, end = ends[u], len = end - beg;
    const int64_t held = len - 1 < vali_n ? (len - 1 > 0 ? len - 1 : 0) : vali_n;
    keep[t] = t < end - held ? 1 : 0;
}

// `sample` (stream.py:232-245): the events at the drawn positions are held out
__global__ __launch_bounds__(256) void stream_hold_sample_kernel(const int64_t* __restrict__ pos, int64_t n_sample, int64_t* __restrict__ keep) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (j < n_sample) keep[pos[j]] = 0;
}

// kept[] = exclusive scan of keep[]: event t goes to train slot kept[t] or to held slot t - kept[t]; both lists stay in file order
__global__ __launch_bounds__(256) void stream_split_kernel(const int32_t* __restrict__ user, const int32_t* __restrict__ item, const int64_t* __restrict__ keep,
                                                           const int64_t* __restrict__ kept, int64_t n, int32_t* __restrict__ train_user,
                                                           int32_t* __restrict__ train_item, int32_t* __restrict__ held_user, int32_t* __restrict__ held_item) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n) return;
    const int64_t k = kept[t];
    if (keep[t]) {
        train_user[k] = user[t];
        train_item[k] = item[t];
    } else {
        held_user[t - k] = user[t];
        held_item[t - k] = item[t];
    }
}

// Item counts (the `uni` of W2V.build_vocab, w2v.py:91-100).  A catalogue of up to kStreamLdsBins items (128 KB of the CU's 160 KB of LDS;
// ML-20M's 27,278 fit): one LDS histogram per block over a grid-stride share of the events, flushed once -- popular items meet in LDS, the
// global adds are spread evenly over the bins.  A larger catalogue: global atomics.  Dynamic LDS: 4 bytes per item.
constexpr int kStreamLdsBins = 32768;
constexpr int kStreamSmallBins = 8192;   // up to here several blocks share a CU

__global__ __launch_bounds__(256) void stream_counts_lds_kernel(const int32_t* __restrict__ items, int64_t n, int num_items,
                                                                unsigned long long* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned s_hist[];
    for (int i = threadIdx.x; i < num_items; i += 256) s_hist[i] = 0u;
    __syncthreads();
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < n; e += static_cast<int64_t>(gridDim.x) * 256) atomicAdd(&s_hist[items[e]], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < num_items; i += 256)
        if (s_hist[i]) atomicAdd(&counts[i], static_cast<unsigned long long>(s_hist[i]));
}

__global__ __launch_bounds__(256) void stream_counts_global_kernel(const int32_t* __restrict__ items, int64_t n, unsigned long long* __restrict__ counts) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (e < n) atomicAdd(&counts[items[e]], 1ull);
}

// ---- distinct (user, item) pairs of a list, in order of first appearance, with their counts (keys and positions: csr_pack_kernel) ----
// keys sorted: head[i] = 1 where a run of equal keys starts; head[n] = 0 so that the scan's last entry is the number of runs
__global__ __launch_bounds__(256) void stream_heads_kernel(const uint64_t* __restrict__ keys, int64_t n, int64_t* __restrict__ head) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i > n) return;
    head[i] = i < n && (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// run r (= hidx[i] at its head i): key, first position (the sort is stable: the head holds the smallest), where it starts; run_start[runs] = n
__global__ __launch_bounds__(256) void stream_runs_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ pos, const int64_t* __restrict__ head,
                                                          const int64_t* __restrict__ hidx, int64_t n, int64_t runs, uint64_t* __restrict__ run_key,
                                                          uint64_t* __restrict__ run_first, int64_t* __restrict__ run_start, int64_t* __restrict__ run_id) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == 0) run_start[runs] = n;
    if (!head[i]) return;
    const int64_t r = hidx[i];
    run_key[r] = keys[i];
    run_first[r] = static_cast<uint64_t>(pos[i]);
    run_start[r] = i;
    run_id[r] = r;
}

// order[j] = the run with the j-th smallest first position -> record j; val = the run's length, or 1 when `unit` (a list that was distinct already)
__global__ __launch_bounds__(256) void stream_emit_kernel(const int64_t* __restrict__ order, const uint64_t* __restrict__ run_key,
                                                          const int64_t* __restrict__ run_start, int64_t runs, int unit, int32_t* __restrict__ rows,
                                                          int32_t* __restrict__ cols, float* __restrict__ vals) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (j >= runs) return;
    const int64_t r = order[j];
    const uint64_t k = run_key[r];
    rows[j] = static_cast<int32_t>(k >> 32);
    cols[j] = static_cast<int32_t>(k & 0xffffffffull);
    vals[j] = unit ? 1.f : static_cast<float>(run_start[r + 1] - run_start[r]);
}

#endif  // __HIPCC__

}  // namespace bfh
