// Device-resident state shared by the BPRMF and WARP backends: the GPU counterpart of
// SGDAlgorithm (/root/reference/include/buffalo/algo.hpp:93-148, lib/algo.cc:133-492) behind the
// accelerator surface of CuBPR (/root/reference/include/buffalo/cuda/bpr/bpr.hpp:29-45).
// SgdHandle is the model and the staging of chunks; the two-pass gradient gather (TwoPassGather, below) and the exchange
// between ranks (RankExchange, sgd_exchange.hpp) are parts it holds and reaches through their methods only.
#pragma once
#include "common.hpp"
#include "sgd_exchange.hpp"

namespace bfh {

struct SgdParams {  // kernel-visible constants
    float* P;
    float* Q;
    float* Qb;
    float* gradP;
    float* gradQ;
    float* gradQb;
    int* cntP;
    int* cntQ;
    const int64_t* indptr;    // [P_rows] end offsets (full matrix)
    const int32_t* keys;      // chunk keys (chunk-local index)
    const int32_t* rows;      // chunk row ids (chunk-local index)
    const int64_t* cum_table; // [Q_rows] or null
    int64_t chunk_nnz;        // nnz in this chunk
    int64_t shift;            // global position of the chunk's first nnz (within this shard)
    int64_t nnz_offset;       // global position of the shard's first nnz
    int P_rows, Q_rows, d, vdim;
    uint32_t seed, epoch;
};

// ------------------------------------------------------------------------------------------------
// Gradient accumulation without per-triple atomics (adam / adagrad BPRMF: bpr.cc:138-156; WARP:
// warp.cc:151-165).  P and Q are frozen inside an epoch, so the three gradient rows of a triple are
// plain sums and any grouping of the terms is the reference's result up to fp32 summation order:
//   pass 1 (user-major, the update kernels): score, coefficient c_t (sigmoid-table logit / WARP's Phi) and
//          the negative of every triple -> two 4-byte arrays; gradP[u] is summed in registers over the
//          user's run (owner computes);
//   pass 2 (`grad_gather_kernel`): the triples seen from the item side.  The incidences (item, triple)
//          are sorted by item -- positives once per resident matrix (that is the CSC order), negatives
//          with one radix sort per call -- and a wave sums  sign * c_t * P[u_t]  over a run of one item's
//          incidences in registers: gradQ receives ONE atomic row add per run instead of one per triple.
// The item-side row term of WARP ( -reg * q, and -/+ Phi * q for the L2 score, warp.cc:42-52) factors
// out of the sum:  (a * sum c + b * n) * q_item, added at the flush.
// ------------------------------------------------------------------------------------------------
struct GatherParams {
    const uint32_t* inc_key;   // [n] item of every incidence, ascending; entries >= Q_rows (rejected positives) are ignored
    const int32_t* inc_idx;    // [n] pos_list: chunk-local nnz position; else chunk-local triple index (position * num_neg + slot)
    int64_t n;
    // uc[t] = (user as int bits, coefficient) of triple t, written by pass 1 -- ONE 8-byte gather per incidence carries everything
    // the gather needs (rounds 1-2 read a row id, a coefficient and WARP's accept flag: three 4-byte gathers, a sector each, a
    // quarter of the gathers' counter traffic at configs[4] size).  A negative coefficient = the positive was rejected (WARP).
    const float2* uc;          // [chunk nnz * num_neg]
    const float* P;
    const float* Q;            // read only when a != 0 or b != 0
    float* gradQ;
    float* gradQb;             // or null
    int* cntQ;                 // or null (per_coordinate_normalize)
    int num_neg, vdim, Q_rows;
    int pos_list;              // 1: one incidence per nnz position, coefficient = sum over its slots
    float sign, a, b;          // gradQ[item] += sign * sum(c p_u) + (a * sum(c) + b * n) * q_item
};

// The buffers and the host steps of the two passes (defined in sgd_base.hip); every step is ordered on the stream `s`.
class TwoPassGather {
 public:
    void prepare(int64_t triples, hipStream_t s);   // pass 1's outputs for a chunk of `triples` triples
    float2* uc() const { return uc_.get(); }        // [triples] (user, coefficient) of pass 1
    uint32_t* neg() const { return neg_.get(); }    // [triples] pass-1 negative (Q_rows: none)
    // the item-sorted positive incidence list of the staged chunk [start_x, next_x); kept while `generation` (>= 0) stays the chunk's
    void build_positive_list(const SgdParams& p, int start_x, int next_x, int64_t generation, hipStream_t s);
    // pass 2 over both lists; sab = (sign, a, b) of GatherParams; a list that is not gathered still counts into `cntQ` (when given)
    void gather(const SgdParams& p, int num_neg, bool do_pos, bool do_neg, const float sab_pos[3], const float sab_neg[3], float* gradQb, int* cntQ,
                int64_t max_waves, hipStream_t s);

 private:
    DevBuf<float2> uc_;
    DevBuf<uint32_t> neg_, nkey_;       // negatives: the sort's input / output keys
    DevBuf<int32_t> iota_, nidx_;       // 0..n-1, sorted triple indices
    DevBuf<uint32_t> pkey_;             // positives sorted by item
    DevBuf<int32_t> pidx_;
    DevBuf<char> tmp_;
    int64_t iota_n_ = 0, pos_gen_ = -1, pos_n_ = -1;   // what the positive list was built from
    int pos_start_ = -1, pos_next_ = -1;
};

class SgdHandle : public HandleBase {
 public:   // the entry points of sgd_abi.hpp
    explicit SgdHandle(int kind) : kind_(kind) {}
    ~SgdHandle() override;
    // ---- reference surface -------------------------------------------------------------------
    bool init(const char* opt_path);
    int get_vdim() const { return vdim_; }
    void initialize_model(float* P, int P_rows, float* Q, float* Qb, int Q_rows, int64_t num_nnz, bool set_gpu);
    void set_placeholder(const int64_t* indptr, size_t batch_size);
    void set_cumulative_table(const int64_t* table);
    void synchronize(bool device_to_host, bool force = false);
    void update_parameters();   // exchange gradients, step, re-base Z, counters
    // ---- extensions --------------------------------------------------------------------------
    void set_resident_csr(const int64_t* indptr, const int32_t* keys, int64_t nnz);
    virtual void set_mode(const std::string& name, int64_t v);   // the shared knobs; a backend overrides it for its own and falls through
    virtual void device_buffer(const std::string& name, void** p, size_t* bytes);
    void sync_stream() { BFH_HIP(hipStreamSynchronize(stream)); }
    // ---- multi-GPU (sgd_exchange.hpp) ------------------------------------------------------------
    void set_comm(Comm* c);
    void set_shard(int64_t nnz_offset, int num_shards) {
        BFH_REQUIRE(num_shards >= 1 && nnz_offset >= 0, "set_shard: bad arguments");
        nnz_offset_ = nnz_offset;
        num_shards_ = num_shards;
    }
    void exchange_finish(bool progressed = false);   // progressed: this rank changed Q since exchange_begin

 protected:
    // ---- staging ---------------------------------------------------------------------------------
    // stage the chunk [start_x,next_x) (keys + row ids) and fill `pr`; returns chunk nnz
    int64_t stage_chunk(int start_x, int next_x, const int64_t* indptr, const int32_t* keys, SgdParams* pr);
    bool chunk_kept() const { return resident_ || (auto_resident_ && !chunks_.empty()); }   // the staged chunk lives on in HBM under csr_generation_
    double current_lr() const;  // deterministic per-call schedule (see DESIGN.md "learning rate")
    void advance_progress(int start_x, int next_x, const int64_t* indptr_host);
    // injected triples (update_triples, compute_loss): uploaded on the stream as [users | pos | neg]; returns the device array
    const int32_t* upload_triples(int64_t n, const int32_t* users, const int32_t* pos, const int32_t* neg);
    void finish_for_reader();   // an exchange in flight is finished before the caller reads (or all-reduces) the replicated tensors itself
    void harvest_timers();
    virtual void parse_specific() = 0;
    virtual bool project_unit_ball() const { return false; }
    // ---- two-pass accumulation: gather_ on this handle's stream, chunk identity and knobs ------------
    void acc_prepare(int64_t triples) { gather_.prepare(triples, stream); }
    void acc_build_positive_list(const SgdParams& p, int start_x, int next_x) {
        gather_.build_positive_list(p, start_x, next_x, chunk_kept() ? csr_generation_ : -1, stream);
    }
    void acc_gather(const SgdParams& p, int num_neg, bool do_pos, bool do_neg, const float sab_pos[3], const float sab_neg[3], bool with_bias);
    // ---- the exchange: exchange_ on the pair this optimizer replicates (model_pair / gradient_pair below) ----
    bool has_comm() const { return exchange_.active(); }
    void exchange_arm() {   // first exchange point of a model: capture the state every rank starts from
        if (model_on_gpu_) exchange_.arm(hogwild() ? model_pair() : gradient_pair(), hogwild());
    }
    void exchange_histogram(const int32_t* keys, int64_t n) { exchange_.histogram(model_pair(), keys, n); }
    void exchange_weights(double interval_triples, double lr, int num_neg, bool uniform) { exchange_.weights(interval_triples, lr, num_neg, uniform); }
    void exchange_begin();

    Options opt_;
    bool model_on_gpu_ = false;
    int d_ = 0, vdim_ = 0, P_rows_ = 0, Q_rows_ = 0;
    std::string optimizer_;
    bool use_bias_ = false, update_i_ = true, update_j_ = true, pcn_ = false, compute_loss_ = false;
    float reg_u_ = 0, reg_i_ = 0, reg_j_ = 0, reg_b_ = 0;
    double reg_b_d_ = 0;   // reg_b as the reference holds it (a double, bpr.cc:81)
    // knobs
    int sequential_ = 0, hogwild_atomic_ = 1, prefetch_ = -1, waves_per_cu_ = 0, chunk_ = 256;  // prefetch -1: the kernel's default
    bool chunk_set_ = false;
    int accum_two_pass_ = 1;       // adam / adagrad / WARP: item-side gradients by the sorted gather (0: one atomic row add per triple)
    int comm_overlap_ = 1;         // leave the last exchange of a call in flight (finished by the next exchange point / reader)
    int comm_segments_ = 0;        // exchange segments per partial_update call (0 = 1: one blocking exchange; k > 1: pipelined)
    int64_t csr_generation_ = 0;   // bumped by set_resident_csr and by every chunk upload
    DevBuf<float> P_, Q_, Qb_, gradP_, gradQ_, gradQb_;
    DevBuf<int> cntP_, cntQ_;
    DevBuf<int32_t> keys_;
    DevBuf<double> scratch_;  // loss / counters returned by kernels
    bool resident_ = false;
    int64_t resident_nnz_ = 0;
    bool have_cum_ = false;
    int64_t cum_total_ = 0;
    int num_cus_ = 256;
    TwoPassGather gather_;
    EventTimer t_main_, t_aux_;   // dominant kernel, everything but it and the optimizer

 private:
    // what the ranks exchange: Hogwild sgd the model's Q | Qb, adam / adagrad / WARP the gradients gradQ | gradQb
    bool hogwild() const { return optimizer_ == "sgd"; }
    ReplicatedPair model_pair() const { return {Q_.get(), Qb_.get(), Q_rows_, vdim_, stream}; }
    ReplicatedPair gradient_pair() const { return {gradQ_.get(), gradQb_.get(), Q_rows_, vdim_, stream}; }
    void optimizer_step();   // adam / adagrad over P, Qb, Q from the epoch's gradients (+ WARP's projection)
    void unpin_host();

    int kind_;  // 0 bpr, 1 warp
    bool inited_ = false, placeholder_set_ = false;
    int64_t num_nnz_ = 0;
    int num_iters_ = 0;
    double lr_ = 0, min_lr_ = 0, beta1_ = 0;
    uint32_t seed_ = 0, epoch_ = 0;
    int iters_ = 0;
    double processed_ = 0;  // sum of job sizes so far (Q-8)
    int64_t nnz_offset_ = 0;
    int num_shards_ = 1;
    // the reference's call pattern hands the chunk's keys over on EVERY call (cuda/_bpr.pyx:60-74) and copies the model back
    // after every epoch.  auto_resident: a chunk seen before -- same row range, same length, same 64-bit hash over the whole host
    // buffer -- is served from its copy in HBM (and keeps its item-major regrouping); lazy_sync: synchronize(device_to_host)
    // only marks the host arrays stale, the copy happens on synchronize(2) / destroy (default off = the reference behaviour);
    // pin_host: the caller's factor arrays are page-locked for the duration of the model (D2H at PCIe rate)
    int auto_resident_ = 1, lazy_sync_ = 0, pin_host_ = 0;   // pin_host: opt-in since round 5 (the default copies back through HostStager)
    HostStager stager_;
    bool host_stale_ = false;
    struct ChunkSig { int64_t n; uint64_t sig; };
    std::map<std::pair<int, int>, ChunkSig> chunks_;
    std::vector<std::pair<void*, size_t>> pinned_;
    int gather_waves_per_cu_ = 0;  // grad_gather_kernel grid (0: 32 waves per CU)
    float *hostP_ = nullptr, *hostQ_ = nullptr, *hostQb_ = nullptr;
    DevBuf<float> momP_, momQ_, momQb_, velP_, velQ_, velQb_;
    DevBuf<int64_t> indptr_, cum_;
    std::vector<int64_t> indptr_host_;
    DevBuf<int32_t> rows_;
    DevBuf<int32_t> inj_;     // upload_triples
    RankExchange exchange_;
    EventTimer t_opt_;        // optimizer
};

}  // namespace bfh
