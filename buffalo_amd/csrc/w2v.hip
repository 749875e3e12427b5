// Word2Vec (skip-gram with negative sampling) on gfx950 -- handle and C ABI (bfh_w2v_*); the kernels are in w2v_kernels.hpp.
//
// Reference semantics: w2v::CW2V (/root/reference/lib/algo_impl/w2v/w2v.cc) behind CyW2V's surface (/root/reference/buffalo/algo/_w2v.pyx).
// The reference queues jobs for worker threads that draw from one mt19937 each and reads a learning rate that a third thread moves;
// here a call to add_jobs is synchronous and everything random or timed is a stated function of the stream:
//   * jobs are cut by the rule of add_jobs (w2v.cc:143-194) and a job's alpha is the schedule of progress_manager (:322-361) evaluated
//     at the words of all earlier jobs -- what the reference converges to when every job is finished before the next one is queued;
//   * every draw is counter_draw(seed, stream, pos, slot, epoch, attempt) at the word's GLOBAL position in the stream
//     (buffalo_hip.h lists the layout), so a split into batches changes no draw.
// add_jobs runs three named steps:
//   a  subsample   w2v_subsample_kernel: one wave per sentence drops OOV and subsampled words, compacts the sentence in order and
//                  draws the reduced window of every kept word;
//   b  plan        w2v_pair_count_kernel (pairs per sentence), then on the host: work items = runs of at most "chunk" consecutive
//                  centres of ONE sentence, with the alpha of the sentence's job;
//   c  update      w2v_update_kernel: a lane group walks the pairs of its item in stream order (update_parameter, w2v.cc:274-320),
//                  the groups of the grid run Hogwild against each other as the reference's workers do.
// Loss: one double per item, written by the item's group, summed over the items in a fixed order; no float atomics.
#include <chrono>

#include "abi.hpp"
#include "w2v_kernels.hpp"

namespace bfh {

// CW2V::build_exp_table w2v.cc:124-130: sigmoid at the 1000 cell starts of [-6, 6)
static void w2v_build_table(float* out) {
    for (int i = 0; i < kW2vTable; ++i) {
        const float x = (static_cast<float>(i) / static_cast<float>(kW2vTable) * 2.f - 1.f) * 6.f;
        const float e = static_cast<float>(std::exp(static_cast<double>(x)));
        out[i] = e / (e + 1.f);
    }
}

class W2vHandle : public HandleBase {
 public:
    ~W2vHandle() override {
        if (stream) (void)hipStreamDestroy(stream);
    }

    bool init(const char* opt_path) {
        std::string err;
        if (!opt_.load(opt_path ? opt_path : "", &err)) {
            last_error = err;
            return false;
        }
        d_ = opt_.integer("d");
        window_ = opt_.integer("window");
        num_neg_ = opt_.integer("num_negative_samples");
        num_iters_ = opt_.integer("num_iters");
        lr_ = opt_.num("lr");
        min_lr_ = opt_.num("min_lr");
        seed_ = static_cast<uint32_t>(static_cast<int64_t>(opt_.num_or("random_seed", 0)));
        batch_size_ = static_cast<int64_t>(opt_.num_or("batch_size", 0));   // json11 gives 0 for a missing key: one sentence per job
        if (batch_size_ < 0) batch_size_ = 10000;                            // w2v.cc:155-156
        compute_loss_ = opt_.boolean_or("compute_loss_on_training", false);
        BFH_REQUIRE(d_ >= 1, "option d must be at least 1");
        if (d_ > 256) throw Error(BFH_ERR_UNSUPPORTED, "W2V: d > 256 is not supported by the gfx950 update kernel (a lane group holds at most 256 columns)");
        BFH_REQUIRE(window_ >= 1, "option window must be at least 1");
        BFH_REQUIRE(window_ <= 127, "W2V: window > 127 is not supported (the sampler's slot j - i + window has 8 bits)");
        BFH_REQUIRE(num_neg_ >= 0 && num_neg_ < 65536, "option num_negative_samples must be in [0, 65536)");
        BFH_REQUIRE(num_iters_ >= 1, "option num_iters must be at least 1");
        vdim_ = vdim_of(d_);
        BFH_HIP(hipSetDevice(device));
        if (!stream) BFH_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        float table[kW2vTable];
        w2v_build_table(table);
        table_.resize(kW2vTable);
        sums_.resize(1);
        rsum_.resize(1);
        bad_.resize(1);
        BFH_HIP(hipMemcpyAsync(table_.get(), table, sizeof(table), hipMemcpyHostToDevice, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        inited_ = true;
        model_ = launched_ = false;
        return true;
    }

    // CW2V::initialize_model w2v.cc:104-122
    void initialize_model(float* L0, int L0_rows, const int32_t* index, int index_size, const uint32_t* scale, const int32_t* dist, int64_t total_word_count) {
        BFH_REQUIRE(inited_, "initialize_model called before init");
        BFH_REQUIRE(L0 && L0_rows > 0, "initialize_model: null L0 or no rows");
        BFH_REQUIRE(index && index_size > 0 && scale && dist, "initialize_model: null index / scale / dist");
        BFH_REQUIRE(total_word_count > 0, "initialize_model: total_word_count must be positive");
        BFH_REQUIRE(num_neg_ == 0 || L0_rows >= 2, "initialize_model: negative sampling needs a vocabulary of at least 2 words (a negative differs from the target)");
        for (int i = 0; i < index_size; ++i) BFH_REQUIRE(index[i] >= 0 && index[i] <= L0_rows, "initialize_model: index holds a word id outside [0, rows of L0]");
        BFH_REQUIRE(dist[0] >= 0, "initialize_model: dist is negative");
        for (int i = 1; i < L0_rows; ++i) BFH_REQUIRE(dist[i] >= dist[i - 1], "initialize_model: dist is not non-decreasing (it is the cumulative sampling table)");
        BFH_REQUIRE(num_neg_ == 0 || dist[L0_rows - 1] > 0, "initialize_model: dist[V - 1] must be positive");
        L0_host_ = L0; V_ = L0_rows; index_size_ = index_size; total_word_count_ = total_word_count;
        L0d_.resize(static_cast<size_t>(V_) * vdim_, true, stream);
        L1d_.resize(static_cast<size_t>(V_) * vdim_, true, stream);
        index_.resize(index_size); scale_.resize(V_); dist_.resize(V_);
        BFH_HIP(hipMemcpyAsync(index_.get(), index, sizeof(int32_t) * index_size, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(scale_.get(), scale, sizeof(uint32_t) * V_, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(dist_.get(), dist, sizeof(int32_t) * V_, hipMemcpyHostToDevice, stream));
        stats.h2d_bytes += 4.0 * index_size + 8.0 * V_;
        model_ = true;
        launched_ = false;
        last_n_ = last_sents_ = 0;
        upload_model();
    }

    void upload_model() {
        BFH_REQUIRE(model_, "synchronize before initialize_model");
        stats.h2d_bytes += rows_to_device(L0d_.get(), vdim_, L0_host_, d_, 0, V_, stream);
        BFH_HIP(hipStreamSynchronize(stream));
    }
    void download_model() {
        BFH_REQUIRE(model_, "synchronize before initialize_model");
        stats.d2h_bytes += rows_to_host(L0_host_, d_, L0d_.get(), vdim_, 0, V_, stream);
        BFH_HIP(hipStreamSynchronize(stream));
    }

    // CW2V::launch_workers w2v.cc:132-140: the schedule of progress_manager starts over
    void launch_workers() {
        BFH_REQUIRE(model_, "launch_workers before initialize_model");
        processed_ = 0;
        loss_sum_ = 0.0;
        launched_ = true;
    }

    // CW2V::add_jobs w2v.cc:143-194 + the workers' share of it (:197-271), finished before it returns
    void add_jobs(int start_x, int next_x, const int64_t* indptr, const int32_t* sequences) {
        BFH_REQUIRE(model_, "add_jobs before initialize_model");
        BFH_REQUIRE(launched_, "add_jobs before launch_workers (or after join)");
        BFH_REQUIRE(indptr, "add_jobs: null indptr");
        BFH_REQUIRE(0 <= start_x && start_x <= next_x, "add_jobs: bad sentence range");
        if (next_x == start_x) return;   // :149-152
        const int sents = next_x - start_x;
        const int64_t shifted = start_x == 0 ? 0 : indptr[start_x - 1], n = indptr[next_x - 1] - shifted;
        BFH_REQUIRE(shifted >= 0 && n >= 0, "add_jobs: indptr is not a non-decreasing list of END offsets");
        BFH_REQUIRE(n == 0 || sequences, "add_jobs: null sequences");
        const uint32_t epoch = epoch_override_ >= 0 ? static_cast<uint32_t>(epoch_override_) : static_cast<uint32_t>(processed_ / total_word_count_);
        if (n == 0) {   // only empty sentences: no job is queued (:170-173)
            last_n_ = last_sents_ = 0;
            return;
        }
        subsample(start_x, sents, shifted, n, indptr, sequences, epoch);
        plan(start_x, sents, shifted, indptr);
        update(epoch);
    }

    // CW2V::join w2v.cc:364-382; the reference returns 0.0, here: the loss summed since launch_workers
    double join() {
        BFH_REQUIRE(model_, "join before initialize_model");
        BFH_REQUIRE(launched_, "join before launch_workers");
        download_model();
        launched_ = false;
        return compute_loss_ ? loss_sum_ : 0.0;
    }

    // test hook: explicit pairs in order through the update code of step c
    void update_pairs(int64_t n, const int32_t* inputs, const int32_t* outputs, int n_out, double alpha) {
        BFH_REQUIRE(model_, "update_pairs before initialize_model");
        BFH_REQUIRE(n >= 0 && n_out >= 1, "update_pairs: n < 0 or no output row");
        if (n == 0) return;
        BFH_REQUIRE(inputs && outputs, "update_pairs: null array");
        for (int64_t i = 0; i < n; ++i) BFH_REQUIRE(inputs[i] >= 0 && inputs[i] < V_, "update_pairs: input word outside the vocabulary");
        for (int64_t i = 0; i < n * n_out; ++i) BFH_REQUIRE(outputs[i] >= 0 && outputs[i] < V_, "update_pairs: output word outside the vocabulary");
        grow(pair_in_, static_cast<size_t>(n));
        grow(pair_out_, static_cast<size_t>(n * n_out));
        BFH_HIP(hipMemcpyAsync(pair_in_.get(), inputs, sizeof(int32_t) * n, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(pair_out_.get(), outputs, sizeof(int32_t) * n * n_out, hipMemcpyHostToDevice, stream));
        W2vPairsArgs a{model_args(0), n, pair_in_.get(), pair_out_.get(), n_out, alpha, sums_.get()};
#define BFH_W2V_PAIRS(GG)                                                                                          \
    do {                                                                                                           \
        if (atomic_) hipLaunchKernelGGL((w2v_pairs_kernel<GG, true>), dim3(1), dim3(64), 0, stream, a);            \
        else hipLaunchKernelGGL((w2v_pairs_kernel<GG, false>), dim3(1), dim3(64), 0, stream, a);                   \
    } while (0)
        dispatch_g([&] { BFH_W2V_PAIRS(16); }, [&] { BFH_W2V_PAIRS(32); }, [&] { BFH_W2V_PAIRS(64); });
#undef BFH_W2V_PAIRS
        BFH_HIP(hipGetLastError());
        double loss = 0.0;
        BFH_HIP(hipMemcpyAsync(&loss, sums_.get(), sizeof(double), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        loss_sum_ += loss;
    }

    void set_mode(const std::string& name, int64_t value) {
        if (name == "sequential") sequential_ = value != 0;
        else if (name == "hogwild_atomic") {
            BFH_REQUIRE(value == 0 || value == 1, "hogwild_atomic: 1 (fp32 atomic adds) or 0 (plain read-modify-write stores)");
            atomic_ = value != 0;
        } else if (name == "chunk") {
            BFH_REQUIRE(value >= 0, "chunk: centres per work item, 0 = a whole sentence");
            chunk_ = value;
        } else if (name == "epoch") {
            BFH_REQUIRE(value >= -1 && value < (int64_t(1) << 24), "epoch: -1 (from the words processed) or a value below 2^24");
            epoch_override_ = value;
        } else if (name == "timing") timing = value != 0;
        else throw Error(BFH_ERR_INVALID, "unknown mode '" + name + "' (sequential, hogwild_atomic, chunk, epoch, timing)");
    }

    void device_buffer(const std::string& name, void** ptr, size_t* bytes) {
        if (name == "L0") { *ptr = L0d_.get(); *bytes = L0d_.bytes(); }
        else if (name == "L1") { *ptr = L1d_.get(); *bytes = L1d_.bytes(); }
        else if (name == "kept") { *ptr = kept_.get(); *bytes = static_cast<size_t>(last_n_) * sizeof(int32_t); }
        else if (name == "kept_pos") { *ptr = kept_pos_.get(); *bytes = static_cast<size_t>(last_n_) * sizeof(int64_t); }
        else if (name == "window_b") { *ptr = window_b_.get(); *bytes = static_cast<size_t>(last_n_) * sizeof(int32_t); }
        else if (name == "sent_end") { *ptr = sent_end_.get(); *bytes = static_cast<size_t>(last_sents_) * sizeof(int64_t); }
        else throw Error(BFH_ERR_INVALID, "unknown device buffer '" + name + "' (L0, L1; of the last add_jobs: kept, kept_pos, sent_end, window_b)");
    }

    void refresh_stats() override {
        stats.kernel_ms = kernel_ms_;
        stats.aux_ms = aux_ms_;
    }
    void clear_accumulators() override { kernel_ms_ = aux_ms_ = 0.0; }
    int vdim() const { return vdim_; }

 private:
    template <typename F0, typename F1, typename F2>
    void dispatch_g(F0 f16, F1 f32, F2 f64) {
        if (vdim_ <= 64) f16();
        else if (vdim_ <= 128) f32();
        else f64();
    }

    W2vModel model_args(uint32_t epoch) const {
        return W2vModel{L0d_.get(), L1d_.get(), dist_.get(), table_.get(), V_, vdim_, window_, num_neg_, compute_loss_ ? 1 : 0, seed_, epoch};
    }

    // the job rule of add_jobs (w2v.cc:158-193) over the call's sentences: alpha_[s] = the alpha of the job that holds sentence s.
    // A job's alpha is the schedule (:344-347) at the words of all earlier jobs; job.size counts words BEFORE subsampling.
    void cut_jobs(int start_x, int sents, int64_t shifted, const int64_t* indptr) {
        alpha_.assign(sents, 0.0);
        std::vector<int> job;
        int64_t job_size = 0, job_words = 0;
        auto push = [&] {   // job_queue_.push(job): also reached with an empty job, which changes nothing
            const double progress = static_cast<double>(processed_) / (static_cast<double>(total_word_count_) * num_iters_);
            const double alpha = std::max(lr_ - (lr_ - min_lr_) * progress, min_lr_);
            for (int s : job) alpha_[s] = alpha;
            processed_ += job_words;
            job.clear();
            job_words = 0;
        };
        for (int s = 0; s < sents; ++s) {
            const int64_t beg = s == 0 ? shifted : indptr[start_x + s - 1], len = indptr[start_x + s] - beg;
            BFH_REQUIRE(len >= 0, "add_jobs: indptr is not a non-decreasing list of END offsets");
            if (len == 0) continue;
            if (len + job_size <= batch_size_) {
                job_size += len;
            } else {
                push();
                job_size = len;
            }
            job.push_back(s);
            job_words += len;
        }
        if (job_words) push();
    }

    // step a
    void subsample(int start_x, int sents, int64_t shifted, int64_t n, const int64_t* indptr, const int32_t* sequences, uint32_t epoch) {
        grow(seq_, static_cast<size_t>(n)); grow(kept_, static_cast<size_t>(n)); grow(kept_pos_, static_cast<size_t>(n)); grow(window_b_, static_cast<size_t>(n));
        grow(ends_, static_cast<size_t>(sents)); grow(sent_end_, static_cast<size_t>(sents)); grow(pairs_, static_cast<size_t>(sents));
        BFH_HIP(hipMemcpyAsync(seq_.get(), sequences, sizeof(int32_t) * n, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemcpyAsync(ends_.get(), indptr + start_x, sizeof(int64_t) * sents, hipMemcpyHostToDevice, stream));
        BFH_HIP(hipMemsetAsync(bad_.get(), 0, sizeof(int), stream));
        stats.h2d_bytes += 4.0 * n + 8.0 * sents;
        W2vSubArgs a{seq_.get(), ends_.get(), shifted, sents, index_.get(), index_size_, scale_.get(), window_, seed_, epoch,
                     kept_.get(), kept_pos_.get(), window_b_.get(), sent_end_.get(), bad_.get()};
        const unsigned blocks = static_cast<unsigned>(std::min<int64_t>((static_cast<int64_t>(sents) + 3) / 4, 8192));
        maybe_timed(t_aux_, [&] {
            hipLaunchKernelGGL(w2v_subsample_kernel, dim3(blocks), dim3(256), 0, stream, a);
            hipLaunchKernelGGL(w2v_pair_count_kernel, dim3(blocks), dim3(256), 0, stream, ends_.get(), shifted, sents, sent_end_.get(), window_b_.get(), window_, pairs_.get());
        });
        BFH_HIP(hipGetLastError());
        last_n_ = n;
        last_sents_ = sents;
    }

    // step b: the counts come back, the items go out
    void plan(int start_x, int sents, int64_t shifted, const int64_t* indptr) {
        const int64_t* ends = indptr + start_x;
        h_sent_end_.resize(sents); h_pairs_.resize(sents);
        int bad = 0;
        BFH_HIP(hipMemcpyAsync(h_sent_end_.data(), sent_end_.get(), sizeof(int64_t) * sents, hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipMemcpyAsync(h_pairs_.data(), pairs_.get(), sizeof(int64_t) * sents, hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipMemcpyAsync(&bad, bad_.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        aux_ms_ += t_aux_.drain();
        stats.d2h_bytes += 16.0 * sents;
        BFH_REQUIRE(!bad, "add_jobs: a word of the stream is outside [0, index_size)");
        cut_jobs(start_x, sents, shifted, indptr);
        const auto t0 = std::chrono::steady_clock::now();
        items_.clear();
        int64_t kept = 0, pairs = 0;
        for (int s = 0; s < sents; ++s) {
            const int64_t kb = (s == 0 ? shifted : ends[s - 1]) - shifted, ke = h_sent_end_[s];
            if (ke == kb) continue;
            kept += ke - kb;
            pairs += h_pairs_[s];
            const int64_t step = chunk_ == 0 ? ke - kb : chunk_;
            for (int64_t c0 = kb; c0 < ke; c0 += step) items_.push_back(W2vItem{kb, ke, c0, std::min(ke, c0 + step), alpha_[s]});
        }
        call_pairs_ = pairs;
        stats.accepted += kept;
        if (!items_.empty()) {
            grow(items_dev_, items_.size()); grow(item_loss_, items_.size()); grow(item_redraws_, items_.size());
            BFH_HIP(hipMemcpyAsync(items_dev_.get(), items_.data(), items_.size() * sizeof(W2vItem), hipMemcpyHostToDevice, stream));
            BFH_HIP(hipStreamSynchronize(stream));   // items_ is reused by the next call
            stats.h2d_bytes += static_cast<double>(items_.size() * sizeof(W2vItem));
        }
        if (timing) aux_ms_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }

    // step c
    void update(uint32_t epoch) {
        const int64_t n_items = static_cast<int64_t>(items_.size());
        if (n_items == 0) return;
        W2vUpdateArgs a{model_args(epoch), items_dev_.get(), n_items, kept_.get(), kept_pos_.get(), window_b_.get(), item_loss_.get(), item_redraws_.get(),
                        sequential_ ? 1 : 0};
        const int ng = vdim_ <= 64 ? 4 : vdim_ <= 128 ? 2 : 1;
        const int64_t waves = (n_items + ng - 1) / ng;
        const dim3 grid(sequential_ ? 1u : static_cast<unsigned>(std::min<int64_t>((waves + 3) / 4, 2048)));
        const dim3 block(sequential_ ? 64 : 256);
#define BFH_W2V_UPDATE(GG)                                                                                       \
    do {                                                                                                         \
        if (atomic_) hipLaunchKernelGGL((w2v_update_kernel<GG, true>), grid, block, 0, stream, a);               \
        else hipLaunchKernelGGL((w2v_update_kernel<GG, false>), grid, block, 0, stream, a);                      \
    } while (0)
        maybe_timed(t_kernel_, [&] { dispatch_g([&] { BFH_W2V_UPDATE(16); }, [&] { BFH_W2V_UPDATE(32); }, [&] { BFH_W2V_UPDATE(64); }); });
#undef BFH_W2V_UPDATE
        BFH_HIP(hipGetLastError());
        hipLaunchKernelGGL(w2v_item_sum_kernel, dim3(1), dim3(256), 0, stream, item_loss_.get(), item_redraws_.get(), n_items, sums_.get(), rsum_.get());
        BFH_HIP(hipGetLastError());
        double loss = 0.0;
        int64_t redraws = 0;
        BFH_HIP(hipMemcpyAsync(&loss, sums_.get(), sizeof(double), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipMemcpyAsync(&redraws, rsum_.get(), sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        BFH_HIP(hipStreamSynchronize(stream));
        kernel_ms_ += t_kernel_.drain();
        loss_sum_ += loss;
        stats.launches += 1;
        stats.samples += call_pairs_;
        stats.scored_negatives += call_pairs_ * num_neg_;
        stats.loaded_rows += redraws;
    }

    template <typename F>
    void maybe_timed(EventTimer& t, F&& fn) {
        if (timing) t.timed(stream, fn);
        else fn();
    }

    Options opt_;
    int d_ = 0, vdim_ = 0, window_ = 0, num_neg_ = 0, num_iters_ = 1, V_ = 0, index_size_ = 0;
    double lr_ = 0, min_lr_ = 0;
    uint32_t seed_ = 0;
    int64_t batch_size_ = 0, total_word_count_ = 1, processed_ = 0, chunk_ = 64, epoch_override_ = -1, call_pairs_ = 0;
    bool compute_loss_ = false, inited_ = false, model_ = false, launched_ = false, sequential_ = false, atomic_ = true;
    double loss_sum_ = 0.0;
    float* L0_host_ = nullptr;
    DevBuf<float> L0d_, L1d_, table_;
    DevBuf<int32_t> index_, dist_, seq_, kept_, window_b_, pair_in_, pair_out_;
    DevBuf<uint32_t> scale_;
    DevBuf<int64_t> ends_, sent_end_, pairs_, kept_pos_, item_redraws_, rsum_;
    DevBuf<double> item_loss_, sums_;
    DevBuf<W2vItem> items_dev_;
    DevBuf<int> bad_;
    std::vector<double> alpha_;
    std::vector<int64_t> h_sent_end_, h_pairs_;
    std::vector<W2vItem> items_;
    int64_t last_n_ = 0, last_sents_ = 0;
    EventTimer t_aux_, t_kernel_;
    double kernel_ms_ = 0, aux_ms_ = 0;
};

}  // namespace bfh

using bfh::guarded;
using bfh::W2vHandle;

extern "C" {

BFH_ABI_LIFECYCLE(w2v, W2vHandle)

int bfh_w2v_init(void* h, const char* opt_json_path) {
    return guarded<W2vHandle>(h, [&](W2vHandle& w) { return w.init(opt_json_path); });
}
int bfh_w2v_get_vdim(void* h) {
    return guarded<W2vHandle>(h, [](W2vHandle& w) { return w.vdim(); });
}
int bfh_w2v_initialize_model(void* h, float* L0, int L0_rows, const int32_t* index, int index_size, const uint32_t* scale, const int32_t* dist,
                             int64_t total_word_count) {
    return guarded<W2vHandle>(h, [&](W2vHandle& w) { w.initialize_model(L0, L0_rows, index, index_size, scale, dist, total_word_count); });
}
int bfh_w2v_launch_workers(void* h) {
    return guarded<W2vHandle>(h, [](W2vHandle& w) { w.launch_workers(); });
}
int bfh_w2v_add_jobs(void* h, int start_x, int next_x, const int64_t* indptr, const int32_t* sequences) {
    return guarded<W2vHandle>(h, [&](W2vHandle& w) { w.add_jobs(start_x, next_x, indptr, sequences); });
}
int bfh_w2v_join(void* h, double* loss) {
    return guarded<W2vHandle>(h, [&](W2vHandle& w) {
        const double v = w.join();
        if (loss) *loss = v;
    });
}
int bfh_w2v_synchronize(void* h, int device_to_host) {
    return guarded<W2vHandle>(h, [&](W2vHandle& w) {
        if (device_to_host) w.download_model();
        else w.upload_model();
    });
}
int bfh_w2v_set_mode(void* h, const char* name, int64_t value) {
    return guarded<W2vHandle>(h, [&](W2vHandle& w) { w.set_mode(name ? name : "", value); });
}
int bfh_w2v_device_buffer(void* h, const char* name, void** ptr, size_t* bytes) {
    return guarded<W2vHandle>(h, [&](W2vHandle& w) { w.device_buffer(name ? name : "", ptr, bytes); });
}
void* bfh_w2v_stream(void* h) { return bfh::stream_of(h); }
int bfh_w2v_update_pairs(void* h, int64_t n, const int32_t* inputs, const int32_t* outputs, int n_out, double alpha) {
    return guarded<W2vHandle>(h, [&](W2vHandle& w) { w.update_pairs(n, inputs, outputs, n_out, alpha); });
}
int bfh_w2v_exp_table(float* out1000) {
    if (!out1000) return BFH_ERR_INVALID;
    bfh::w2v_build_table(out1000);
    return BFH_OK;
}

}  // extern "C"
