// RankExchange: how the ranks of a multi-GPU run (one process per GPU, users sharded, item factors replicated; SURVEY.md
// section 8(e)) keep a replicated pair -- a [rows, vdim] matrix and its [rows] bias column -- in step.  Defined in sgd_base.hip.
//
// Hogwild sgd exchanges the model itself, Q | Qb: local SGD on the rank's replica; what the rank changed since the state Z all
// ranks agree on is summed over the ranks with ONE all-reduce per exchange point.  The exchange is pipelined one deep on the
// communicator's stream: `begin` publishes S = Q - Z and returns, the next walk runs on the local replica, and `finish` (at the
// next exchange point, or before anything reads Q) advances Z <- Z + R (R = summed deltas: the same arithmetic on every rank, Z
// stays bit-identical) and folds in what the OTHER ranks sent, Q += R - S -- or, when the rank has not worked since `begin` (a
// flush), Q <- Z exactly, so flushed replicas are bit-identical.  Every delta is applied exactly once everywhere.
// adam / adagrad / WARP exchange the gradient buffers, gradQ | gradQb (| counts): their deltas are summed once per
// update_parameters (`gradients`), before the (then identical) optimizer step -- exactly the single-GPU result up to summation
// order (algo.cc:382); `rebase` then makes what the buffers keep after the step the base of the next delta.
#pragma once
#include "common.hpp"

namespace bfh {

class Comm;

// the replicated pair of one call, and the stream its kernels are ordered on
struct ReplicatedPair {
    float* X;    // [rows, vdim]
    float* Xb;   // [rows]
    int rows, vdim;
    hipStream_t stream;
};

class RankExchange {
 public:
    ~RankExchange();   // waits for an exchange in flight
    bool active() const { return comm_ != nullptr; }
    bool pending() const { return pending_; }
    void set_comm(Comm* c, int device);   // nothing may be pending
    void set_stiffness(int bias_milli) { stiffness_milli_ = bias_milli; }
    void set_stiffness_q(int rows_milli) { stiffness_q_milli_ = rows_milli; }
    void reset();                         // a new model: an exchange in flight is waited for and dropped, `arm` captures again
    // first exchange point of a model: Z <- the pair as every rank starts from it; `weighted` (the Hogwild exchange): combination weights of 1
    void arm(const ReplicatedPair& q, bool weighted);
    void histogram(const ReplicatedPair& q, const int32_t* keys, int64_t n);
    void weights(double interval_triples, double lr, int num_neg, bool uniform);
    void begin(const ReplicatedPair& q, bfh_stats& stats);
    // progressed: this rank changed the pair since `begin`.  num_nnz, the cumulative table (null: uniform negatives) and its total feed the weights
    void finish(const ReplicatedPair& q, bool progressed, int64_t num_nnz, const int64_t* cum, int64_t cum_total);
    void gradients(const ReplicatedPair& g, int* counts, bfh_stats& stats);   // synchronous; counts: per_coordinate_normalize's, or null
    void rebase(const ReplicatedPair& g);
    void drain_timers(bfh_stats& stats);

 private:
    // matrix | bias (padded to 4) | 4 scalars that travel with the delta: [0] this rank's triples inside the interval, [1] its lr --
    // their sums come back with R, so the combination weights are computed from the SAME numbers on every rank
    static size_t scalars_at(const ReplicatedPair& q) { return static_cast<size_t>(q.rows) * q.vdim + ((static_cast<size_t>(q.rows) + 3) / 4) * 4; }
    static size_t count(const ReplicatedPair& q) { return scalars_at(q) + 4; }
    void capture(const ReplicatedPair& q);   // Z <- the pair as it is now
    void publish(const ReplicatedPair& q);   // S <- the pair - Z

    Comm* comm_ = nullptr;          // not owned
    bool armed_ = false, pending_ = false;
    DevBuf<float> Z_, S_, R_;       // [count()]: state at the last exchange, own delta, summed deltas
    DevBuf<float> W_, Wb_;          // [rows] combination weight of every factor row / bias for the exchange in flight (sum .. mean)
    DevBuf<int> gcnt_;              // [rows] positives per item over all ranks
    double gcnt_total_ = 0;
    bool gcnt_ready_ = false;
    int stiffness_milli_ = 250;     // curvature the saturation model assumes for the biases (permille); 0: plain sum
    int stiffness_q_milli_ = 25;    // ... and for the factor rows (the reference's default regulariser)
    hipEvent_t ready_ = nullptr, done_ = nullptr;
    double w_interval_ = 0, w_lr_ = 0;   // what `weights` announced for the exchange that begins next
    int w_num_neg_ = 1;
    bool w_uniform_ = true;
    int p_num_neg_ = 1;             // ... of the exchange in flight (snapshot taken by `begin`)
    bool p_uniform_ = true;
    EventTimer t_xk_, t_ar_;        // exchange kernels, all-reduces
};

}  // namespace bfh
