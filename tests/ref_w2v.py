"""Numpy restatement of Word2Vec (skip-gram, negative sampling) as include/buffalo_hip.h states it for bfh_w2v_*: the vocabulary of
buffalo/algo/w2v.py:91-157, the job rule and the learning-rate schedule of w2v.cc:143-194 / :322-361, the counter sampler (streams 2, 3, 4 of
ref_numpy.counter_draw) and update_parameter (w2v.cc:274-320) in float64 or float32.  Test infrastructure: nothing here is used by the product.

A dot product f is SAFE when the sigmoid-table cell (clamps included) is the same for f - e and f + e, with
    e = 2^-14 * sum |a_k b_k|  +  2^-21.
2^-14 is 1024 roundings of 2^-24: any summation order at d <= 256 plus about 250 earlier three-rounding updates of either row.  2^-21 covers the
two float32 roundings of (f + 6) * 83 itself (half an ulp of a number below 8, and half an ulp of an index below 1024 divided by 83).  When every dot
of a run is safe, float32 arithmetic in any order takes the same table cells as float64, and the device can be held to the float64 run with a
rounding-sized bound."""
import json

import numpy as np

import ref_numpy as rn

STREAM_SUB, STREAM_WIN, STREAM_NEG = 2, 3, 4
EPS32 = float(np.float32(1e-8))
MAX_RETRY = 0xffff


# ------------------------------------------------------------------------------------------------
# vocabulary (w2v.py:91-157)
# ------------------------------------------------------------------------------------------------
def sampling_distribution(uni, use, total_vocab):
    dist0 = np.zeros(shape=total_vocab, dtype=np.float64)
    for i in range(len(use)):
        if use[i]:
            dist0[use[i] - 1] = uni[i]
    dist0 = dist0 ** 0.75
    dist0 /= dist0.sum()
    dist = np.zeros(shape=total_vocab, dtype=np.int32)
    summed = 0.0
    for i in range(total_vocab):
        summed += dist0[i]
        dist[i] = summed * 0x7FFFFFFF
    return dist


def build_vocab(counts, min_count, sample):
    """counts[i] = occurrences of word i in the stream -> dict(index, scale, dist, size, total_word_count)."""
    uni = [int(c) for c in counts]
    use, total_vocab = [0] * len(uni), 0
    for i, c in enumerate(uni):
        if c >= min_count:
            total_vocab += 1
            use[i] = total_vocab
    scale = np.zeros(shape=total_vocab, dtype=np.uint32)
    threshold = sum(uni[i] for i in range(len(uni)) if use[i])
    if sample > 0.0:
        threshold *= sample
    for i, c in enumerate(uni):
        if not use[i]:
            continue
        p = (((c / threshold) ** 0.5) + 1) * (threshold / c)
        if not p < 1.0:
            p = 1.0
        scale[use[i] - 1] = p * 0xFFFFFFFF
    return {"index": np.array(use, dtype=np.int32), "scale": scale, "dist": sampling_distribution(uni, use, total_vocab),
            "size": total_vocab, "total_word_count": int(sum(uni))}


def vocab_of_stream(seq, num_items, min_count=1, sample=0.0):
    return build_vocab(np.bincount(np.asarray(seq, dtype=np.int64), minlength=num_items), min_count, sample)


# ------------------------------------------------------------------------------------------------
# jobs and the learning rate
# ------------------------------------------------------------------------------------------------
def effective_batch_size(opt):
    b = int(opt.get("batch_size", 0))     # json11: a missing key reads 0
    return 10000 if b < 0 else b


def cut_jobs(lengths, batch_size):
    """The jobs one add_jobs call queues: lists of sentence numbers, in order (w2v.cc:158-193).  An empty job is queued when the first
    sentence already overflows; empty sentences belong to no job."""
    jobs, job, job_size = [], [], 0
    for s, n in enumerate(lengths):
        if n == 0:
            continue
        if n + job_size <= batch_size:
            job.append(s)
            job_size += n
        else:
            jobs.append(job)
            job, job_size = [s], n
    if job:
        jobs.append(job)
    return jobs


def alpha_at(processed, total_word_count, num_iters, lr, min_lr):
    return max(lr - (lr - min_lr) * (processed / (float(total_word_count) * num_iters)), min_lr)


# ------------------------------------------------------------------------------------------------
# the sampler
# ------------------------------------------------------------------------------------------------
def _o0(seed, stream, pos, slot, epoch, attempt):
    return rn.counter_draw(seed, stream, pos, slot, epoch, attempt)[0]


def subsample(words, first_pos, vocab, seed, epoch, window):
    """One sentence: (kept vocabulary ids, their global positions, the reduced window b of each)."""
    kept, kept_pos, b = [], [], []
    for t, w in enumerate(words):
        if not vocab["index"][w]:
            continue
        wid, pos = int(vocab["index"][w]) - 1, first_pos + t
        if int(vocab["scale"][wid]) <= _o0(seed, STREAM_SUB, pos, 0, epoch, 0):
            continue
        kept.append(wid)
        kept_pos.append(pos)
        b.append((_o0(seed, STREAM_WIN, pos, 0, epoch, 0) * window) >> 32)
    return kept, kept_pos, b


def pairs(n, b, window):
    """(centre i, context j) in the order the worker visits them."""
    return [(i, j) for i in range(n) for j in range(max(0, i - window + b[i]), min(n, i + window + 1 - b[i])) if j != i]


def negative(vocab, seed, epoch, pos, slot, target, k):
    """Negative k of one pair: (word, redraws)."""
    dist = vocab["dist"]
    total, retry = int(dist[-1]), 0
    while True:
        r3 = (_o0(seed, STREAM_NEG, pos, slot, epoch, (k << 16) | retry) * total) >> 32
        neg = int(np.searchsorted(dist, r3, side="left"))
        if neg != target or retry == MAX_RETRY:
            return neg, retry
        retry += 1


def negatives(vocab, seed, epoch, pos, slot, target, num_neg):
    """The negatives of one pair and the number of redraws."""
    drawn = [negative(vocab, seed, epoch, pos, slot, target, k) for k in range(num_neg)]
    return [w for w, _ in drawn], sum(r for _, r in drawn)


def _o0_many(seed, stream, pos, slot, epoch, attempt):
    """counter_draw(...)[0] over arrays of positions, slots and attempts (the same ten Philox rounds on uint64 lanes)."""
    M = np.uint64(0xffffffff)
    pos = np.asarray(pos, dtype=np.uint64)
    c0, c1 = pos & M, (pos >> np.uint64(32)) & M
    c2 = np.asarray(attempt, dtype=np.uint64) & M
    c3 = ((np.uint64(epoch) << np.uint64(8)) | (np.asarray(slot, dtype=np.uint64) & np.uint64(0xff))) & M
    k0, k1 = np.uint64(seed & 0xffffffff), np.uint64(0x5bf03635 ^ stream)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M, p0 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return c0


def negatives_many(vocab, seed, epoch, pos, slot, target, num_neg):
    """`negatives` for many pairs at once: ([pairs, num_neg] words, redraws); the rare redraws go through the scalar loop."""
    dist = vocab["dist"]
    n = len(pos)
    if n == 0 or num_neg == 0:
        return np.zeros((n, num_neg), dtype=np.int64), 0
    k = np.arange(num_neg, dtype=np.uint64)[None, :]
    o0 = _o0_many(seed, STREAM_NEG, np.asarray(pos, dtype=np.uint64)[:, None], np.asarray(slot, dtype=np.uint64)[:, None], epoch, k << np.uint64(16))
    out = np.searchsorted(dist, ((o0 * np.uint64(int(dist[-1]))) >> np.uint64(32)).astype(np.int64), side="left").astype(np.int64)
    redraws = 0
    for p, kk in zip(*np.nonzero(out == np.asarray(target)[:, None])):
        out[p, kk], r = negative(vocab, seed, epoch, int(pos[p]), int(slot[p]), int(target[p]), int(kk))
        redraws += r
    return out, redraws


# ------------------------------------------------------------------------------------------------
# update_parameter and the trainer
# ------------------------------------------------------------------------------------------------
def _cell(f):
    if f > 6.0:
        return -1
    if f < -6.0:
        return -2
    return int((f + 6.0) * 83.0)


class Trainer:
    """CyW2V's call surface over numpy arrays.  dtype float64: the truth; float32: the reference's arithmetic, one worker.
    `fast` = no per-dot bookkeeping and one vectorised step per pair whose output rows are distinct (float64 quality runs)."""

    def __init__(self, opt, vocab, L0, table, dtype=np.float64, L1=None, fast=False):
        self.opt, self.vocab, self.T, self.fast = opt, vocab, dtype, fast
        self.table = np.asarray(table, dtype=np.float32).astype(dtype)
        self.L0 = np.array(L0, dtype=dtype)
        self.L1 = np.zeros_like(self.L0) if L1 is None else np.array(L1, dtype=dtype)
        self.window, self.num_neg, self.seed = int(opt["window"]), int(opt["num_negative_samples"]), int(opt.get("random_seed", 0))
        self.compute_loss = bool(opt.get("compute_loss_on_training", False))
        self.epoch_override = -1
        self.launch_workers()
        self.dots, self.unsafe, self.stats = 0, 0, {"samples": 0, "scored_negatives": 0, "accepted": 0, "loaded_rows": 0}
        self.last = None

    def launch_workers(self):
        self.processed, self.loss = 0, 0.0

    def add_jobs(self, start_x, next_x, indptr, seq):
        """`seq` is the WHOLE stream here (the device gets the chunk); indptr are END offsets."""
        if next_x == start_x:
            return
        o = self.opt
        total = int(self.vocab["total_word_count"])
        epoch = self.epoch_override if self.epoch_override >= 0 else self.processed // total
        begs = [0 if x == 0 else int(indptr[x - 1]) for x in range(start_x, next_x)]
        ends = [int(indptr[x]) for x in range(start_x, next_x)]
        alphas = {}
        for job in cut_jobs([e - b for b, e in zip(begs, ends)], effective_batch_size(o)):
            a = alpha_at(self.processed, total, int(o["num_iters"]), float(o["lr"]), float(o["min_lr"]))
            for s in job:
                alphas[s] = a
                self.processed += ends[s] - begs[s]
        self.last = {"kept": [], "kept_pos": [], "window_b": []}
        for s, (b0, e0) in enumerate(zip(begs, ends)):
            kept, kept_pos, b = subsample(seq[b0:e0], b0, self.vocab, self.seed, epoch, self.window)
            for k, v in zip(("kept", "kept_pos", "window_b"), (kept, kept_pos, b)):
                self.last[k].append(v)
            self.stats["accepted"] += len(kept)
            ij = pairs(len(kept), b, self.window)
            negs, redraws = negatives_many(self.vocab, self.seed, epoch, [kept_pos[i] for i, _ in ij], [j - i + self.window for i, j in ij],
                                           [kept[i] for i, _ in ij], self.num_neg)
            self.stats["samples"] += len(ij)
            self.stats["scored_negatives"] += len(ij) * self.num_neg
            self.stats["loaded_rows"] += redraws
            for (i, j), ng in zip(ij, negs):
                self.update_pair(kept[j], [kept[i]] + [int(w) for w in ng], alphas[s])

    def update_pairs(self, inputs, outputs, alpha):
        for inp, outs in zip(inputs, outputs):
            self.update_pair(int(inp), [int(r) for r in outs], alpha)

    def update_pair(self, inp, outs, alpha):
        if self.fast and len(set(outs)) == len(outs):
            return self._update_pair_fast(inp, outs, alpha)
        T = self.T
        l0 = self.L0[inp].copy()
        work = np.zeros_like(l0)
        for k, r in enumerate(outs):
            row = self.L1[r].copy()
            prod = row * l0
            f = T(np.sum(prod, dtype=T))
            if not self.fast:
                e = 2.0 ** -14 * float(np.sum(np.abs(prod.astype(np.float64)))) + 2.0 ** -21
                self.dots += 1
                self.unsafe += _cell(float(f) - e) != _cell(float(f) + e)
            label = T(1.0 if k == 0 else 0.0)
            if f > 6:
                g = label - T(1.0)
            elif f < -6:
                g = label
            else:
                g = label - self.table[int((f + T(6.0)) * T(83.0))]
            if self.compute_loss:
                if T is np.float32:
                    self.loss -= np.log(np.float64(np.float32(g + np.float32(EPS32)))) if k == 0 else np.log(1.0 - np.float64(g) + EPS32)
                else:
                    self.loss -= np.log(g + EPS32) if k == 0 else np.log(1.0 - g + EPS32)
            g = T(np.float64(g) * alpha)
            work = work + g * row
            self.L1[r] = row + g * l0
        self.L0[inp] = self.L0[inp] + work

    def _update_pair_fast(self, inp, outs, alpha):
        l0 = self.L0[inp].copy()
        rows = self.L1[outs]
        f = rows @ l0
        label = np.zeros(len(outs))
        label[0] = 1.0
        g = label - self.table[np.clip(((f + 6.0) * 83.0).astype(np.int64), 0, 999)]
        g = np.where(f > 6.0, label - 1.0, np.where(f < -6.0, label, g))
        if self.compute_loss:
            self.loss -= np.log(g[0] + EPS32) + np.sum(np.log(1.0 - g[1:] + EPS32))
        g = g * alpha
        self.L1[outs] = rows + g[:, None] * l0[None, :]
        self.L0[inp] = l0 + g @ rows

    def join(self):
        return self.loss if self.compute_loss else 0.0


def train(opt, vocab, indptr, seq, L0, table, dtype=np.float64, L1=None, epochs=1, batches=None, fast=False):
    """launch_workers, `epochs` passes of add_jobs over `batches` (a list of (start_x, next_x); default one batch), join.
    Returns the Trainer (L0, L1, loss, dots, unsafe, stats, last)."""
    t = Trainer(opt, vocab, L0, table, dtype, L1, fast)
    batches = batches or [(0, len(indptr))]
    for _ in range(epochs):
        for a, b in batches:
            t.add_jobs(a, b, indptr, seq)
    return t


# ------------------------------------------------------------------------------------------------
# streams
# ------------------------------------------------------------------------------------------------
def make_stream(sents):
    """list of word lists -> (indptr of END offsets int64, words int32)"""
    indptr = np.cumsum([len(s) for s in sents]).astype(np.int64)
    seq = np.array([w for s in sents for w in s], dtype=np.int32)
    return indptr, seq


def random_stream(seed, num_items, num_sents, max_len, min_len=1):
    rng = np.random.default_rng(seed)
    return [list(rng.integers(0, num_items, size=int(rng.integers(min_len, max_len + 1)))) for _ in range(num_sents)]


def uneven_batches(num_sents, n):
    """n uneven consecutive sentence ranges."""
    if n <= 1:
        return [(0, num_sents)]
    w = np.arange(1, n + 1, dtype=np.float64) ** 2
    edges = np.concatenate([[0], np.round(np.cumsum(w) / w.sum() * num_sents)]).astype(int)
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:]) if b > a]


def planted_stream(seed, words=64, groups=8, num_sents=200, length=12):
    """Every sentence is drawn from ONE group of words: word w belongs to group w % groups."""
    rng = np.random.default_rng(seed)
    per = words // groups
    sents = []
    for _ in range(num_sents):
        g = int(rng.integers(0, groups))
        sents.append([int(g + groups * m) for m in rng.integers(0, per, size=length)])
    return sents


def group_share(L0, groups=8, k=3):
    """Share of words whose k nearest cosine neighbours all lie in the word's own group (w % groups)."""
    X = np.asarray(L0, dtype=np.float64)
    X = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-30)
    S = X @ X.T
    np.fill_diagonal(S, -np.inf)
    top = np.argsort(-S, axis=1)[:, :k]
    own = (np.arange(X.shape[0]) % groups)[:, None]
    return float(np.mean(np.all(top % groups == own, axis=1)))


def init_L0(seed, V, d):
    """w2v.py:135-138: |N(0, 1 / d^2)|"""
    return np.abs(np.random.default_rng(seed).normal(scale=1.0 / (d ** 2), size=(V, d))).astype(np.float32)


def write_opt(opt):
    import tempfile
    f = tempfile.NamedTemporaryFile(mode="w", suffix=".json", delete=False)
    json.dump(opt, f)
    f.close()
    return f.name


# ------------------------------------------------------------------------------------------------
# the parity cases shared by tests/test_w2v_ref_cpu.py (every dot safe) and tests/test_w2v_gpu.py (device against float64)
# ------------------------------------------------------------------------------------------------
# seed of every (d, num_negative_samples) case: the first seed >= 0 whose float64 run has only safe dots (tests/test_w2v_ref_cpu.py checks it)
PARITY_SEEDS = {(20, 0): 0, (20, 2): 1, (20, 5): 0, (100, 0): 1, (100, 2): 0, (100, 5): 0, (128, 0): 1, (128, 2): 0, (128, 5): 0,
                (200, 0): 1, (200, 2): 0, (200, 5): 0}
PAIRS_SEEDS = {20: 0, 128: 0, 200: 0}


def parity_case(d, num_neg, seed=None):
    """A tiny stream (V about 24) with OOV words, subsampling and several jobs per call; at most about 500 dots."""
    seed = PARITY_SEEDS[(d, num_neg)] if seed is None else seed
    small = d <= 64
    rng = np.random.default_rng(2000 + seed)
    sents = random_stream(1000 + seed, 26, 5 if small else 4, 8 if small else 5)
    indptr, seq = make_stream(sents)
    # the vocabulary of a larger corpus this stream is a part of: about 24 of the 26 words, the rest below min_count
    counts = np.bincount(seq, minlength=26) + rng.integers(0, 40, size=26)
    vocab = build_vocab(counts, min_count=4, sample=0.02)
    vocab["total_word_count"] = int(seq.shape[0])     # the schedule and the epoch counter run over THIS stream
    epochs = 2 if num_neg == 0 or (small and num_neg <= 2) else 1
    opt = {"d": d, "window": 3 if small else 2, "num_negative_samples": num_neg, "num_iters": epochs, "lr": 0.05, "min_lr": 0.01,
           "random_seed": seed, "batch_size": 8, "compute_loss_on_training": True, "num_workers": 1}
    sigma = 0.1 if small else 0.05
    V = vocab["size"]
    L0 = rng.normal(scale=sigma, size=(V, d)).astype(np.float32)
    L1 = rng.normal(scale=sigma, size=(V, d)).astype(np.float32)
    return {"opt": opt, "vocab": vocab, "indptr": indptr, "seq": seq, "L0": L0, "L1": L1, "epochs": epochs}


def run_case(case, table, dtype, batches=None):
    return train(case["opt"], case["vocab"], case["indptr"], case["seq"], case["L0"], table, dtype, case["L1"], case["epochs"], batches)


def pairs_case(d, seed=None):
    """Explicit pairs for bfh_w2v_update_pairs: a repeated output row, a dot above 6 and one below -6."""
    seed = PAIRS_SEEDS[d] if seed is None else seed
    rng = np.random.default_rng(3000 + seed)
    V, sigma = 12, 0.1 if d <= 64 else 0.05
    L0 = rng.normal(scale=sigma, size=(V, d)).astype(np.float32)
    L1 = rng.normal(scale=sigma, size=(V, d)).astype(np.float32)
    n2 = float(np.dot(L0[0].astype(np.float64), L0[0].astype(np.float64)))
    L1[1] = (L0[0] * (8.0 / n2)).astype(np.float32)      # f = 8
    L1[2] = (L0[0] * (-8.0 / n2)).astype(np.float32)     # f = -8
    inputs = np.array([0, 3, 4, 3, 5, 6], dtype=np.int32)
    outputs = np.array([[1, 2, 7, 8], [5, 9, 9, 10], [6, 7, 8, 9], [4, 4, 11, 5], [3, 10, 11, 7], [8, 9, 10, 8]], dtype=np.int32)
    opt = {"d": d, "window": 2, "num_negative_samples": 3, "num_iters": 1, "lr": 0.05, "min_lr": 0.05, "random_seed": 0,
           "compute_loss_on_training": True, "num_workers": 1}
    vocab = {"index": np.arange(1, V + 1, dtype=np.int32), "scale": np.full(V, 0xFFFFFFFF, dtype=np.uint32),
             "dist": np.linspace(1, 0x7FFFFFFF, V).astype(np.int32), "size": V, "total_word_count": 100}
    return {"opt": opt, "vocab": vocab, "L0": L0, "L1": L1, "inputs": inputs, "outputs": outputs, "alpha": 0.05}


def run_pairs_case(case, table, dtype):
    t = Trainer(case["opt"], case["vocab"], case["L0"], table, dtype, case["L1"])
    t.update_pairs(case["inputs"], case["outputs"], case["alpha"])
    return t


PARITY_DIMS = (20, 100, 128, 200)
PARITY_NEGS = (0, 2, 5)


class RefW2V:
    """The float64 restatement behind CyW2V's method surface (buffalo/algo/_w2v.pyx), so the front of
    tests/front_harness/buffalo_front/algo/w2v.py can drive it.  `join` rewrites the caller's float32 L0."""

    def init(self, opt_path):
        with open(opt_path.decode() if isinstance(opt_path, bytes) else opt_path) as f:
            self.opt = json.load(f)
        return True

    def initialize_model(self, L0, index, scale, dist, total_word_count):
        from buffalo_amd.backend import CyW2V
        self.L0_host = L0
        vocab = {"index": index, "scale": scale, "dist": dist, "size": L0.shape[0], "total_word_count": int(total_word_count)}
        self.t = Trainer(self.opt, vocab, L0, CyW2V.exp_table(), np.float64, fast=True)

    def launch_workers(self):
        self.t.launch_workers()

    def add_jobs(self, start_x, next_x, indptr, sequences):
        whole = np.zeros(int(indptr[-1]), dtype=np.int32)
        beg = 0 if start_x == 0 else int(indptr[start_x - 1])
        whole[beg:beg + sequences.shape[0]] = sequences
        self.t.add_jobs(start_x, next_x, indptr, whole)

    def join(self):
        self.L0_host[:] = self.t.L0.astype(np.float32)
        return self.t.join()
