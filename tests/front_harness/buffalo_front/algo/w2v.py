"""W2V front: what stock buffalo's `buffalo/algo/w2v.py` asks of `CyW2V`, reduced to `initialize` (vocabulary, factors, model binding),
`train` (launch_workers -> add_jobs per rowwise batch and iteration -> join), `get_index` / `get_feature` through the vocabulary and
`most_similar`.  The option defaults sit here; imported by module path (`buffalo_front.algo.w2v`)."""
import numpy as np

from buffalo_amd.backend import CyW2V
from ..misc import Option
from .base import EPS, Algo, Evaluable
from .options import AlgoOption


class W2VOption(AlgoOption):
    def get_default_option(self):  # options.py:319-352
        opt = super().get_default_option()
        opt.update({
            "evaluation_on_learning": False, "num_workers": 1, "num_iters": 3, "d": 20, "window": 5, "min_count": 5, "sample": 0.001,
            "num_negative_samples": 5, "lr": 0.025, "min_lr": 0.0001, "model_path": "", "data_opt": {},
        })
        return Option(opt)


class W2V(Algo, W2VOption, Evaluable):
    backend = CyW2V             # tests swap in the float64 restatement (tests/ref_w2v.py: RefW2V)
    batch_rows = 0              # > 0: batches of that many sentences, like BufferedDataStream.fetch_batch; 0: one batch

    def __init__(self, opt_path=None, *args, **kwargs):
        Algo.__init__(self)
        W2VOption.__init__(self, *args, **kwargs)
        Evaluable.__init__(self)
        self._open("W2V", type(self).backend, opt_path, kwargs, ["stream"])
        self._vocab = Option({"size": 0, "index": None, "inv_index": None, "scale": None, "dist": None, "total_word_count": 0})

    def normalize(self, group="item"):  # w2v.py:61-64
        self._normalize_once(group, {"item": ("L0", "_nrz_L0")})

    def get_index(self, key, group="item"):  # w2v.py:66-74: the position in the id map, then the vocabulary; None below min_count
        many = isinstance(key, list)
        found = super().get_index(key if many else [key], group)
        found = [None if i is None or self._vocab.index[i] < 1 else int(self._vocab.index[i]) - 1 for i in found]
        return found if many else found[0]

    def get_feature(self, name, group="item"):  # base.py:181-185 + w2v.py:76-79
        index = self.get_index(name, group)
        return None if index is None or group != "item" else self.L0[index]

    def _stream(self):
        g = self.data.get_group("rowwise")
        return np.ascontiguousarray(g["indptr"][:], dtype=np.int64), np.ascontiguousarray(g["key"][:], dtype=np.int32)

    def initialize(self):  # w2v.py:81-89
        super().initialize()
        assert self.data, "Data is not set"
        self.build_vocab()
        self.init_factors(self._vocab.size)
        self.obj.initialize_model(self.L0, self._vocab.index, self._vocab.scale, self._vocab.dist, self._vocab.total_word_count)

    def build_vocab(self):  # w2v.py:91-133
        num_items = self.data.get_header()["num_items"]
        _, keys = self._stream()
        uni = np.bincount(keys, minlength=num_items).tolist()
        use, total_vocab = [0] * num_items, 0
        for i in range(num_items):
            if uni[i] >= self.opt.min_count:
                total_vocab += 1
                use[i] = total_vocab
        scale = np.zeros(shape=total_vocab, dtype=np.uint32)
        threshold_count = sum(uni[i] for i in range(num_items) if use[i])
        if self.opt.sample > 0.0:
            threshold_count *= self.opt.sample
        for i in range(num_items):
            if use[i]:
                p = (((uni[i] / threshold_count) ** 0.5) + 1) * (threshold_count / uni[i])
                scale[use[i] - 1] = (p if p < 1.0 else 1.0) * 0xFFFFFFFF
        v = self._vocab
        v.size, v.scale, v.index = total_vocab, scale, np.array(use, dtype=np.int32)
        v.inv_index = np.array([idx for idx, u in enumerate(use) if u > 0], dtype=np.int32)
        v.dist = self.get_sampling_distribution(uni, use, total_vocab)
        v.total_word_count = int(keys.shape[0])

    def get_sampling_distribution(self, uni, use, total_vocab):  # w2v.py:140-157
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
        assert abs(dist[-1] - 0x7FFFFFFF) < 3
        return dist

    def init_factors(self, vocab_size):  # w2v.py:135-138
        self.L0 = np.abs(np.random.normal(scale=1.0 / (self.opt.d ** 2), size=(vocab_size, self.opt.d)).astype("float32"))

    def _iterate(self):  # w2v.py:174-191
        indptr, keys = self._stream()
        n = indptr.shape[0]
        step = self.batch_rows or n
        for a in range(0, n, step):
            b = min(n, a + step)
            beg, end = (0 if a == 0 else int(indptr[a - 1])), int(indptr[b - 1])
            self.obj.add_jobs(a, b, indptr, np.ascontiguousarray(keys[beg:end]))

    def train(self, training_callback=None):  # w2v.py:193-202
        self.validation_result = {}
        self.obj.launch_workers()
        for _ in range(self.opt.num_iters):
            self._iterate()
        self.train_loss = self.obj.join()
        return {}

    def most_similar(self, key, topk=10, pool=None):
        """base.py:89-155 + w2v.py:162-169 for one item key: [(key, cosine)] best first, the query itself left out."""
        if not self._idmanager.itemid_mapped:
            self.build_itemid_map()
        col = self.get_index(key)
        if col is None:
            return []
        F = self.L0 if pool is None else self.L0[[i for i in self.get_index(list(pool)) if i is not None]]
        ids = np.arange(self.L0.shape[0]) if pool is None else np.array([i for i in self.get_index(list(pool)) if i is not None])
        q = self.L0[col]
        dot = F.dot(q)
        if not self.opt.get("_nrz_L0"):
            dot = dot / (np.linalg.norm(q) * np.linalg.norm(F, axis=1) + EPS)
        top = self.get_topk(dot, k=min(topk + 1, dot.shape[0]))
        names = self._idmanager.itemids
        return [(names[int(self._vocab.inv_index[ids[t]])], float(dot[t])) for t in top if ids[t] != col][:topk]

    def get_scores(self, row_col_pairs):  # w2v.py:171-172
        return []

    def _get_data(self):  # w2v.py:204-209
        return super()._get_data() + [("opt", self.opt), ("L0", self.L0), ("_vocab", self._vocab)]
