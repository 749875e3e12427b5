"""PLSI front: what stock buffalo's `buffalo/algo/plsi.py` asks of `CyPLSI`, reduced to the training loop (`_iterate`: reset -> partial_update
per rowwise batch -> normalize -> swap), `normalize(group)`, `_get_scores` and the top-k of the common base.  Imported by module path
(`buffalo_front.algo.plsi`)."""
import numpy as np

from buffalo_amd.backend import CyPLSI
from ..misc import Option
from .base import Algo, Evaluable
from .options import AlgoOption


class PLSIOption(AlgoOption):
    def get_default_option(self):  # options.py:359-385
        opt = super().get_default_option()
        opt.update({
            "d": 20, "num_iters": 10, "num_workers": 1, "alpha1": 1.0, "alpha2": 1.0, "eps": 1e-10, "model_path": "",
            "save_factors": False, "data_opt": {}, "inherit_opt": {},
        })
        return Option(opt)


class PLSI(Algo, PLSIOption, Evaluable):
    backend = CyPLSI            # tests swap in the float64 restatement (tests/ref_plsi.py: RefPLSI)
    batch_rows = 0              # > 0: rowwise batches of that many rows, like BufferedDataMatrix.fetch_batch; 0: one batch

    def __init__(self, opt_path=None, *args, **kwargs):
        Algo.__init__(self)
        PLSIOption.__init__(self, *args, **kwargs)
        Evaluable.__init__(self)
        self._open("PLSI", type(self).backend, opt_path, kwargs, ["matrix"])

    def normalize(self, group="item"):  # plsi.py:56-60
        if group == "item":
            self.Q /= (np.sum(self.Q, axis=0, keepdims=True) + self.opt.eps)
        elif group == "user":
            self.P /= (np.sum(self.P, axis=1, keepdims=True) + self.opt.eps)

    def initialize(self):  # plsi.py:92-98 (inherit() is the caller's overwrite of rows + synchronize(False))
        super().initialize()
        self.init_factors()

    def init_factors(self):  # plsi.py:100-112
        assert self.data, "Did not set data"
        header = self.data.get_header()
        self.num_users, self.num_items, self.num_nnz = header["num_users"], header["num_items"], header["num_nnz"]
        self.P = np.zeros((self.num_users, self.opt.d), dtype="float32")
        self.Q = np.zeros((self.num_items, self.opt.d), dtype="float32")
        self.obj.initialize_model(self.P, self.Q)

    def _batches(self):
        g = self.data.get_group("rowwise")
        indptr = np.ascontiguousarray(g["indptr"][:], dtype=np.int64)
        keys, vals = g["key"][:], g["val"][:]
        step = self.batch_rows or self.num_users
        for a in range(0, self.num_users, step):
            b = min(self.num_users, a + step)
            beg, end = (0 if a == 0 else int(indptr[a - 1])), int(indptr[b - 1])
            yield a, b, indptr, np.ascontiguousarray(keys[beg:end], dtype=np.int32), np.ascontiguousarray(vals[beg:end], dtype=np.float32)

    def _iterate(self):  # plsi.py:131-160
        self.obj.reset()
        loss_nume = loss_deno = 0.0
        for start_x, next_x, indptr, keys, vals in self._batches():
            loss_nume += self.obj.partial_update(start_x, next_x, indptr, keys, vals)
            loss_deno += np.sum(vals)
        self.obj.normalize(self.opt.alpha1, self.opt.alpha2)
        self.obj.swap()
        return loss_nume, loss_deno

    def _epoch(self, _):
        nume, deno = self._iterate()
        return nume / (deno + self.opt.eps)

    def train(self, training_callback=None):  # plsi.py:162-190
        return self._result(self._epochs(self._epoch, training_callback, report="Loss"))

    def get_scores(self, row_col_pairs):  # plsi.py:123-125
        return {(r, c): self.P[r].dot(self.Q[c]) for r, c in row_col_pairs}

    def _get_data(self):  # plsi.py:199-202
        return super()._get_data() + [("opt", self.opt), ("Q", self.Q), ("P", self.P)]
