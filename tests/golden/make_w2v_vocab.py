"""Golden vocabularies of Word2Vec, made with the REFERENCE's own `W2V.build_vocab` / `get_sampling_distribution`
(buffalo/algo/w2v.py:91-157).  The module is imported unmodified from /root/reference with the stubs of make_front_traces.py
(`install_reference`); the two methods run on a stand-in for `self` that carries what they touch: the header, a one-batch buffer
over the stream, the options min_count / sample and a logger.  Recorded per stream: counts, index, scale, dist, total_word_count.
`tests/test_w2v_ref_cpu.py` requires tests/ref_w2v.build_vocab to give the same bits.  Run from the repo root:
    python tests/golden/make_w2v_vocab.py
"""
import logging
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# name: (stream seed, words, tokens, zipf exponent, min_count, sample)
STREAMS = {
    "w2v_vocab_small": (1, 30, 400, 1.1, 3, 0.01),
    "w2v_vocab_no_sample": (2, 50, 900, 0.8, 1, 0.0),
}


def stream(seed, words, tokens, expo):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, words + 1) ** expo
    return rng.choice(words, size=tokens, p=p / p.sum()).astype(np.int32)


def reference_vocab(keys, num_items, min_count, sample):
    import make_front_traces as ft
    ft.install_reference()
    from buffalo.algo.w2v import W2V

    class Buf:
        def fetch_batch(self):
            yield keys.shape[0]

        def get(self):
            return 0, 1, np.array([keys.shape[0]], dtype=np.int64), keys

    me = types.SimpleNamespace(data=types.SimpleNamespace(get_header=lambda: {"num_items": num_items}), buf=Buf(),
                               opt=types.SimpleNamespace(min_count=min_count, sample=sample), logger=logging.getLogger("w2v-golden"),
                               _vocab=types.SimpleNamespace())
    me.get_sampling_distribution = types.MethodType(W2V.get_sampling_distribution, me)
    W2V.build_vocab(me)
    return me._vocab


def main():
    for name, (seed, words, tokens, expo, min_count, sample) in STREAMS.items():
        keys = stream(seed, words, tokens, expo)
        v = reference_vocab(keys, words, min_count, sample)
        np.savez(os.path.join(HERE, name + ".npz"), counts=np.bincount(keys, minlength=words).astype(np.int64), index=v.index, scale=v.scale,
                 dist=v.dist, total_word_count=np.int64(v.total_word_count), min_count=np.int64(min_count), sample=np.float64(sample))
        print(name, "vocab", v.size, "of", words, "total", v.total_word_count)


if __name__ == "__main__":
    main()
