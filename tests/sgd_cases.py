"""The matrices of the SGD accumulate stage tests (tests/test_sgd_ref_cpu.py, test_sgd_gradients_gpu.py, test_sgd_optimizer_gpu.py),
built deterministically around the bounds of csrc/sgd_kernels.hpp.  Every case carries `seen`: what it was built to contain,
computed from the matrix (and, where the sampler decides, from the yardstick's triples); the tests assert every entry.

GATHER_CHUNK is read from the library (bfh_sgd_gather_chunk, host-only): a change of kGatherChunk moves the cases with it or
fails their `seen`, it cannot silently empty them.

pattern()        521 users x 32 items, 2,597 entries.  Item-sorted positive list (C = GATHER_CHUNK = 256), by item:
                   item 0   C entries        [0, C): a run that covers a whole chunk and ends on a boundary; item 1 begins on it
                   item 1   100              [C, C + 100): crosses the 64-incidence tile at C + 64, no chunk boundary
                   item 2   300              cut by one boundary (2C)
                   item 3   2C + 8 = 520     crosses 3C and 4C: three waves flush into one gradQ row
                   item 4   103              ends at 5C - 1
                   item 5   1                the last slot of a chunk;   item 6   1   the first slot of the next
                   item 7   0                no incidence in either list under sampling_power = 1.0: gradQ / countQ stay 0
                   items 8 ... 31            54 or 55 each; the list ends 37 entries into its last chunk (odd, < 64: the UN tails)
                 Users: user 0 has one entry (a run of 1), users 1 ... 264 two (items 2, 3), users 265 ... 300 three (item 0 too),
                 users 301 ... 520 carry everything else, so that the negatives of item 2 (drawn only by users without it, in proportion to its 300 positives) form a run of more than
                 2C - 1 incidences: cut by a boundary and covering a whole chunk.  521 = 8 * 65 + 1: the user side ends on a lone row at
                 every rpw of sgd_update_rows_kernel, the 32 items on a full wave.
pattern_wide()   2,001 x 304 at 12 %: more chunks in either list than compute units, so that with gather_waves_per_cu = 1 the grid-stride
                 loop of grad_gather_kernel takes a second chunk (the test asserts n_work > multi_processor_count).
warp_pattern()   64 users x 96 items: user 0 has seen 95 items (Phi = log(max(1, 0)) = 0: accepted, counted, coefficient 0), user 1 has
                 seen 94, users 2 ... 5 87 ... 90 (their unseen candidates lie beyond the pre-drawn attempts and, for some, beyond the
                 first 64-draw batch), the rest about 10 %.
"""
import numpy as np

from buffalo_amd.synth import CSR


def gather_chunk():
    from buffalo_amd import _lib
    return int(_lib.lib().bfh_sgd_gather_chunk())


def rpw_of(vdim):
    """Rows per wave of sgd_update_rows_kernel: 64 / lane_group_of(vdim) (csrc/common.hpp)."""
    G = 8
    while G < 64 and G * 4 < vdim:
        G *= 2
    return 64 // G


def vdim_of(d):
    return (d + 31) // 32 * 32


def _csr_from_items(U, I, item_users):
    r = np.concatenate([np.asarray(us, np.int64) for us in item_users])
    c = np.concatenate([np.full(len(us), i, np.int64) for i, us in enumerate(item_users)])
    assert np.unique(r * I + c).shape[0] == r.shape[0], "an entry twice"
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    cnt = np.bincount(r, minlength=U)
    assert cnt.min() >= 1, "an empty user row"
    return CSR(U, I, np.cumsum(cnt, dtype=np.int64), c.astype(np.int32), np.ones(c.shape[0], np.float32))


def pattern():
    C = gather_chunk()
    U, I = 2 * C + 9, 32
    heavy = np.arange(301, U)                                   # 220 users
    items = [np.arange(U - C, U),                               # 0: C users, the heavy ones and 36 light ones
             np.arange(400, 500),                               # 1
             np.arange(1, 301),                                 # 2: every light user but user 0
             np.arange(0, 2 * C + 8),                           # 3: everybody but the last user
             np.arange(301, 404),                               # 4
             np.array([U - 1]), np.array([U - 1]),              # 5, 6
             np.array([], np.int64)]                            # 7
    # the list must end 37 entries into a chunk: 5C + 1 so far
    rest = 5 * C + 36
    per = [rest // 24 + (1 if j < rest % 24 else 0) for j in range(24)]
    for j, n in enumerate(per):
        assert n <= heavy.shape[0]
        items.append(heavy[(j * 37 + np.arange(n) * 3) % heavy.shape[0]])     # 3 is coprime with 220
    csr = _csr_from_items(U, I, items)
    seen = seen_positive_list(csr, C)
    seen.update(seen_user_runs(csr, 1))
    seen.update({"num_negative_samples = 3: " + k: v for k, v in seen_user_runs(csr, 3).items()})
    return dict(name="pattern", csr=csr, C=C, sampling_power=1.0, seen=seen)     # the negative list's entries: test_sgd_ref_cpu.py, from the triples


def pattern_wide():
    U, I = 2001, 304
    rng = np.random.default_rng(5)
    M = rng.random((U, I)) < 0.12
    M[:, 7] = False                                             # an item nobody has
    M[np.arange(U), 8 + rng.integers(0, I - 8, U)] = True       # no empty rows
    items = [np.flatnonzero(M[:, i]) for i in range(I)]
    csr, C = _csr_from_items(U, I, items), gather_chunk()
    seen = {"more chunks than the 256 compute units of an MI355X (the device test asks the device)": -(-csr.nnz // C) > 256,
            "an item without a positive": not (csr.keys == 7).any(),
            "num_users % 8 == 1 and num_items % 8 == 0": U % 8 == 1 and I % 8 == 0}
    return dict(name="pattern_wide", csr=csr, C=C, sampling_power=1.0, seen=seen)


def warp_pattern():
    U, I = 64, 96
    rng = np.random.default_rng(11)
    M = np.zeros((U, I), bool)
    for u, n in ((0, I - 1), (1, I - 2), (2, 90), (3, 89), (4, 88), (5, 87)):
        M[u, rng.permutation(I)[:n]] = True
    for u in range(6, U):
        M[u, rng.permutation(I)[:9 + u % 3]] = True
    items = [np.flatnonzero(M[:, i]) for i in range(I)]
    per_user = M.sum(axis=1)
    seen = {"a user who has seen I - 1 items, one I - 2": bool((per_user == I - 1).any() and (per_user == I - 2).any()),
            "four more users at 90 % and above": int((per_user >= 0.9 * I).sum()) >= 6,
            "the rest at about 10 %": bool((per_user[6:] <= 0.12 * I).all())}
    return dict(name="warp_pattern", csr=_csr_from_items(U, I, items), C=gather_chunk(), seen=seen)   # the trial loop's entries: test_sgd_ref_cpu.py


# ---------------------------------------------------------------------------------------------
# what a case contains
# ---------------------------------------------------------------------------------------------
def runs_of(sorted_items):
    """(item, begin, end) of every run of an ascending list."""
    it = np.asarray(sorted_items)
    if it.shape[0] == 0:
        return np.zeros((0, 3), np.int64)
    beg = np.flatnonzero(np.concatenate([[True], it[1:] != it[:-1]]))
    end = np.concatenate([beg[1:], [it.shape[0]]])
    return np.stack([it[beg], beg, end], axis=1)


def seen_positive_list(csr, C):
    """The runs of the item-sorted positive list against the bounds of grad_gather_kernel."""
    r = runs_of(np.sort(csr.keys.astype(np.int64), kind="stable"))
    b, e = r[:, 1], r[:, 2]
    n = csr.nnz
    crossed = (e - 1) // C - b // C                            # chunk boundaries inside the run
    tail = n % C
    return {
        "run ends on a chunk boundary and the next begins on it": bool(((e % C == 0) & (e < n)).any()),
        "run covers a whole chunk": bool(((b % C == 0) & (e - b >= C)).any() or (crossed >= 2).any()),
        "run cut by exactly one boundary": bool((crossed == 1).any()),
        "run of 2C + 1 or more on three waves": bool(((e - b >= 2 * C + 1) & (crossed >= 2)).any()),
        "one-incidence run in the last slot of a chunk": bool(((e - b == 1) & (b % C == C - 1)).any()),
        "one-incidence run in the first slot of a chunk": bool(((e - b == 1) & (b % C == 0) & (b > 0)).any()),
        "run crosses a 64-incidence tile but no chunk boundary": bool(((crossed == 0) & ((e - 1) // 64 > b // 64)).any()),
        "last chunk shorter than 64 and odd": bool(0 < tail < 64 and tail % 2 == 1),
        "an item without a positive": bool((np.bincount(csr.keys, minlength=csr.num_items) == 0).any()),
        "num_users % 8 == 1 and num_items % 8 == 0": csr.num_users % 8 == 1 and csr.num_items % 8 == 0,
    }


def seen_negative_list(neg, C, num_items, empty_item):
    r = runs_of(np.sort(np.asarray(neg, np.int64)))
    b, e = r[:, 1], r[:, 2]
    covers = (b + C - 1) // C * C + C <= e                     # the first chunk that begins inside the run also ends inside it
    return {
        "a negative run is cut by a boundary and covers a whole chunk": bool((covers & ((e - 1) // C > b // C)).any()),
        "the item without a positive is never drawn": bool((np.asarray(neg) != empty_item).all()),
    }


def seen_user_runs(csr, nn, chunk=64):
    """The user-major walk: work items of `chunk` triples."""
    beg = np.concatenate([[0], csr.indptr[:-1]]) * nn
    end = csr.indptr * nn
    return {
        "a user run of one entry": bool((csr.indptr - np.concatenate([[0], csr.indptr[:-1]]) == 1).any()),
        "a user run straddles a work item (two flushes into one gradP row)": bool(((end - 1) // chunk > beg // chunk).any()),
        "a position's slots straddle a 64-triple tile": bool(nn == 1 or ((np.arange(csr.nnz) * nn) // 64 != (np.arange(csr.nnz) * nn + nn - 1) // 64).any()),
    }


GOLDEN = (5 ** 0.5 - 1) / 2


def init_state(csr, d, seed, scale, bias="zero"):
    """Float32 factors N(0, scale^2) in d columns (the caller pads to vdim) and a bias column: "zero", "normal" (scale / 3), or
    "golden": Qb[i] = i * GOLDEN / 83.  With factors small enough that the dot does not matter, the score of a triple is then
    (pos - neg) * GOLDEN cells of the sigmoid table from 0, and a multiple of the golden ratio stays 1 / (sqrt(5) n) away from every
    integer: no triple of a case of any size lies near a cell edge, while the scores spread over hundreds of cells."""
    rng = np.random.default_rng(seed)
    P = rng.normal(scale=scale, size=(csr.num_users, d)).astype(np.float32)
    Q = rng.normal(scale=scale, size=(csr.num_items, d)).astype(np.float32)
    Qb = np.zeros((csr.num_items, 1), np.float32)
    if bias == "normal":
        Qb = rng.normal(scale=scale / 3, size=(csr.num_items, 1)).astype(np.float32)
    elif bias == "golden":
        Qb = (np.arange(csr.num_items) * GOLDEN / 83.0).astype(np.float32).reshape(-1, 1)
    return P, Q, Qb


def design_state(ds, csr):
    return init_state(csr, ds["d"], SEEDS[ds["name"]], ds["scale"], ds["bias"] if ds["use_bias"] else "zero")


# ---------------------------------------------------------------------------------------------
# the designs the stage tests run (device: test_sgd_gradients_gpu.py; CPU: test_sgd_ref_cpu.py holds the yardstick to the oracle
# on every one of them and asserts unsafe == 0 for the seed of SEEDS)
# ---------------------------------------------------------------------------------------------
def bpr_design(name, optimizer, d, nn, scale, lr, two_pass=1, n_chunks=1, resident=False, update_i=True, update_j=True, use_bias=True,
               case="pattern", gather_waves_per_cu=0, inject=False, bias="normal", reg=0.025, epochs=2, seed_of=None):
    return dict(name=name, optimizer=optimizer, d=d, nn=nn, scale=scale, lr=lr, two_pass=two_pass, n_chunks=n_chunks, resident=resident,
                update_i=update_i, update_j=update_j, use_bias=use_bias, case=case, gather_waves_per_cu=gather_waves_per_cu, inject=inject, bias=bias, reg=reg, epochs=epochs, seed_of=seed_of)


# d 20 / 200 / 320 / 520: K = 1, 4, 8, 16 of grad_gather_kernel (UN 8, 8, 4, 2) and rpw 8, 1, 1, 1.  The factor scale and lr fall with
# d: the float32 dot error grows with d while a cell of the sigmoid table stays 1/83 wide, and `unsafe` must be 0 (ref_sgd.py).  At
# d = 520, and on the 72,000 triples of `pattern_wide`, no model seed leaves every triple at twice that distance: there the scores
# come from golden-ratio biases (init_state); reg = 0 at d = 520, where among 270,000 tiny gradients one would cancel against 2 reg x to
# the size of FEPS and turn the step's fourth digit into a matter of contraction (the optimizer tests carry the reg term).
BPR_DESIGNS = [
    bpr_design("adagrad-d20-nn2", "adagrad", 20, 2, 0.1, 0.02),
    bpr_design("adam-d20-nn3-atomic", "adam", 20, 3, 0.1, 0.02, two_pass=0),
    # the same with another model: on this one gradQb[3], 1,566 same-sign terms in hardware order, lands at 3.6 ... 4.0 x the oracle's own
    # draw (ref_sgd.order_term).  One epoch: its second has two triples inside twice the unsafe distance.
    bpr_design("adam-d20-nn3-atomic-seed4", "adam", 20, 3, 0.1, 0.02, two_pass=0, epochs=1),
    bpr_design("adagrad-d200-nn1-chunks3", "adagrad", 200, 1, 0.01, 0.002, n_chunks=3),
    bpr_design("adam-d200-nn2-resident-no_update_i", "adam", 200, 2, 0.01, 0.002, resident=True, update_i=False),
    bpr_design("adagrad-d320-nn2-no_update_j", "adagrad", 320, 2, 0.01, 0.002, update_j=False),
    bpr_design("adam-d320-nn1-atomic-chunks3-no_bias", "adam", 320, 1, 0.01, 0.002, two_pass=0, n_chunks=3, use_bias=False),
    bpr_design("adagrad-d520-nn2-resident", "adagrad", 520, 2, 3e-4, 1e-6, resident=True, bias="golden", reg=0.0),
    bpr_design("adam-d520-nn2", "adam", 520, 2, 3e-4, 1e-6, bias="golden", reg=0.0),
    bpr_design("wide-adagrad-d20-nn1", "adagrad", 20, 1, 3e-4, 1e-6, case="pattern_wide", gather_waves_per_cu=1, bias="golden"),
    bpr_design("inject-adagrad-d20-nn1", "adagrad", 20, 1, 0.3, 0.05, two_pass=0, inject=True),
]

# (max_trials, threshold): the violating candidate's index k reaches 1 ... 5 and, at max_trials 20, 8 and more (the 1 / 2 / 4 / 4
# speculation batches of warp_update_kernel); 1 and 2 accept nothing (Q-10: trial = 2k >= max_trials), 3 and 4 only k = 1
WARP_TRIALS = [(1, 0.0), (2, 0.0), (3, 0.0), (4, 0.0), (12, 0.0), (20, 0.0), (12, -1e9), (12, 1e9)]
WARP_D, WARP_SCALE = 24, 0.3

# model seed per design: the first for which both epochs have unsafe_2x == 0 (searched on the CPU with the float32 restatement
# carrying the state from the first epoch to the second)
SEEDS = {"adagrad-d20-nn2": 15, "adam-d20-nn3-atomic": 88, "adam-d20-nn3-atomic-seed4": 4, "adagrad-d200-nn1-chunks3": 7, "adam-d200-nn2-resident-no_update_i": 36,
         "adagrad-d320-nn2-no_update_j": 28, "adam-d320-nn1-atomic-chunks3-no_bias": 24, "adagrad-d520-nn2-resident": 1, "adam-d520-nn2": 1,
         "wide-adagrad-d20-nn1": 1, "inject-adagrad-d20-nn1": 43, "warp": 2}


def hardware_order(ds):
    """Every gradient term of the design is its own atomic add: ref_sgd.stage_bound carries the order term."""
    return bool(ds["inject"] or not ds["two_pass"])


def make_case(name):
    return {"pattern": pattern, "pattern_wide": pattern_wide, "warp_pattern": warp_pattern}[name]()


def bpr_options(ds):
    """conftest.bpr_opt's keys for a design (the caller merges them into the defaults)."""
    return dict(d=ds["d"], optimizer=ds["optimizer"], lr=ds["lr"], num_iters=2, random_seed=3, num_negative_samples=ds["nn"], sampling_power=1.0,
                per_coordinate_normalize=True, update_i=ds["update_i"], update_j=ds["update_j"], use_bias=ds["use_bias"],
                reg_u=ds["reg"], reg_i=ds["reg"], reg_j=ds["reg"], reg_b=ds["reg"])


def warp_options(score_func, max_trials, threshold, optimizer="adagrad"):
    return dict(d=WARP_D, optimizer=optimizer, lr=0.05, num_iters=2, random_seed=5, score_func=score_func, max_trials=max_trials, threshold=threshold,
                per_coordinate_normalize=True, reg_u=0.01, reg_i=0.02, reg_j=0.01)


# ---------------------------------------------------------------------------------------------
# the drawn inputs of the optimizer step (device: test_sgd_optimizer_gpu.py; CPU: the step defects of test_sgd_ref_cpu.py)
# ---------------------------------------------------------------------------------------------
SPECIAL_GRADS = np.array([1e-12, 1e-10, 1.0, 1e6], np.float32)


def step_rng(kind, optimizer, vdim):
    """The one generator both files draw a (kind, optimizer, vdim) case from: P's first call, Q's first call, then the second calls."""
    return np.random.default_rng(vdim + 7 * (optimizer == "adam") + 13 * (kind == "warp"))


def step_rows(vdim):
    rpw = rpw_of(vdim)
    return {"P": 4 * rpw + 1, "Q": max(1, rpw - 1)}


def draw_step_inputs(rng, rows, d, warp, signs=None):
    """One call's inputs for a matrix of `rows` rows and its bias column: (X, Xb, grad, gradb, counts, signs).  No element cancels.
    BPRMF: a gradient has the sign opposite to its X in both calls (g - 2 reg X adds magnitudes; beta mom + (1 - beta) g likewise) and
    0.15 <= |X| <= 0.4 stays above two steps of lr = 0.05 (|step| <= 1 under adagrad, and under adam with beta2 read from beta1).
    WARP (reg = 0, and the projection shrinks X below that margin): the gradient has the sign OF its X, so X + lr step adds magnitudes.
    The elementwise error relative to |f64| then measures the kernel's roundings, not how close an output happens to lie to 0."""
    if signs is None:
        signs = (rng.choice([-1.0, 1.0], size=(rows, d)), rng.choice([-1.0, 1.0], size=rows))
    sg, sb = signs
    X = (sg * rng.uniform(0.15, 0.4, size=(rows, d))).astype(np.float32)
    Xb = (sb * rng.uniform(0.15, 0.4, size=rows)).astype(np.float32)
    gs = sg if warp else -sg
    g = (gs * np.abs(rng.normal(size=(rows, d))) * 10.0 ** rng.uniform(-3, 1, size=(rows, d))).astype(np.float32)
    gb = (-sb * np.abs(rng.normal(size=rows)) * 10.0 ** rng.uniform(-3, 1, size=rows)).astype(np.float32)
    X[:, :4] = 0
    g[:, :4] = SPECIAL_GRADS
    cnt = rng.integers(1, 6, size=rows).astype(np.int32)
    cnt[0] = 0
    if warp and rows >= 5:
        g[1:5] = 0
        for r, nrm in zip(range(1, 5), (0.5, 1.0, 1.0 + 2.0 ** -20, 30.0)):
            if nrm in (1.0, 1.0 + 2.0 ** -20):
                X[r] = 0
                X[r, 5] = nrm
            else:
                X[r] = (X[r] / np.linalg.norm(X[r].astype(np.float64)) * nrm).astype(np.float32)
    return X, Xb, g, gb, cnt, signs
