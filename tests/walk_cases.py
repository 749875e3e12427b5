"""Closed-slice matrices for the item-major BPRMF walk (csrc/bpr_item_major.hpp), and the designs the walk tests run on them.

A slice is 64 // nn entries of one queue in item order; one wave (one half-wave of the two-triples kernel) walks it sequentially.
Here every slice is a closed COMPONENT: its users, its positive items and -- where the draw allows: `ref_walk.classify` -- its
negatives are touched by no triple of another slice, so whatever the schedule each component has one possible result, the sequential
replay of its own triples in walk order (`ref_walk.replay`).

What makes slice == component for 1, 2, 4 and 8 queues (held in test_bpr_walk_ref_cpu.py against the library's own plan):
  * the users of a component are all = r (mod 8) for one r: one queue, whatever the number of queues;
  * its items are consecutive ids nobody else has, so its entries are contiguous in the queue's item order;
  * every full component has exactly E = 64 // nn entries;
  * the one partial component (`tail`) has the highest item ids of the matrix: it is the last slice of its queue.

Kinds (what each is there for; lengths for nn = 1, E = 64 / nn = 3, E = 21):
  run         1 item x E users            one run over the whole slice: every flush interval, the fold-in behind every flush
  grid        8 items x 8 users           (nn = 1 only) runs of 8, the item changes mid-slice, every user is back after 8 steps
  two_users   E/2 items x 2 users         the user of two steps ago at every step (`prev2` of the prefetching one-triple kernel)
  heavy_user  1 user x E items            P[u] carried / re-read at every step; the row the collision rule flags hot
  ragged      runs of 1 2 3 5 8 13 32     the flush counters across runs of differing length (nn = 3: 1 2 3 5 10); the users come from
              over 32 shared users        a pool as large as the longest run -- an item cannot have a user twice
  tail        fewer than E entries        the partial slice
"""
import numpy as np

KINDS = ("run", "grid", "two_users", "heavy_user", "ragged")
RAGGED = {64: (1, 2, 3, 5, 8, 13, 32), 21: (1, 2, 3, 5, 10)}
TAIL = (3, 1, 4)          # runs of the partial component: 8 entries


def _local(kind, E):
    """(user, item) pairs of one component in local ids."""
    if kind == "run":
        return [(k, 0) for k in range(E)]
    if kind == "grid":
        assert E == 64
        return [(u, i) for i in range(8) for u in range(8)]
    if kind == "two_users":
        return [(u, i) for i in range(E // 2) for u in range(2)] + ([(0, E // 2)] if E % 2 else [])
    if kind == "heavy_user":
        return [(0, i) for i in range(E)]
    runs = TAIL if kind == "tail" else RAGGED[E]
    pool, out, at = max(runs), [], 0
    for i, n in enumerate(runs):
        out += [((at + k) % pool, i) for k in range(n)]
        at += n
    return out


class Case:
    """csr, and per entry (nnz position) its component; per component its kind, residue, users and items."""


def build(nn, copies, tail_residue, num_items, first_item=4096):
    """`copies` components of every kind, their residues dealt round-robin (kind k, copy c -> (k + c * 3) mod 8), then the tail."""
    from buffalo_amd.synth import CSR
    E = 64 // nn
    kinds = [k for k in KINDS if not (k == "grid" and E != 64)]
    comps = [(k, (ki + c * 3) % 8) for c in range(copies) for ki, k in enumerate(kinds)] + [("tail", tail_residue)]
    next_slot = [1] * 8                      # user r (slot 0) of every residue stays without entries
    item = first_item
    ent_u, ent_i, ent_c = [], [], []
    case = Case()
    case.kind, case.residue, case.users, case.items = [], [], [], []
    for c, (kind, r) in enumerate(comps):
        loc = _local(kind, E)
        assert len(loc) == E or kind == "tail"
        nu, ni = 1 + max(u for u, _ in loc), 1 + max(i for _, i in loc)
        users = r + 8 * (next_slot[r] + np.arange(nu))
        next_slot[r] += nu
        items = item + np.arange(ni)
        item += ni
        ent_u += [users[u] for u, _ in loc]
        ent_i += [items[i] for _, i in loc]
        ent_c += [c] * len(loc)
        case.kind.append(kind); case.residue.append(r); case.users.append(users); case.items.append(items)
    assert item < num_items
    U = 8 * (max(next_slot) + 1)
    ent_u, ent_i, ent_c = np.array(ent_u), np.array(ent_i), np.array(ent_c)
    o = np.lexsort((ent_i, ent_u))           # CSR order: by user, keys ascending
    deg = np.bincount(ent_u, minlength=U)
    case.csr = CSR(U, num_items, np.cumsum(deg, dtype=np.int64), ent_i[o].astype(np.int32), np.ones(o.size, np.float32))
    case.comp = ent_c[o]                     # component of every nnz position
    case.nn, case.E, case.n_comp = nn, E, len(comps)
    return case


def walk_positions(case, c):
    """nnz positions of component c in walk order: by item, then by position (the regrouping's sort is stable)."""
    pos = np.flatnonzero(case.comp == c)
    return pos[np.argsort(case.csr.keys[pos], kind="stable")]


def slices_of(case, nq):
    """The slices of every queue as lists of nnz positions, cut from helpers.item_major_order (one wave's order over the library's
    own plan); returns [(queue, slice index, positions)]."""
    import helpers as H
    from test_schedule_cpu import plan
    csr, nn = case.csr, case.nn
    order = H.item_major_order(csr, nq, 1, nn)
    entries = np.bincount(csr.rows() % nq, minlength=nq)
    slice_len, segments, slices, stride = plan([int(e) for e in entries], nn, 1 << 40)
    assert slice_len == case.E * nn
    out, at = [], 0
    for x in range(nq):
        for ticket in range(int(slices[x])):
            sl = (ticket * int(stride[x])) % int(slices[x])
            n = min(slice_len, int(entries[x]) * nn - sl * slice_len)
            trip = order[at:at + n]
            at += n
            assert np.array_equal(trip % nn, np.tile(np.arange(nn), n // nn))
            out.append((x, sl, trip[::nn] // nn))
    assert at == order.size
    return out


def pairings(case, nq, sync):
    """What the two half-waves of the two-triples walk are handed, over every queue and merge segment: it takes the tickets of a
    segment two at a time (half 0: the even one)."""
    from test_schedule_cpu import plan
    entries = np.bincount(case.csr.rows() % nq, minlength=nq)
    slice_len, segments, slices, stride = plan([int(e) for e in entries], case.nn, sync)
    seen = {"partial_half0": False, "partial_half1": False, "idle_half1": False, "two_full": False}
    for x in range(nq):
        n = int(slices[x])
        full = lambda t: (t * int(stride[x])) % n != n - 1 or int(entries[x]) * case.nn % slice_len == 0
        for s in range(segments):
            beg, end = n * s // segments, n * (s + 1) // segments
            for t in range(beg, end, 2):
                if t + 1 >= end:
                    seen["idle_half1"] = True
                    seen["partial_half0"] |= not full(t)
                else:
                    seen["partial_half0"] |= not full(t)
                    seen["partial_half1"] |= not full(t + 1)
                    seen["two_full"] |= full(t) and full(t + 1)
    return seen, segments


def num_items_for(vdim):
    """The catalogue the negatives are drawn from: as large as 256 MB per copy of Q allows (the walk keeps 8 replicas and their base),
    so that few draws of ~1,700 land on a row another component touches."""
    n = 1 << 19
    while n * 2 * vdim * 4 <= (1 << 28):
        n *= 2
    return n


# ---- the matrices.  "a" / "b": 36 components (nn = 3: 29), the queue of the tail with an odd / an even number of slices: at least 8
# workgroups per launch, one per XCD.  "big": 96 (77), for the calls cut into three merge segments -- a segment's launch is sized by
# ITS slices, and an XCD that receives no workgroup leaves its queue to the drain launch.  At that size only the 2 M-item catalogue
# of d = 8 keeps the components apart.  (pairings() over the designs' variants and segment cuts is asserted.)
VARIANTS = {"a": dict(copies=7, tail_residue=0), "b": dict(copies=7, tail_residue=2), "big": dict(copies=19, tail_residue=0)}
_cases = {}


def case(variant, nn, num_items):
    key = (variant, nn, num_items)
    if key not in _cases:
        _cases[key] = build(nn, num_items=num_items, **VARIANTS[variant])
    return _cases[key]


BASE_MODES = dict(hogwild_atomic=3, im_dual=1, im_blocks=1, im_user_replicas=0, im_user_hybrid=0, im_drift_budget=0,
                  xcd_stiff_q=0, xcd_stiff_b=0, xcd_stiff_p=0,
                  # the row flags follow from the waves the call counts on: pinned (20 per CU = the two-triples kernel's own occupancy),
                  # so that one "im_max_stale" / "xcd_hot_tau" gives the same flags for every kernel; nothing hot unless a design says so
                  waves_per_cu=20, xcd_hot_tau=0)
WAVES_PER_CU = 20


def inflight(num_cus, dual=True):
    """ImCall::inflight of a walk that reads its rows where it uses them (bpr.hip, im_plan_call), at 8 queues."""
    return 0.25 * (num_cus * WAVES_PER_CU / 8.0) * (2.0 if dual else 1.0)


def heavy_tau(case, num_cus):
    """"xcd_hot_tau" (permille) at which the collision rule flags the heavy users alone: between the owner-queue share of a
    `two_users` user and that of a `heavy_user` user (geometric mean)."""
    deg = np.bincount(case.csr.rows(), minlength=case.csr.num_users)
    lo = max(int(deg[case.users[c]].max()) for c in range(case.n_comp) if case.kind[c] != "heavy_user")
    assert lo < case.E
    share = np.sqrt(lo * case.E) * case.nn / (case.csr.nnz * case.nn / 8.0)
    return int(round(1000.0 * share * inflight(num_cus)))
MID_STALE = 3000       # "im_max_stale" between the two ends: flush_every of a `run` item strictly between 1 and 64 (read back and asserted)


# (sampler seed = option random_seed, seed of the start factors) where the first pair (1, 1) misses the cap of
# test_bpr_walk_ref_cpu.py::test_replay_is_the_oracle_and_the_cap_holds: searched there, on the reference alone
SEEDS = {"d96": (2, 1)}


def _d(name, d, nn=1, variant="a", epochs=1, opt=None, modes=None, expect=None):
    seed, model_seed = SEEDS.get(name, (1, 1))
    return dict(name=name, d=d, nn=nn, variant=variant, epochs=epochs, seed=seed, model_seed=model_seed, opt=opt or {}, modes=modes or {},
                expect=expect or {})


# seed = the sampler's (option random_seed), model_seed = the start factors': searched in test_bpr_walk_ref_cpu.py so that the cap holds
# on the reference alone (>= 3 clean and safe components of every kind, >= 60 % of all)
DESIGNS = [
    _d("d8", 8), _d("d40", 40), _d("d96", 96), _d("d128", 128),
    _d("d40-generic", 40, modes=dict(im_dual_generic=1)), _d("d128-generic", 128, modes=dict(im_dual_generic=1)),
    _d("d128-b", 128, variant="b"),
    _d("d96-nn3", 96, nn=3), _d("d128-nn3-b", 128, nn=3, variant="b"), _d("d40-nn3-generic", 40, nn=3, modes=dict(im_dual_generic=1)),
    _d("d128-nobias", 128, opt=dict(use_bias=False)),
    _d("d128-frozen-i", 128, opt=dict(update_i=False), modes=dict(im_max_stale=1)),
    _d("d96-frozen-j", 96, opt=dict(update_j=False)),
    _d("d128-stale1", 128, modes=dict(im_max_stale=1), expect=dict(flush="one")),
    _d("d128-stale-mid", 128, modes=dict(im_max_stale=MID_STALE), expect=dict(flush="mid")),
    _d("d128-stale-inf", 128, modes=dict(im_max_stale=10 ** 6), expect=dict(flush="64")),
    _d("d96-nn3-stale-mid", 96, nn=3, modes=dict(im_max_stale=MID_STALE), expect=dict(flush="mid")),
    _d("d128-cold", 128, modes=dict(xcd_hot_tau=0), expect=dict(hot="none")),
    _d("d128-all-hot", 128, modes=dict(xcd_hot_tau=1, im_max_stale=MID_STALE), expect=dict(hot="all")),
    _d("d128-heavy-hot", 128, modes=dict(xcd_hot_tau="heavy", im_max_stale=MID_STALE), expect=dict(hot="heavy")),
    _d("d40-nn3-heavy-hot", 40, nn=3, modes=dict(xcd_hot_tau="heavy"), expect=dict(hot="heavy")),
    _d("d8-segments", 8, variant="big", modes=dict(xcd_sync_updates="third", im_max_stale=MID_STALE * 3), expect=dict(segments=3)),
    # 25 slices per segment are 7 workgroups: one XCD's queue is left to the drain launch, which flushes at every step -- so does the
    # walk here ("im_max_stale" = 1), and the replay need not know which kernel took a component
    _d("d8-nn3-segments", 8, nn=3, variant="big", modes=dict(xcd_sync_updates="third", im_max_stale=1), expect=dict(segments=3)),
    _d("d8-two-epochs", 8, epochs=2, modes=dict(im_max_stale=MID_STALE)),
    _d("d8-two-epochs-presample1", 8, epochs=2, modes=dict(im_presample=1)),
    _d("d8-nn3-two-epochs", 8, nn=3, epochs=2),
    # the one-triple kernels under many waves, same matrices
    _d("single-d128", 128, modes=dict(im_dual=0, prefetch=0, im_max_stale=MID_STALE)),
    _d("single-d128-prefetch", 128, modes=dict(im_dual=0, prefetch=1, im_max_stale=MID_STALE)),
    _d("single-d200", 200, modes=dict(im_dual=0, prefetch=0)),
    _d("single-d200-prefetch-nn3", 200, nn=3, modes=dict(im_dual=0, prefetch=1, im_max_stale=MID_STALE)),
]
BY_NAME = {x["name"]: x for x in DESIGNS}


def vdim_of(d):
    return ((d + 31) // 32) * 32
