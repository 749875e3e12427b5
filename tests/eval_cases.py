"""Shared fixtures of the validation-evaluator tests: inputs, the old ranking path (dot_topn of topk + |seen| candidates, filtered
on the host) and the reference's metric loop (evaluate/base.py:83-126) over lists that are already filtered."""
import numpy as np

from buffalo_amd.synth import CSR


def csr_of(U, I, rows, cols):
    order = np.lexsort((cols, rows))
    rows, cols = np.asarray(rows)[order], np.asarray(cols)[order]
    cnt = np.bincount(rows, minlength=U)
    return CSR(U, I, np.cumsum(cnt, dtype=np.int64), cols.astype(np.int32), np.ones(len(cols), np.float32))


def planted(U=300, I=500, d=20, seed=5, bias=False, n_vali=400):
    """Random training matrix with user 0 WITHOUT seen items and user 1 having seen all but 3; vali pairs outside the training
    matrix, users 0 and 1 among them, some pairs listed twice."""
    rng = np.random.default_rng(seed)
    M = rng.random((U, I)) < 0.08
    M[np.arange(U), rng.integers(0, I, size=U)] = True
    M[0, :] = False
    M[1, :] = True
    M[1, rng.choice(I, size=3, replace=False)] = False
    rows, cols = np.nonzero(M)
    train = csr_of(U, I, rows, cols)
    vr = np.concatenate([[0, 0, 1], rng.integers(2, U, size=n_vali)]).astype(np.int32)
    vc = rng.integers(0, I, size=len(vr)).astype(np.int32)
    vc[2] = np.flatnonzero(~M[1])[0]
    keep = ~M[vr, vc]
    vr, vc = vr[keep], vc[keep]
    vr, vc = np.concatenate([vr, vr[:25]]), np.concatenate([vc, vc[:25]])     # duplicate pairs
    perm = rng.permutation(len(vr))
    vali = {"row": np.ascontiguousarray(vr[perm]), "col": np.ascontiguousarray(vc[perm]),
            "val": rng.integers(1, 6, size=len(vr)).astype(np.float32)}
    P = rng.normal(size=(U, d)).astype(np.float32)
    Q = rng.normal(size=(I, d)).astype(np.float32)
    Qb = rng.normal(scale=0.5, size=(I, 1)).astype(np.float32) if bias else None
    return train, vali, P, Q, Qb


def seen_of(train, u):
    beg = 0 if u == 0 else int(train.indptr[u - 1])
    return train.keys[beg:int(train.indptr[u])]


def old_path_candidates(dot_topn, train, rows, topk):
    """{row: (keys, scores)} -- the dot_topn list of min(topk + |seen_u|, I) candidates of every row (one call per distinct length).
    `dot_topn(rows, k) -> (keys [n, k], scores [n, k])` must admit every score (flt_min_rule = 0)."""
    need = np.array([min(topk + len(seen_of(train, int(u))), train.num_items) for u in rows])
    out = {}
    for k in np.unique(need):
        sel = np.flatnonzero(need == k)
        keys, scores = dot_topn(np.ascontiguousarray(np.asarray(rows)[sel], dtype=np.int32), int(k))
        for i, u in enumerate(np.asarray(rows)[sel]):
            out[int(u)] = (keys[i], scores[i])
    return out


def filtered(cands, train, rows, topk):
    """filter_seen_items (evaluate/base.py:71-78) over the old path's candidates, -1 where the unseen items run out."""
    out = np.full((len(rows), topk), -1, dtype=np.int32)
    for i, u in enumerate(rows):
        seen = set(seen_of(train, int(u)).tolist())
        keep = [int(t) for t in cands[int(u)][0] if int(t) >= 0 and int(t) not in seen][:topk]
        out[i, :len(keep)] = keep
    return out


def host_metrics(lists, rows, train, vali, topk):
    """evaluate/base.py:83-126 over filtered lists (int32 [n, topk], -1 = no entry): (ndcg, map, accuracy, auc, N) and the
    per-row values."""
    gt = {}
    for r, c in zip(vali["row"].tolist(), vali["col"].tolist()):
        gt.setdefault(r, set()).add(c)
    num_items = train.num_items
    idcgs = np.cumsum(1.0 / np.log2(np.arange(2, topk + 2)))
    dcgs = 1.0 / np.log2(np.arange(2, topk + 2))
    NDCG = AP = HIT = AUC = N = 0.0
    per_row = np.zeros((len(rows), 4))
    for b, row in enumerate(np.asarray(rows).tolist()):
        if len(seen_of(train, row)) == 0 or row not in gt:
            continue
        _topk = [t for t in lists[b].tolist() if t >= 0]
        _gt = gt[row]
        acc = len(set(_topk) & _gt) / len(_gt)
        idcg = idcgs[min(len(_gt), topk) - 1]
        dcg = hit = miss = ap = auc = 0.0
        num_pos_items = len(_gt)
        num_neg_items = num_items - num_pos_items
        for i, r in enumerate(_topk):
            if r in _gt:
                hit += 1
                ap += hit / (i + 1.0)
                dcg += dcgs[i]
            else:
                miss += 1
                auc += hit
        auc += ((hit + num_pos_items) / 2.0) * (num_neg_items - miss)
        auc /= (num_pos_items * num_neg_items)
        ap /= min(len(_gt), topk)
        per_row[b] = (dcg / idcg, ap, acc, auc)
        NDCG += dcg / idcg
        AP += ap
        HIT += acc
        AUC += auc
        N += 1.0
    if N == 0:
        return (0.0, 0.0, 0.0, 0.0, 0.0), per_row
    return (NDCG / N, AP / N, HIT / N, AUC / N, N), per_row


def hold_out(full, seed):
    """One random entry of every user with >= 2 entries moves to vali."""
    rng = np.random.default_rng(seed)
    beg = np.concatenate([[0], full.indptr[:-1]])
    deg = full.indptr - beg
    users = np.flatnonzero(deg >= 2)
    pos = beg[users] + (rng.random(len(users)) * deg[users]).astype(np.int64)
    held = np.zeros(full.nnz, dtype=bool)
    held[pos] = True
    rows = full.rows()
    vali = {"row": np.ascontiguousarray(rows[held], dtype=np.int32), "col": np.ascontiguousarray(full.keys[held]),
            "val": np.ascontiguousarray(full.vals[held])}
    cnt = np.bincount(rows[~held], minlength=full.num_users)
    return CSR(full.num_users, full.num_items, np.cumsum(cnt, dtype=np.int64), full.keys[~held], full.vals[~held]), vali
