"""Stream databases restated in plain Python (TEST INFRASTRUCTURE, not collected) + the case generators of test_stream_ref_cpu.py and
test_stream_gpu.py.  `restate` is written from /root/reference/buffalo/data/stream.py:197-271 (and :120-122 for the names) with str.split, a
dict and collections.Counter; tests/test_stream_ref_cpu.py pins it to the databases the reference's own Stream.create() built."""
import io
from collections import Counter

import numpy as np


def lines_of(data):
    """The lines of `data` as Python's text mode reads a file (universal newlines, UTF-8)."""
    return list(io.TextIOWrapper(io.BytesIO(data), encoding="utf-8", newline=None))


def restate(names, text, vali_n=0, sample_positions=None):
    """names / text: bytes of the item-id file and of the main file.  Raises KeyError((line, token)) for the first unknown token."""
    name_lines = lines_of(names)
    itemids = {line.strip(): idx for idx, line in enumerate(name_lines)}                  # stream.py:120-122, 0-based
    if len(itemids) != len(name_lines):
        raise ValueError("duplicate names")
    held = set(int(p) for p in sample_positions) if sample_positions is not None else set()
    tokens, total, indptr, events, records, vali = 0, 0, [], [], [], []
    for user, line in enumerate(lines_of(text)):
        data = line.strip().split()
        for tok in data:
            if tok not in itemids:
                raise KeyError((user + 1, tok))
        tokens += len(data)
        vali_data, train = [], []
        if vali_n > 0:                                                                    # :224-231
            cut = len(data) - min(vali_n, len(data) - 1)
            vali_data = [itemids[c] for c in Counter(data[cut:])]
            data = data[:cut]
        for idx, tok in enumerate(data):                                                  # :239-246
            (vali_data if idx + total in held else train).append(itemids[tok])
        total += len(data)
        events += train
        indptr.append(len(events))
        records += [(user, c, v) for c, v in Counter(train).items()]                      # :253-254
        vali += [(user, c, v) for c, v in Counter(vali_data).items()]                     # :255-256
    return {"num_users": len(indptr), "num_items": len(name_lines), "num_events": tokens,
            "indptr": np.array(indptr, np.int64), "items": np.array(events, np.int32), "records": triples(records), "vali": triples(vali),
            "item_counts": np.bincount(np.array(events, np.int64), minlength=len(name_lines)).astype(np.int64)}


def triples(recs):
    return (np.array([r for r, _, _ in recs], np.int32), np.array([c for _, c, _ in recs], np.int32), np.array([v for _, _, v in recs], np.float32))


def group(records, num_major, sort_key, cut=None):
    """The first `cut` records stable-sorted by (major, minor) and compressed: fileio.hpp:263-420 in numpy."""
    rows, cols, vals = (a[:cut] for a in records)
    major, minor = (rows, cols) if sort_key == 1 else (cols, rows)
    order = np.lexsort((minor, major))                                                    # stable
    return {"indptr": np.cumsum(np.bincount(major, minlength=num_major)).astype(np.int64), "key": minor[order], "val": vals[order]}


def vali_values_reordered(rows, cols, vals):
    """base.py:249-253: the values pass through csr_matrix((val, (row, col))).data, which lists them by (row, col)."""
    return vals[np.lexsort((cols, rows))]


def assert_same(res, want, num_items, cut=None):
    """Every output of a StreamResult against the restatement, exactly."""
    c = res.counts
    assert (c["num_users"], c["num_train"], c["num_records"], c["num_vali"]) == (want["num_users"], len(want["items"]), len(want["records"][0]),
                                                                                 len(want["vali"][0])), c
    assert c["num_events"] == want["num_events"]
    indptr, items = res.events()
    assert indptr.dtype == np.int64 and items.dtype == np.int32
    assert np.array_equal(indptr, want["indptr"]) and np.array_equal(items, want["items"])
    for got, exp, what in ((res.records(), want["records"], "records"), (res.vali(), want["vali"], "vali")):
        for g, e, part in zip(got, exp, ("rows", "cols", "vals")):
            assert g.dtype == e.dtype and np.array_equal(g, e), (what, part, g[:8], e[:8])
    assert np.array_equal(res.item_counts(), want["item_counts"])
    n = c["num_records"] if cut is None else cut
    for sort_key, num_major in ((1, want["num_users"]), (2, num_items)):
        got, exp = res.group(sort_key, -1 if cut is None else cut), group(want["records"], num_major, sort_key, n)
        for k in ("indptr", "key", "val"):
            assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), ("group", sort_key, k)


# ------------------------------------------------------------------------------------------------
# case generators
# ------------------------------------------------------------------------------------------------
# every non-empty prefix of a name is a name: a text cut anywhere still holds only names
PREFIX_NAMES = [a + b + c for a in "ab" for b in ("", "a", "b") for c in (("", "a", "b") if b else ("",))]
SEPARATORS = [" ", " ", " ", "\t", "  ", "\n", "\n", "\r\n", "\r", " \v", "\f ", "\x1c", "\x1d\x1e", "\x1f ", "\n\n"]


def names_file(names):
    return "".join(n + "\n" for n in names).encode("utf-8")


def text_of_size(size, seed):
    """Exactly `size` bytes of PREFIX_NAMES tokens between mixed separators and line ends."""
    rng = np.random.default_rng(seed)
    parts, length = [], 0
    while length < size:
        piece = PREFIX_NAMES[rng.integers(len(PREFIX_NAMES))] + SEPARATORS[rng.integers(len(SEPARATORS))]
        parts.append(piece)
        length += len(piece)
    return "".join(parts).encode()[:size]


def boundary_cases():
    """name -> (names bytes, text bytes)"""
    pre = names_file(PREFIX_NAMES)
    out = {"size_%d" % n: (pre, text_of_size(n, n)) for n in (0, 1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5)}
    long20, long9000 = "straddles-two-tiles!", "x" * 8999 + "y"
    out["token_over_a_tile_border"] = (names_file(PREFIX_NAMES + [long20]), text_of_size(4086, 1) + b"\n a " + long20.encode() + b" b\nab " + long20.encode())
    assert out["token_over_a_tile_border"][1].index(long20.encode()) in range(4077, 4096)
    out["token_of_9000_bytes"] = (names_file(PREFIX_NAMES + [long9000]), b"a b\nab " + long9000.encode() + b" a\n" + long9000.encode() + b"\nb")
    out["last_line_open"] = (pre, b"a b\nab")
    out["last_line_closed"] = (pre, b"a b\nab\n")
    out["crlf_and_lone_cr"] = (pre, b"a b\r\nab\rb a\r\r\nab\r")
    out["mixed_white_space"] = (pre, b"a\v\fb \x1c\x1d ab\x1e\x1fba\t\t a\n  \t\n\x1f b \x1c\n")
    out["empty_lines_around"] = (pre, b"\n\na b\n\n\r\n\nab a ab\n\n")
    out["only_empty_lines"] = (pre, b"\n\r\n\r \n")
    out["one_event_users"] = (pre, b"a\nab b\nb\n\nab ab ab\n")
    return out


def mixed_names(n):
    """Names of equal length that differ only in the last byte, names that are prefixes of other names, UTF-8 names."""
    kinds = (lambda s: s + "a", lambda s: s + "b", lambda s: s + "ab", lambda s: "é" + s + "ü中")
    return [kinds[i % 4]("k%03d" % (i // 4)) for i in range(n)]


def random_stream(names, num_users, max_len, seed, total=None):
    """One line per user, 0..max_len names each (or `total` events spread over the users); returns bytes."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, num_users) if total is None else np.bincount(rng.integers(0, num_users, total), minlength=num_users)
    ids = rng.integers(0, len(names), int(lens.sum()))
    lines, at = [], 0
    for n in lens:
        lines.append(" ".join(names[i] for i in ids[at:at + n]))
        at += n
    return ("\n".join(lines) + "\n").encode("utf-8")
