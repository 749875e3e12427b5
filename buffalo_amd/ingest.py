"""COO -> compressed rows on the GPU (`bfh_coo_to_csr`): the device-side replacement of the sort + binarization
step of buffalo's data creation (/root/reference/buffalo/data/fileio.hpp:263-420, called per orientation from
data/base.py:399-451), and the SPPMI matrix of a stream (`bfh_sppmi_*`: stream.py:257-267 + fileio.hpp:109-254 +
stream.py:169-195), and the Stream database itself (`bfh_stream_*`: stream.py:81-158, 197-271 + w2v.py:91-100), and the MatrixMarket database
(`bfh_mm_*`: mm.py:110-279 + base.py:210-253, 399-451 + prepro.py).  No CPU fallback."""
import ctypes as C
import os

import numpy as np

from ._lib import BuffaloHipError, Stats, lib
from .backend import _Base, _ptr


def coo_to_csr(major, minor, vals, num_major, num_minor, with_stats=False):
    """Stable sort by (major, minor), duplicates kept.  Returns {"indptr": int64 END offsets [num_major],
    "key": int32 [nnz], "val": float32 [nnz]} -- the layout of an HDF5 group of the reference
    (`rowwise` / `colwise`: indptr, key, val)."""
    major = np.ascontiguousarray(major, dtype=np.int32)
    minor = np.ascontiguousarray(minor, dtype=np.int32)
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    if not (major.shape == minor.shape == vals.shape and major.ndim == 1):
        raise ValueError("major, minor and vals must be 1-d arrays of one length")
    nnz = major.shape[0]
    indptr = np.empty(int(num_major), dtype=np.int64)
    key = np.empty(nnz, dtype=np.int32)
    val = np.empty(nnz, dtype=np.float32)
    st = Stats()
    L = lib()
    rc = L.bfh_coo_to_csr(major.ctypes.data_as(C.POINTER(C.c_int32)), minor.ctypes.data_as(C.POINTER(C.c_int32)),
                          vals.ctypes.data_as(C.POINTER(C.c_float)), nnz, int(num_major), int(num_minor),
                          indptr.ctypes.data_as(C.POINTER(C.c_int64)), key.ctypes.data_as(C.POINTER(C.c_int32)),
                          val.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st))
    if rc < 0:
        raise BuffaloHipError((L.bfh_last_error(None) or b"bfh_coo_to_csr failed").decode())
    g = {"indptr": indptr, "key": key, "val": val}
    return (g, st.as_dict()) if with_stats else g


def _text_bytes(text):
    if isinstance(text, (bytes, bytearray, memoryview)):
        return bytes(text) if not isinstance(text, bytes) else text
    if isinstance(text, np.ndarray) and text.dtype == np.uint8:
        return text.tobytes()
    raise TypeError("text must be bytes (the working file's content) or a uint8 array")


def parse_triples(text, total_lines, with_stats=False):
    """The first `total_lines` lines of buffalo's working text file ("row col val", 1-based ids: data/mm.py:175-234) as the reference's
    sscanf(line, "%d %d %f") reads them (fileio.hpp:300-303), parsed on the device (`bfh_parse_triples`).  Returns (rows, cols, vals) with the
    ids still 1-based; stats["merges"] = lines the device handed back to sscanf."""
    buf = _text_bytes(text)
    n = int(total_lines)
    rows, cols, vals = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
    st = Stats()
    L = lib()
    rc = L.bfh_parse_triples(buf, len(buf), n, rows.ctypes.data_as(C.POINTER(C.c_int32)), cols.ctypes.data_as(C.POINTER(C.c_int32)),
                             vals.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st))
    if rc < 0:
        raise BuffaloHipError((L.bfh_last_error(None) or b"bfh_parse_triples failed").decode())
    return ((rows, cols, vals), st.as_dict()) if with_stats else (rows, cols, vals)


def text_to_csr(text, total_lines, num_major, num_minor, sort_key, with_stats=False):
    """Working text file -> the `rowwise` (sort_key 1) / `colwise` (sort_key 2) group, everything between the bytes and the group on the device
    (`bfh_text_to_csr` = fileio.hpp:263-420: parse, stable sort by (major, minor), END offsets, 0-based minors)."""
    buf = _text_bytes(text)
    n = int(total_lines)
    indptr = np.empty(int(num_major), dtype=np.int64)
    key, val = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float32)
    st = Stats()
    L = lib()
    rc = L.bfh_text_to_csr(buf, len(buf), n, int(num_major), int(num_minor), int(sort_key), indptr.ctypes.data_as(C.POINTER(C.c_int64)),
                           key.ctypes.data_as(C.POINTER(C.c_int32)), val.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st))
    if rc < 0:
        raise BuffaloHipError((L.bfh_last_error(None) or b"bfh_text_to_csr failed").decode())
    g = {"indptr": indptr, "key": key, "val": val}
    return (g, st.as_dict()) if with_stats else g


class _Sppmi(_Base):
    _PFX = "bfh_sppmi_"


def build_sppmi(indptr, items, num_items, windows, k, with_stats=False):
    """SPPMI group of a stream: `indptr` = END offsets [num_users] over the 0-based `items` of the users' sequences,
    `windows` / `k` = the reference's data.sppmi options (stream.py:34-36).  Returns {"indptr": int64 END offsets
    [num_items], "key": int32 [nnz], "val": float32 [nnz], "total_lines": D} -- the layout of the reference's `sppmi`
    HDF5 group (stream.py:183-188), which CFR reads as its context matrix.  Like the reference's builder, pairs with the
    largest id that occurs are left out (fileio.hpp:182-250 never flushes the group at end of file); rows hold their
    entries in column order (the reference: std::unordered_set iteration order -- same entries per row)."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    items = np.ascontiguousarray(items, dtype=np.int32)
    if indptr.ndim != 1 or items.ndim != 1 or indptr.shape[0] == 0 or int(indptr[-1]) != items.shape[0]:
        raise ValueError("indptr must be 1-d END offsets whose last entry is len(items)")
    h = _Sppmi()
    try:
        nnz, lines = C.c_int64(0), C.c_int64(0)
        h._call("build", _ptr(indptr, C.c_int64), _ptr(items, C.c_int32), indptr.shape[0], int(num_items), int(windows), int(k), C.byref(nnz),
                C.byref(lines))
        out_indptr = np.empty(int(num_items), dtype=np.int64)
        key = np.empty(nnz.value, dtype=np.int32)
        val = np.empty(nnz.value, dtype=np.float32)
        h._call("fetch", _ptr(out_indptr, C.c_int64), _ptr(key, C.c_int32), _ptr(val, C.c_float))
        st = h.stats()
    finally:
        h.close()
    g = {"indptr": out_indptr, "key": key, "val": val, "total_lines": lines.value}
    return (g, st) if with_stats else g


# bytes.split() knows \t \n \v \f \r and the space; str.split() also \x1c-\x1f
_STR_SPLIT = bytes(32 if 28 <= b <= 31 else b for b in range(256))


class _Result:
    """What one `build` of a builder left on the device; the next `build` of the same builder replaces the device arrays: fetch first."""
    _OWNER = None

    def __init__(self, builder, serial):
        self._b, self._serial = builder, serial

    def _call(self, name, *args):
        if self._b._serial != self._serial:
            raise BuffaloHipError("this result was replaced by a later build of its %s" % self._OWNER)
        return self._b._call(name, *args)

    def _triples(self, name, n):
        rows, cols, vals = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
        self._call(name, _ptr(rows, C.c_int32), _ptr(cols, C.c_int32), _ptr(vals, C.c_float))
        return rows, cols, vals


class StreamResult(_Result):
    """What one `StreamBuilder.build` left on the device; every method copies one output to the host.

    counts: {"num_users", "num_events", "num_train", "num_records", "num_vali"}; stats: the handle's `bfh_stats` right after the build
    (samples = tokens, accepted = train events, merges = records, loaded_rows = extra table probes, kernel_ms = token boundaries + lookup,
    aux_ms = the rest).  The next `build` of the same builder replaces the device arrays: fetch first."""
    _OWNER = "StreamBuilder"

    def __init__(self, builder, serial, counts, stats):
        super().__init__(builder, serial)
        self.counts, self.stats = counts, stats

    def events(self):
        """(indptr int64 END offsets [num_users], items int32 [num_train]): the train events in order -- the `rowwise` group of
        internal_data_type "stream" (stream.py:160-164) and the input of `build_sppmi` / `bfh_w2v_add_jobs`."""
        indptr, items = np.empty(self.counts["num_users"], np.int64), np.empty(self.counts["num_train"], np.int32)
        self._call("fetch_events", _ptr(indptr, C.c_int64), _ptr(items, C.c_int32))
        return indptr, items

    def records(self):
        """(rows, cols, vals), 0-based: the working file of internal_data_type "matrix" (stream.py:253-254)."""
        return self._triples("fetch_records", self.counts["num_records"])

    def vali(self):
        """(rows, cols, vals) of the held-out events in the order met; base.py:241-253 reorders the values afterwards."""
        return self._triples("fetch_vali", self.counts["num_vali"])

    def group(self, sort_key, max_records=-1):
        """The first `max_records` records (all when negative) as the `rowwise` (sort_key 1) / `colwise` (2) group: {"indptr", "key", "val"}."""
        n = self.counts["num_records"] if max_records < 0 else min(int(max_records), self.counts["num_records"])
        num_major = self.counts["num_users"] if int(sort_key) == 1 else self._b.num_items
        indptr, key, val = np.empty(num_major, np.int64), np.empty(n, np.int32), np.empty(n, np.float32)
        self._call("fetch_group", int(sort_key), int(max_records), _ptr(indptr, C.c_int64), _ptr(key, C.c_int32), _ptr(val, C.c_float))
        return {"indptr": indptr, "key": key, "val": val}

    def item_counts(self):
        """int64 [num_items]: occurrences of every item among the train events (`uni` of W2V.build_vocab, w2v.py:91-100)."""
        counts = np.empty(self._b.num_items, np.int64)
        self._call("fetch_counts", _ptr(counts, C.c_int64))
        return counts


def _sample_positions(sample_positions):
    """(pointer, count) of the `sample` split's positions; an empty draw is still the `sample` method: the pointer must not be NULL."""
    if sample_positions is None:
        return None, 0, None
    arr = np.ascontiguousarray(sample_positions, dtype=np.int64)
    if arr.ndim != 1:
        raise ValueError("sample_positions must be 1-d")
    keep = arr if arr.size else np.zeros(1, np.int64)
    return _ptr(keep, C.c_int64), int(arr.size), keep


class StreamBuilder(_Base):
    """Stream text -> database arrays on the device (`bfh_stream_*`).  `stats()` = the handle's `bfh_stats` now (summed over set_vocabulary,
    builds and fetches since the last reset).

    names: the item-id file's bytes (one name per line, item i = line i stripped), or a list of str, or None.  With None the vocabulary is taken
    from the first text built: `sorted(set(text.split()))` (str.split's white space), computed ON THE HOST (the reference numbers the items in set order, which is
    arbitrary; discovering the vocabulary on the device is not done)."""
    _PFX = "bfh_stream_"

    def __init__(self, names=None, device=None):
        super().__init__()
        self._serial, self.num_items, self.names = 0, None, None
        if device is not None:
            self.set_device(device)
        if names is not None:
            self.set_vocabulary(names)

    def set_vocabulary(self, names):
        """Replace the vocabulary (bytes of the id file, or a list of str); results built before are dropped."""
        given = None
        if not isinstance(names, (bytes, bytearray, memoryview, np.ndarray)):
            given = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in names]
            names = b"".join(n + b"\n" for n in given)
        buf = _text_bytes(names)
        n = C.c_int(0)
        self._serial += 1
        self._call("set_vocabulary", buf, len(buf), C.byref(n))
        if given is not None and n.value != len(given):
            raise ValueError("the names hold line ends: %d names became %d lines" % (len(given), n.value))
        self.num_items, self.names = n.value, buf

    def build(self, text, vali_n=0, sample_positions=None):
        """`vali_n` > 0: the `newest` split; `sample_positions`: ascending global event indices of the `sample` split (drawn by the caller as
        base.py:220-226 draws them, then sorted).  Returns a StreamResult."""
        buf = _text_bytes(text)
        if self.num_items is None:
            self.set_vocabulary(sorted(set(buf.translate(_STR_SPLIT).split())))
        pos, n_pos, _keep = _sample_positions(sample_positions)
        out = (C.c_int64 * 5)()
        self._serial += 1
        self._call("build", buf, len(buf), int(vali_n), pos, n_pos, out)
        counts = dict(zip(("num_users", "num_events", "num_train", "num_records", "num_vali"), (int(v) for v in out)))
        return StreamResult(self, self._serial, counts, self.stats())


class MatrixMarketResult(_Result):
    """What one `MatrixMarketBuilder.build` left on the device; every method copies one output to the host.

    header: {"num_users", "num_items", "num_nnz" (the size line's), "num_header_lines" (the size line included), "num_train", "num_vali"};
    stats: the handle's `bfh_stats` right after the build (samples = body lines, accepted = train entries, merges = lines the host parsed,
    kernel_ms = line ends + parse, aux_ms = the rest).  The next `build` of the same builder replaces the device arrays: fetch first."""
    _OWNER = "MatrixMarketBuilder"

    def __init__(self, builder, serial, header, stats):
        super().__init__(builder, serial)
        self.header, self.stats = header, stats

    def group(self, sort_key):
        """The train entries as the `rowwise` (sort_key 1) / `colwise` (2) group of the reference's database: {"indptr", "key", "val"}, values
        transformed by the builder's value_prepro (base.py:399-451)."""
        n = self.header["num_train"]
        num_major = self.header["num_users"] if int(sort_key) == 1 else self.header["num_items"]
        indptr, key, val = np.empty(num_major, np.int64), np.empty(n, np.int32), np.empty(n, np.float32)
        self._call("fetch_group", int(sort_key), _ptr(indptr, C.c_int64), _ptr(key, C.c_int32), _ptr(val, C.c_float))
        return {"indptr": indptr, "key": key, "val": val}

    def vali(self):
        """(rows, cols, vals) of the held-out lines: rows / cols 0-based in file order, vals as the reference stores them -- in (row, col) order
        (base.py:249-253), transformed; with mode "vali_file_order" = 1 value k belongs to triple k."""
        return self._triples("fetch_vali", self.header["num_vali"])

    def value_range(self):
        """float32 [4]: MinMaxScalar's (value_min, value_max) when the rowwise group was scaled and when the colwise group was (prepro.py:42-45)."""
        out = np.empty(4, np.float32)
        self._call("fetch_value_range", _ptr(out, C.c_float))
        return out


class MatrixMarketBuilder(_Base):
    """MatrixMarket text file -> database arrays on the device (`bfh_mm_*`).  The `idmap` names (uid / iid files) stay with the caller.
    `stats()` = the handle's `bfh_stats` now (summed over builds and fetches since the last reset)."""
    _PFX = "bfh_mm_"
    _PREPRO_ARGS = {None: (), "OneBased": (), "MinMaxScalar": ("min", "max"), "ImplicitALS": ("epsilon",)}

    def __init__(self, device=None):
        super().__init__()
        self._serial = 0
        if device is not None:
            self.set_device(device)

    def set_value_prepro(self, name, **kw):
        """data.value_prepro of the reference's options: None, "OneBased", "MinMaxScalar" (min=, max=) or "ImplicitALS" (epsilon=); stays until
        it is changed.  Names the library does not know are passed on and refused there."""
        name = name or None
        want = self._PREPRO_ARGS.get(name, tuple(kw))
        if sorted(kw) != sorted(want):
            raise TypeError("value_prepro %s takes %s" % (name, ", ".join(want) or "no arguments"))
        a, b = ([float(kw[k]) for k in want] + [0.0, 0.0])[:2]
        self._call("set_value_prepro", name.encode() if name else None, a, b)

    def build(self, text, sample_positions=None):
        """`text`: the main file's bytes, or its path; `sample_positions`: strictly ascending body-line indices of the `sample` split (drawn by the
        caller as base.py:220-226 draws them, then sorted).  Returns a MatrixMarketResult."""
        if isinstance(text, (str, os.PathLike)):
            with open(text, "rb") as f:
                text = f.read()
        buf = _text_bytes(text)
        pos, n_pos, _keep = _sample_positions(sample_positions)
        out = (C.c_int64 * 6)()
        self._serial += 1
        self._call("build", buf, len(buf), pos, n_pos, out)
        header = dict(zip(("num_users", "num_items", "num_nnz", "num_header_lines", "num_train", "num_vali"), (int(v) for v in out)))
        return MatrixMarketResult(self, self._serial, header, self.stats())
