"""MatrixMarket databases restated in numpy (TEST INFRASTRUCTURE, not collected) + the case generators of test_mm_ref_cpu.py and
test_mm_gpu.py.  `restate` is written from /root/reference/buffalo/data/mm.py:110-279, data/base.py:210-253, 399-451 and data/prepro.py;
tests/test_mm_ref_cpu.py pins it to the databases the reference's own MatrixMarket.create() built."""
import io

import numpy as np

F32 = np.float32


def lines_of(data):
    """The lines of `data` as Python's text mode reads a file (universal newlines): "\\n", "\\r\\n" and a lone "\\r" end a line."""
    return list(io.TextIOWrapper(io.BytesIO(data), encoding="utf-8", newline=None))


def header(lines):
    """(num_users, num_items, num_nnz, num_header_lines with the size line): mm.py:154-159 and :248-251, which must agree."""
    n = 0
    while lines[n].strip().startswith("%"):
        if not lines[n].startswith("%"):
            raise ValueError("line %d: mm.py:156 and mm.py:250 disagree" % (n + 1))
        n += 1
    num_users, num_items, num_nnz = map(int, lines[n].split())
    return num_users, num_items, num_nnz, n + 1


def ulps(a, b):
    """Distance of two float32 arrays in units in the last place (finite values of one sign)."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------
# prepro.py with every float32 step spelled out
# ------------------------------------------------------------------------------------------------
class Prepro:
    """One object for the rowwise values, the held-out values and the colwise values, in this order (base.py:399-451)."""

    def __init__(self, name=None, **kw):
        self.name, self.kw = name, kw
        self.value_min, self.value_max = F32(np.inf), F32(0.0)                 # prepro.py:36-37

    def __call__(self, v):
        v = np.asarray(v, F32)
        if self.name == "OneBased":
            return np.ones_like(v)
        if self.name == "ImplicitALS":                                         # float32 quotient and sum, then the correctly rounded log
            s = (F32(1.0) + (v / F32(self.kw["epsilon"])).astype(F32)).astype(F32)
            return np.log(s.astype(np.float64)).astype(F32)
        if self.name == "MinMaxScalar" and len(v):
            self.value_min, self.value_max = min(self.value_min, v.min()), max(self.value_max, v.max())
        return v

    def post(self, v):
        if self.name != "MinMaxScalar":
            return v
        lo, hi = F32(self.kw["min"]), F32(self.kw["max"])
        width = F32(self.value_max - self.value_min)
        if width < F32(0.00000001):
            return np.full_like(v, hi)
        span = F32(float(self.kw["max"]) - float(self.kw["min"]))              # formed in double, rounded once
        a = (v - self.value_min).astype(F32)
        b = (a / width).astype(F32)
        m = (b * span).astype(F32)
        return (m + lo).astype(F32)

    def range(self):
        return np.array([self.value_min, self.value_max], F32)


def group(rows, cols, vals, num_major, sort_key):
    """Stable sort by (major, minor) and compression: fileio.hpp:263-420 in numpy."""
    major, minor = (rows, cols) if sort_key == 1 else (cols, rows)
    order = np.lexsort((minor, major))                                         # stable
    return {"indptr": np.cumsum(np.bincount(major, minlength=num_major)).astype(np.int64), "key": minor[order].astype(np.int32), "val": vals[order]}


def restate(text, sample_positions=None, prepro=None, vali_file_order=False, **kw):
    """text: bytes of the main file.  Returns the header, both groups, the held-out triples, the value ranges and the working text."""
    lines = lines_of(text)
    num_users, num_items, num_nnz, skip = header(lines)
    body = lines[skip:skip + num_nnz]                                          # only the first num_nnz body lines count
    if len(body) < num_nnz:
        raise ValueError("%d body lines, the header says %d" % (len(body), num_nnz))
    held = [] if sample_positions is None else [int(p) for p in sample_positions]
    if any(b <= a for a, b in zip(held, held[1:])) or any(not 0 <= p < num_nnz - 1 for p in held):
        raise ValueError("sample positions")
    fields = [ln.split() for ln in body]
    rows = np.array([int(f[0]) - 1 for f in fields], np.int32)
    cols = np.array([int(f[1]) - 1 for f in fields], np.int32)
    vals = np.array([F32(f[2]) for f in fields], F32)                          # strtof: the decimal string rounded once to float32
    keep = np.ones(num_nnz, bool)
    keep[held] = False
    pp = Prepro(prepro, **kw)
    out = {"header": {"num_users": num_users, "num_items": num_items, "num_nnz": num_nnz, "num_header_lines": skip,
                      "num_train": int(keep.sum()), "num_vali": len(held)},
           "working_text": "".join(ln.rstrip("\r\n") + "\n" for ln, k in zip(body, keep) if k).encode()}
    tr, tc, tv = rows[keep], cols[keep], vals[keep]
    out["rowwise"] = group(tr, tc, pp(tv), num_users, 1)
    out["rowwise"]["val"] = pp.post(out["rowwise"]["val"])
    ranges = [pp.range()]
    hr, hc, hv = rows[~keep], cols[~keep], vals[~keep]
    if len(hr):                                                                # base.py:240-253
        order = np.lexsort((hc, hr))
        if len(set(zip(hr.tolist(), hc.tolist()))) != len(hr):
            raise ValueError("a held-out pair is listed twice")
        hv = pp(hv if vali_file_order else hv[order])
    out["vali"] = (hr, hc, hv)
    out["colwise"] = group(tr, tc, pp(tv), num_items, 2)
    out["colwise"]["val"] = pp.post(out["colwise"]["val"])
    out["value_range"] = np.concatenate([ranges[0], pp.range()])
    return out


# ------------------------------------------------------------------------------------------------
# case generators
# ------------------------------------------------------------------------------------------------
PREPROS = {"none": (None, {}), "onebased": ("OneBased", {}), "minmax": ("MinMaxScalar", {"min": 1, "max": 5}), "ials": ("ImplicitALS", {"epsilon": 0.5})}
CONSTANT_TEXT = "%%MatrixMarket matrix coordinate integer general\n3 4 5\n1 1 2\n2 3 2\n3 4 2\n1 2 2\n2 2 2\n"


def as_crlf(text):
    return text.replace("\n", "\r\n")


def as_lone_cr(text):
    return text.replace("\n", "\r")


def without_final_newline(text):
    assert text.endswith("\n")
    return text[:-1]


def with_extra_comments(text):
    first, rest = text.split("\n", 1)
    return first + "\n%\n% a comment line\n%%\n" + rest


def tile_text(num_users=300, num_items=200, nnz=3000, seed=11):
    """A body of `nnz` lines with real values of mixed width (1 to 9 characters), so that lines straddle the 4,096-byte tile ends; every (row, col) once."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(num_users * num_items, nnz, replace=False)
    rows, cols = cells // num_items + 1, cells % num_items + 1
    digits = rng.integers(0, 8, nnz)
    vals = [repr(round(float(v), int(d))) if d else str(int(v) + 1) for v, d in zip(rng.random(nnz) * 9 + 0.001, digits)]
    head = "%%%%MatrixMarket matrix coordinate real general\n%% tile case\n%d %d %d\n" % (num_users, num_items, nnz)
    return head + "".join("%d %d %s\n" % t for t in zip(rows, cols, vals))


def tile_positions(text_bytes, tile=4096):
    """Held-out body lines of the tile case: 0 and 1, five in a row, around every tile boundary of the first few tiles (the line that ends exactly at a
    boundary and the one that starts there, where the text has such a line, else the line that straddles it and its successor), num_nnz - 2."""
    lines = lines_of(text_bytes)
    _, _, nnz, skip = header(lines)
    raw = text_bytes.decode()
    starts, at = [], 0
    for ln in lines_raw(raw):
        starts.append(at)
        at += len(ln)
    pos = {0, 1, nnz - 2} | set(range(100, 105))
    exact = 0
    for boundary in range(tile, len(raw), tile):
        k = max(i for i, s in enumerate(starts) if s <= boundary) - skip       # the body line that holds (or starts at) the boundary byte
        if 1 <= k < nnz - 2:
            exact += starts[k + skip] == boundary
            pos |= {k - 1, k}
    return np.array(sorted(p for p in pos if 0 <= p < nnz - 1), np.int64), exact


def lines_raw(raw):
    """Lines with their terminators kept as they are ("\\r\\n" stays two bytes)."""
    out, at = [], 0
    while at < len(raw):
        e = at
        while e < len(raw) and raw[e] not in "\r\n":
            e += 1
        e += 2 if raw[e:e + 2] == "\r\n" else (1 if e < len(raw) else 0)
        out.append(raw[at:e])
        at = e
    return out


def align_to_tile(text, tile=4096):
    """Pad the second comment line so that some body line starts exactly at a multiple of `tile` bytes."""
    first, rest = text.split("\n", 1)
    raw = lines_raw(text)
    at, skip = 0, header(lines_of(text.encode()))[3]
    starts = []
    for ln in raw:
        starts.append(at)
        at += len(ln)
    target = next(s for s in starts[skip + 10:] if s > tile)                   # a body line start behind the first boundary
    pad = (-target) % tile
    pad += tile if pad < 2 else 0                                              # a comment line is at least "%\n"
    return first + "\n" + "%" + "x" * (pad - 2) + "\n" + rest
