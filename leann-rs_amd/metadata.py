"""Metadata filters evaluated on the device (include/leann_backend.h "metadata filters evaluated on the device", csrc/meta.hip).

MetaColumns is a leann_meta: the passages' metadata fields as columns in HBM.  parse_filter is the twin of the reference's
MetadataFilter::parse (src/index/filter.rs:52-316); the ABI takes the parsed tree, so the mini-language stays up here.  A filter is
("cond", field, op, value) | ("and", [filters]) | ("or", [filters]) with op one of OPS and value None, a bool, a number, a str or a
list of those; every method that takes a filter also takes its text."""
import ctypes as C
import re

import numpy as np

from . import _native as N
from ._native import LeannError, u8p

OPS = ("eq", "ne", "gt", "gte", "lt", "lte", "in", "notin", "contains", "startswith", "endswith", "exists")
TAG_MISSING, TAG_NULL, TAG_FALSE, TAG_TRUE, TAG_NUMBER, TAG_STRING, TAG_OTHER = range(7)


# ---- MetadataFilter::parse ---------------------------------------------------------------------------------------------------
_INT = re.compile(r"[+-]?[0-9]+\Z")
_FLOAT = re.compile(r"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?\Z")
_COMPARISONS = (("!=", "ne"), (">=", "gte"), ("<=", "lte"), (">", "gt"), ("<", "lt"))  # in the order filter.rs looks for them


def _parse_value(s):  # parse_value, filter.rs:420-439: i64, then a finite f64, then a bool, else the string
    if _INT.match(s) and -(1 << 63) <= int(s) < (1 << 63):
        return int(s)
    if _FLOAT.match(s):
        f = float(s)
        if np.isfinite(f):
            return f
    return {"true": True, "false": False}.get(s, s)


def _split_top_level_commas(text):
    parts, cur, depth = [], [], 0
    for ch in text:
        depth += (ch == "[") - (ch == "]")
        if ch == "," and depth == 0:
            parts.append("".join(cur))
            cur = []
        else:
            cur.append(ch)
    if cur:
        parts.append("".join(cur))
    return parts


def _has_top_level_comma(text):
    depth = 0
    for ch in text:
        depth += (ch == "[") - (ch == "]")
        if ch == "," and depth == 0:
            return True
    return False


def _parse_single(text):
    text = text.strip()
    if text.endswith("?"):
        return ("cond", text[:-1], "exists", None)
    for marker, op in ((" in [", "in"), (" not_in [", "notin")):
        at = text.find(marker)
        if at >= 0:
            rest = text[at + len(marker):]
            end = rest.find("]")
            if end >= 0:
                return ("cond", text[:at].strip(), op, [_parse_value(v.strip()) for v in rest[:end].split(",")])
    for sep, op in (("~", "contains"), ("^", "startswith"), ("$", "endswith")):
        if sep in text and not (sep == "^" and ">=" in text):
            field, value = text.split(sep, 1)
            return ("cond", field, op, value)
    for sep, op in _COMPARISONS:
        if sep in text:
            field, value = text.split(sep, 1)
            return ("cond", field, op, _parse_value(value))
    sep = "=" if "=" in text else (":" if ":" in text else None)
    if sep is None:
        return None
    field, value = text.split(sep, 1)
    if "*" in value:  # glob forms
        if value.startswith("*") and value.endswith("*") and len(value.encode()) > 2:
            return ("cond", field, "contains", value[1:-1])
        if value.startswith("*"):
            return ("cond", field, "endswith", value[1:])
        if value.endswith("*"):
            return ("cond", field, "startswith", value[:-1])
    return ("cond", field, "eq", _parse_value(value))


def _group(kind, filters):
    filters = [f for f in filters if f is not None]
    if len(filters) > 1:
        return (kind, filters)
    return filters[0] if filters else None


def parse_filter(text):
    """MetadataFilter::parse: the filter tree of `text`, or None where the reference returns None"""
    text = text.strip()
    if " OR " in text:
        return _group("or", [parse_filter(p.strip()) for p in text.split(" OR ")])
    if " AND " in text:
        return _group("and", [_parse_single(p.strip()) for p in text.split(" AND ")])
    if _has_top_level_comma(text):
        return _group("and", [_parse_single(p.strip()) for p in _split_top_level_commas(text)])
    return _parse_single(text)


def filter_fields(flt):
    """the fields a filter names, in first-use order"""
    out = []
    stack = [flt]
    while stack:
        f = stack.pop(0)
        if f[0] == "cond":
            if f[1] not in out:
                out.append(f[1])
        else:
            stack = list(f[1]) + stack
    return out


# ---- the tree as the ABI takes it ---------------------------------------------------------------------------------------------
class MetaValue(C.Structure):
    pass


MetaValue._fields_ = [("type", C.c_int32), ("boolean", C.c_int32), ("num", C.c_double), ("str", C.c_char_p), ("len", C.c_size_t),
                      ("list", C.POINTER(MetaValue))]


class MetaNode(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_children", C.c_uint32), ("field", C.c_char_p), ("op", C.c_int32), ("value", MetaValue)]


def _as_filter(flt):
    if isinstance(flt, str):
        parsed = parse_filter(flt)
        if parsed is None:
            raise LeannError(1, f"metadata filter: cannot parse {flt!r}")
        return parsed
    return flt


def _fill_value(dst, v, keep, in_list=False):
    if v is None:
        dst.type = 0
    elif isinstance(v, bool):
        dst.type, dst.boolean = 1, int(v)
    elif isinstance(v, (int, float)):
        dst.type, dst.num = 2, float(v)
    elif isinstance(v, (str, bytes)):
        raw = v.encode() if isinstance(v, str) else v
        buf = C.create_string_buffer(raw, len(raw) + 1)
        keep.append(buf)
        dst.type, dst.str, dst.len = 3, C.cast(buf, C.c_char_p), len(raw)
    elif isinstance(v, (list, tuple)):
        dst.type, dst.len = 4, len(v)
        if not in_list and len(v):
            arr = (MetaValue * len(v))()
            keep.append(arr)
            for i, x in enumerate(v):
                _fill_value(arr[i], x, keep, True)
            dst.list = C.cast(arr, C.POINTER(MetaValue))
        elif in_list:
            dst.len = 0  # a nested list equals nothing
    else:
        raise LeannError(1, f"metadata filter: unsupported value {v!r}")


def _flatten(flt):
    flat = []

    def walk(f):
        if f[0] == "cond":
            if f[2] not in OPS:
                raise LeannError(1, f"metadata filter: unknown op {f[2]!r}")
            flat.append(f)
        else:
            flat.append(f)
            for c in f[1]:
                walk(c)
    walk(_as_filter(flt))
    return flat


def _fill_nodes(nodes, at, flat, keep):
    for i, f in enumerate(flat):
        nd = nodes[at + i]
        if f[0] == "cond":
            field = C.create_string_buffer(f[1].encode())
            keep.append(field)
            nd.kind, nd.field, nd.op = 0, C.cast(field, C.c_char_p), OPS.index(f[2])
            _fill_value(nd.value, f[3], keep)
        else:
            nd.kind, nd.n_children = {"and": 1, "or": 2}[f[0]], len(f[1])


def encode_tree(flt):
    """(MetaNode array in prefix order, node count, objects to keep alive while the array is in use)"""
    flat, keep = _flatten(flt), []
    nodes = (MetaNode * len(flat))()
    _fill_nodes(nodes, 0, flat, keep)
    return nodes, len(flat), keep


def encode_trees(filters):
    """a batch of filters as the ABI takes it: (one MetaNode array, node_off as a size_t array [len(filters) + 1], number of filters,
    objects to keep alive while the arrays are in use)"""
    flats, keep = [_flatten(f) for f in filters], []
    off = (C.c_size_t * (len(flats) + 1))()
    for i, flat in enumerate(flats):
        off[i + 1] = off[i] + len(flat)
    nodes = (MetaNode * max(off[len(flats)], 1))()
    for i, flat in enumerate(flats):
        _fill_nodes(nodes, off[i], flat, keep)
    return nodes, off, len(flats), keep


# ---- leann_meta ----------------------------------------------------------------------------------------------------------------
_MISSING = object()


def _nested(record, path):  # get_nested_value, filter.rs:376-388
    cur = record
    for part in path.split("."):
        if not isinstance(cur, dict) or part not in cur:
            return _MISSING
        cur = cur[part]
    return cur


def column_arrays(records, field):
    """tag u8 [n], num f64 [n], str_blob bytes, str_off u64 [n + 1] of one field over json-decoded records (None: unreadable)"""
    n = len(records)
    tag = np.zeros(n, np.uint8)
    num = np.zeros(n, np.float64)
    off = np.zeros(n + 1, np.uint64)
    blob = bytearray()
    for i, r in enumerate(records):
        v = _nested(r, field) if r is not None else _MISSING
        if v is _MISSING:
            t = TAG_MISSING
        elif v is None:
            t = TAG_NULL
        elif isinstance(v, bool):
            t = TAG_TRUE if v else TAG_FALSE
        elif isinstance(v, (int, float)):
            t, num[i] = TAG_NUMBER, float(v)
        elif isinstance(v, str):
            t = TAG_STRING
            blob += v.encode()
        else:
            t = TAG_OTHER
        tag[i] = t
        off[i + 1] = len(blob)
    return tag, num, bytes(blob), off


class MetaColumns:
    """a leann_meta: one column per metadata field, on `device`"""

    def __init__(self, n, valid=None, device=0):
        h = C.c_void_p()
        if valid is not None:
            valid = np.ascontiguousarray(valid, np.uint8)
            if valid.ndim != 1 or valid.shape[0] < (n + 7) // 8:
                raise LeannError(1, "valid bitmap shape does not match n")
        N.check(N.lib().leann_meta_create(n, valid.ctypes.data_as(u8p) if valid is not None else None, device, C.byref(h)))
        self._h = h
        self.device = device

    @classmethod
    def from_records(cls, records, fields, device=0):
        """records: a list of dicts (a passage's metadata); None marks a passage whose metadata could not be read"""
        n = len(records)
        valid = None
        if any(r is None for r in records):
            valid = np.packbits(np.array([r is not None for r in records], bool), bitorder="little")
        m = cls(n, valid, device)
        for f in fields:
            m.add_records_column(f, records)
        return m

    def add_records_column(self, field, records):
        tag, num, blob, off = column_arrays(records, field)
        self.add_column(field, tag, num, blob, off)

    def add_column(self, field, tag, num=None, str_blob=None, str_off=None):
        tag = np.ascontiguousarray(tag, np.uint8)
        num = None if num is None else np.ascontiguousarray(num, np.float64)
        str_off = None if str_off is None else np.ascontiguousarray(str_off, np.uint64)
        n = self.len()
        if tag.shape != (n,) or (num is not None and num.shape != (n,)) or (str_off is not None and str_off.shape != (n + 1,)):
            raise LeannError(1, "column arrays do not match the store's length")
        if str_off is not None and n and int(str_off.max()) > len(str_blob or b""):
            raise LeannError(1, "str_off points behind str_blob")
        N.check(N.lib().leann_meta_add_column(
            self._h, field.encode(), tag.ctypes.data_as(u8p),
            num.ctypes.data_as(C.POINTER(C.c_double)) if num is not None else None, str_blob,
            str_off.ctypes.data_as(N.u64p) if str_off is not None else None))

    def len(self):
        return int(N.lib().leann_meta_len(self._h))

    def has_column(self, field):
        return bool(N.lib().leann_meta_has_column(self._h, field.encode()))

    def eval(self, flt, with_count=False):
        """the allow-bitmap of the filter, np.uint8 [ceil(n / 8)] (and the number of allowed rows)"""
        nodes, k, keep = encode_tree(flt)
        out = np.zeros(max((self.len() + 7) // 8, 1), np.uint8)
        cnt = C.c_size_t(0)
        N.check(N.lib().leann_meta_eval(self._h, nodes, k, out.ctypes.data_as(u8p), C.byref(cnt)))
        del keep
        out = out[: (self.len() + 7) // 8]
        return (out, int(cnt.value)) if with_count else out

    def eval_device(self, flt, d_bitmap, d_and=None, d_n_allowed=None, stream=None):
        """enqueue the evaluation into device memory (pointers as ints) on `stream`; returns without waiting"""
        nodes, k, keep = encode_tree(flt)
        N.check(N.lib().leann_meta_eval_device(self._h, nodes, k, d_and, d_bitmap, d_n_allowed, stream))
        del keep

    def eval_batch(self, filters, with_count=False):
        """the allow-bitmaps of a batch of filters in one pass over the columns: np.uint8 [len(filters), ceil(n / 8)], row i what
        eval(filters[i]) returns (and the numbers of allowed rows, np.int64 [len(filters)])"""
        nodes, off, k, keep = encode_trees(filters)
        nbytes = (self.len() + 7) // 8
        out = np.zeros((k, max(nbytes, 1)), np.uint8)
        cnt = (C.c_size_t * max(k, 1))()
        N.check(N.lib().leann_meta_eval_batch(self._h, nodes, off, k, out.ctypes.data_as(u8p), out.shape[1], cnt, None))
        del keep
        out = out[:, :nbytes]
        return (out, np.array(cnt[:k], np.int64)) if with_count else out

    def eval_batch_device(self, filters, d_bitmaps, stride, d_and=None, d_n_allowed=None, stream=None):
        """enqueue the batch into device memory (pointers as ints) on `stream`: bitmap i at d_bitmaps + i * stride, d_n_allowed u32
        [len(filters)]; returns without waiting, with the number of distinct programs that run"""
        nodes, off, k, keep = encode_trees(filters)
        distinct = C.c_size_t(0)
        N.check(N.lib().leann_meta_eval_batch_device(self._h, nodes, off, k, d_and, d_bitmaps, stride, d_n_allowed, C.byref(distinct),
                                                     stream))
        del keep
        return int(distinct.value)

    def close(self):
        if self._h:
            N.lib().leann_meta_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
