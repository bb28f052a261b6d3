"""A literal restatement of the reference's src/index/filter.rs over json-decoded Python values: parse (:52-316), matches (:319-373),
get_nested_value (:376-388), values_equal (:390-400), compare_values (:402-418), parse_value (:420-439).  The expected side of the
metadata-filter tests; nothing here knows about columns, dictionaries or the device.

A filter is ("cond", field, op, value) | ("and", [filters]) | ("or", [filters]); op is the reference's lowercase name.  A value is
None, bool, int, float, str or a list of those.  repr() of a tree tells 1, 1.0 and True apart, == does not."""
import re
import sys

OPS = ("eq", "ne", "gt", "gte", "lt", "lte", "in", "notin", "contains", "startswith", "endswith", "exists")
EPS = sys.float_info.epsilon  # f64::EPSILON

_I64 = re.compile(r"^[+-]?[0-9]+$")
_F64 = re.compile(r"^[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?$")


def parse_value(s):
    if _I64.match(s) and -2 ** 63 <= int(s) < 2 ** 63:
        return int(s)
    if _F64.match(s):  # (Rust also parses "inf" / "nan"; serde_json::Number::from_f64 refuses them: they stay strings)
        f = float(s)
        if f == f and abs(f) != float("inf"):
            return f
    if s == "true":
        return True
    if s == "false":
        return False
    return s


def _cond(field, op, value):
    return ("cond", field, op, value)


def parse(text):
    text = text.strip()
    if " OR " in text:
        fs = [f for f in (parse(p.strip()) for p in text.split(" OR ")) if f is not None]
        return ("or", fs) if len(fs) > 1 else (fs[0] if fs else None)
    has_and = " AND " in text
    depth, comma = 0, False
    for c in text:
        if c == "[":
            depth += 1
        elif c == "]":
            depth -= 1
        elif c == "," and depth == 0:
            comma = True
            break
    if has_and or comma:
        if has_and:
            parts = text.split(" AND ")
        else:
            parts, cur, depth = [], "", 0
            for c in text:
                if c == "[":
                    depth += 1
                    cur += c
                elif c == "]":
                    depth -= 1
                    cur += c
                elif c == "," and depth == 0:
                    parts.append(cur)
                    cur = ""
                else:
                    cur += c
            if cur:
                parts.append(cur)
        fs = [f for f in (parse_single(p.strip()) for p in parts) if f is not None]
        return ("and", fs) if len(fs) > 1 else (fs[0] if fs else None)
    return parse_single(text)


def parse_single(text):
    text = text.strip()
    if text.endswith("?"):
        return _cond(text[:-1], "exists", None)
    for marker, op in ((" in [", "in"), (" not_in [", "notin")):
        idx = text.find(marker)
        if idx >= 0:
            rest = text[idx + len(marker):]
            end = rest.find("]")
            if end >= 0:
                return _cond(text[:idx].strip(), op, [parse_value(v.strip()) for v in rest[:end].split(",")])
    if "~" in text:
        a, b = text.split("~", 1)
        return _cond(a, "contains", b)
    if "^" in text and ">=" not in text:
        a, b = text.split("^", 1)
        return _cond(a, "startswith", b)
    if "$" in text:
        a, b = text.split("$", 1)
        return _cond(a, "endswith", b)
    for sep, op in (("!=", "ne"), (">=", "gte"), ("<=", "lte"), (">", "gt"), ("<", "lt")):
        if sep in text:
            a, b = text.split(sep, 1)
            return _cond(a, op, parse_value(b))
    if "=" in text:
        field, value = text.split("=", 1)
    elif ":" in text:
        field, value = text.split(":", 1)
    else:
        return None
    if "*" in value:
        if value.startswith("*") and value.endswith("*") and len(value.encode()) > 2:
            return _cond(field, "contains", value[1:-1])
        if value.startswith("*"):
            return _cond(field, "endswith", value[1:])
        if value.endswith("*"):
            return _cond(field, "startswith", value[:-1])
    return _cond(field, "eq", parse_value(value))


_MISSING = object()


def get_nested_value(metadata, path):
    cur = metadata
    for part in path.split("."):
        if not isinstance(cur, dict) or part not in cur:  # Value::get(&str) answers only for an object
            return _MISSING
        cur = cur[part]
    return cur


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _is_string(v):  # (bytes: a string given as its raw bytes — the ABI takes any bytes, JSON only valid UTF-8)
    return isinstance(v, (str, bytes))


def _b(v):
    return v.encode() if isinstance(v, str) else v


def values_equal(a, b):
    if _is_string(a) and _is_string(b):
        return _b(a) == _b(b)
    if _is_number(a) and _is_number(b):
        return abs(float(a) - float(b)) < EPS
    if isinstance(a, bool) and isinstance(b, bool):
        return a == b
    return a is None and b is None


def compare_values(a, b):
    if _is_number(a) and _is_number(b):
        n1, n2 = float(a), float(b)
        return -1 if n1 < n2 else (1 if n1 > n2 else 0)
    if _is_string(a) and _is_string(b):
        x, y = _b(a), _b(b)  # str::cmp is bytewise
        return -1 if x < y else (1 if x > y else 0)
    return 0


def cond_matches(field, op, value, metadata):
    v = get_nested_value(metadata, field)
    some = v is not _MISSING
    if op == "exists":
        return some
    if op == "eq":
        return some and values_equal(v, value)
    if op == "ne":
        return not some or not values_equal(v, value)
    if op == "gt":
        return some and compare_values(v, value) > 0
    if op == "gte":
        return some and compare_values(v, value) >= 0
    if op == "lt":
        return some and compare_values(v, value) < 0
    if op == "lte":
        return some and compare_values(v, value) <= 0
    if op == "in":
        return isinstance(value, list) and some and any(values_equal(v, x) for x in value)
    if op == "notin":
        return not isinstance(value, list) or not some or not any(values_equal(v, x) for x in value)
    pattern = _b(value) if _is_string(value) else b""
    if not some or not _is_string(v):
        return False
    v = _b(v)
    if op == "contains":
        return pattern in v
    if op == "startswith":
        return v.startswith(pattern)
    if op == "endswith":
        return v.endswith(pattern)
    raise ValueError(op)


def matches(flt, metadata):
    if flt[0] == "cond":
        return cond_matches(flt[1], flt[2], flt[3], metadata)
    if flt[0] == "and":
        return all(matches(f, metadata) for f in flt[1])
    return any(matches(f, metadata) for f in flt[1])


def bitmap(flt, records, valid=None):
    """the allow-bitmap of `flt` over `records` (np.uint8 [ceil(n / 8)], pad bits zero); records[i] is None = unreadable metadata"""
    import numpy as np
    bits = np.zeros(len(records), bool)
    for i, r in enumerate(records):
        bits[i] = r is not None and (valid is None or bool(valid[i])) and matches(flt, r)
    return np.packbits(bits, bitorder="little"), int(bits.sum())
