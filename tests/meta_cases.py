"""Record sets and filters shared by the metadata-filter tests (test_cpu_meta_plan.py drives host/meta_plan_selftest with them,
test_gpu_meta_filter.py the device), and the plain column extraction both use for the expected side's input.  A string value may
be given as bytes where a case needs bytes no JSON text can hold (0xFF)."""
import bisect
import struct

import filter_ref as fr

TAG_MISSING, TAG_NULL, TAG_FALSE, TAG_TRUE, TAG_NUMBER, TAG_STRING, TAG_OTHER = range(7)

# one row per tag and corner for field "f": missing, null, both bools, numbers (around 5 under the epsilon rule, 2^53 + 1, -0.0),
# strings (empty, "5", entries that are proper prefixes of others, non-ASCII whose UTF-16 order differs from the bytewise one), array, object
MATRIX_RECORDS = [
    {}, {"f": None}, {"f": False}, {"f": True},
    {"f": 5}, {"f": 5.0 + 1e-17}, {"f": 5.0 + 1e-15}, {"f": 4.999}, {"f": -0.0}, {"f": 0}, {"f": 1}, {"f": 2 ** 53 + 1}, {"f": -7.5}, {"f": 100},
    {"f": ""}, {"f": "5"}, {"f": "abc"}, {"f": "ab"}, {"f": "abd"}, {"f": "abc.rs"}, {"f": "b"}, {"f": "true"}, {"f": "Zebra"},
    {"f": "été"}, {"f": "～"}, {"f": "\U0001f600"}, {"f": "abc"},
    {"f": [5, "abc"]}, {"f": {"g": 5}}, {"g": 5}, {"f": []},
]
MATRIX_VALUES = {  # right-hand sides by type
    "number": 5, "string": "abc", "bool": True, "null": None, "list": [5, "abc", True, None, "b", 0.0],
}


def matrix_filters():
    """every op x every right-hand type, as (name, filter)"""
    return [(f"{op}-{kind}", ("cond", "f", op, v)) for op in fr.OPS for kind, v in MATRIX_VALUES.items()]


# the corners DESIGN.md §3c / meta_plan.h name, one by one, over MATRIX_RECORDS
CORNERS = [
    ("gte_is_true_for_every_present_row_of_another_type", ("cond", "f", "gte", 5)),
    ("lte_is_true_for_every_present_row_of_another_type", ("cond", "f", "lte", "abc")),
    ("gt_lt_false_for_another_type", ("or", [("cond", "f", "gt", "abc"), ("cond", "f", "lt", 5)])),
    ("bool_rhs_makes_gte_exists", ("cond", "f", "gte", True)),
    ("null_rhs_makes_lte_exists", ("cond", "f", "lte", None)),
    ("bool_rhs_makes_gt_never", ("cond", "f", "gt", False)),
    ("null_rhs_makes_lt_never", ("cond", "f", "lt", None)),
    ("ne_true_on_missing", ("cond", "f", "ne", 5)),
    ("notin_true_on_missing", ("cond", "f", "notin", [5, "abc"])),
    ("eq_in_ordered_false_on_missing", ("or", [("cond", "nope", "eq", 5), ("cond", "nope", "in", [5]), ("cond", "nope", "gte", 5), ("cond", "nope", "lte", "a")])),
    ("number_1_is_not_true", ("cond", "f", "eq", 1)),
    ("true_is_not_number_1", ("cond", "f", "eq", True)),
    ("string_5_is_not_number_5", ("cond", "f", "eq", "5")),
    ("null_equals_null", ("cond", "f", "eq", None)),
    ("exists_true_for_null", ("cond", "f", "exists", None)),
    ("string_value_absent_from_dictionary_orders", ("and", [("cond", "f", "gt", "abca"), ("cond", "f", "lt", "abe")])),
    ("string_eq_absent", ("cond", "f", "eq", "abca")),
    ("string_ne_absent", ("cond", "f", "ne", "abca")),
    ("startswith_entry_that_prefixes_another", ("cond", "f", "startswith", "abc")),
    ("startswith_empty", ("cond", "f", "startswith", "")),
    ("contains_empty_is_every_string", ("cond", "f", "contains", "")),
    ("endswith_empty_is_every_string", ("cond", "f", "endswith", "")),
    ("contains", ("cond", "f", "contains", "bc")),
    ("endswith", ("cond", "f", "endswith", ".rs")),
    ("in_mixed_is_the_union", ("cond", "f", "in", [None, False, 100, "b", "été", "nothere"])),
    ("notin_mixed", ("cond", "f", "notin", [None, False, 100, "b", "été", "nothere"])),
    ("in_empty_list", ("cond", "f", "in", [])),
    ("notin_empty_list", ("cond", "f", "notin", [])),
    ("in_without_a_list_is_false", ("cond", "f", "in", "abc")),
    ("notin_without_a_list_is_true", ("cond", "f", "notin", 5)),
    ("pattern_op_with_a_number_uses_the_empty_pattern", ("cond", "f", "startswith", 5)),
    ("contains_with_null_uses_the_empty_pattern", ("cond", "f", "contains", None)),
    ("eq_against_a_list_equals_nothing", ("cond", "f", "eq", [5])),
    ("ne_against_a_list", ("cond", "f", "ne", [5])),
    ("number_2_53_plus_1_rounds_as_the_reference", ("cond", "f", "eq", 2 ** 53)),
    ("minus_zero_equals_zero", ("cond", "f", "eq", 0)),
    ("minus_zero_not_below_zero", ("cond", "f", "lt", 0)),
    ("1e_17_apart_is_equal", ("cond", "f", "eq", 5.0)),
    ("1e_15_apart_is_not", ("cond", "f", "eq", 5.0 + 1e-15)),
    ("in_numbers_under_the_epsilon", ("cond", "f", "in", [5.0 + 1e-15, -7.5])),
    ("nested_path", ("cond", "f.g", "eq", 5)),
    ("indexing_into_a_string_is_missing", ("cond", "f.g", "ne", 5)),
    ("non_ascii_order_is_bytewise", ("cond", "f", "gt", "～")),   # U+FF5E sorts above U+1F600 in UTF-16, below it bytewise
    ("non_ascii_range", ("and", [("cond", "f", "gte", "é"), ("cond", "f", "lte", "～")])),
    ("or_of_ands", ("or", [("and", [("cond", "f", "gte", 0), ("cond", "f", "lt", 5)]), ("and", [("cond", "f", "startswith", "ab"), ("cond", "f", "ne", "abc")])])),
    ("two_fields", ("and", [("cond", "f", "exists", None), ("cond", "g", "ne", 5)])),
]


def nested_filter(depth):
    """AND / OR alternating `depth` levels deep, conditions at every level"""
    f = ("cond", "f", "gte", 1)
    for d in range(depth):
        kind = "and" if d % 2 == 0 else "or"
        other = ("cond", "f", "ne", "abc") if kind == "and" else ("cond", "f", "eq", d)
        f = (kind, [other, f, ("cond", "f", "exists", None)] if kind == "and" else [other, f])
    return f


def dictionary_records(D):
    """D distinct strings in field "s" in a shuffled, repeating order, plus rows of the other tags; some strings contain "7", end in "3" """
    words = [f"w{(i * 7919) % D:05d}" for i in range(D)]
    recs = [{"s": w} for w in words] + [{"s": words[i]} for i in range(0, D, 3)]
    return recs + [{}, {"s": None}, {"s": 7}, {"s": ["w00000"]}]


def dictionary_filters(D):
    some = [f"w{i:05d}" for i in (0, D // 2, D - 1, D, 31, 32, 33, 63, 64) if i >= 0]
    return [("cond", "s", "contains", "7"), ("cond", "s", "endswith", "3"), ("cond", "s", "in", some), ("cond", "s", "notin", some),
            ("cond", "s", "gte", f"w{D // 2:05d}"), ("cond", "s", "lt", f"w{max(D - 1, 0):05d}"), ("cond", "s", "startswith", "w0003"),
            ("cond", "s", "ne", "w00031"), ("cond", "s", "eq", f"w{max(D - 1, 0):05d}"), ("cond", "s", "startswith", "")]


# ranges and prefix ranges, over raw bytes: entries "b", "d", "d\xff", "d\xff\xff", "d\xffz", "e", "f" + a proper-prefix pair
RANGE_RECORDS = [{"s": v} for v in (b"b", b"d", b"d\xff", b"d\xff\xff", b"d\xffz", b"e", b"f", b"fa", b"\xff", b"\xff\xff", b"b", b"")] + [{}, {"s": 1}]
RANGE_FILTERS = (
    [("cond", "s", op, v) for op in ("eq", "ne", "gt", "gte", "lt", "lte") for v in (b"a", b"c", b"d", b"g", b"\xff\xff\xff", b"")]  # below, between, equal, above
    + [("cond", "s", "startswith", p) for p in (b"", b"d\xff", b"d\xff\xff", b"\xff", b"\xff\xff", b"\xff\xff\xff", b"f", b"fa", b"d", b"c", b"z")]
    + [("cond", "s", "contains", b"\xff"), ("cond", "s", "endswith", b"\xff"), ("cond", "s", "in", [b"d\xff", b"", b"nope"])]
)


# ---- plain column extraction and the selftest's text protocol -----------------------------------------------------------------
def column(records, field):
    """(dictionary: sorted distinct bytes, tag list, num list, code list) of one field; records[i] None = unreadable (MISSING)"""
    tags, nums, strs = [], [], []
    for r in records:
        v = fr.get_nested_value(r, field) if r is not None else fr._MISSING
        num, s = 0.0, None
        if v is fr._MISSING:
            t = TAG_MISSING
        elif v is None:
            t = TAG_NULL
        elif isinstance(v, bool):
            t = TAG_TRUE if v else TAG_FALSE
        elif isinstance(v, (int, float)):
            t, num = TAG_NUMBER, float(v)
        elif isinstance(v, (str, bytes)):
            t, s = TAG_STRING, (v.encode() if isinstance(v, str) else v)
        else:
            t = TAG_OTHER
        tags.append(t)
        nums.append(num)
        strs.append(s)
    dictionary = sorted(set(s for s in strs if s is not None))  # Python orders bytes bytewise, a proper prefix first
    codes = [bisect.bisect_left(dictionary, s) if s is not None else 0 for s in strs]
    return dictionary, tags, nums, codes


def _hex(b):
    b = b.encode() if isinstance(b, str) else b
    return b.hex() if b else "-"


def _f64(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _value(v, in_list=False):
    if v is None:
        return "n"
    if isinstance(v, bool):
        return f"b {int(v)}"
    if isinstance(v, (int, float)):
        return f"f {_f64(v)}"
    if isinstance(v, (str, bytes)):
        return f"s {_hex(v)}"
    assert not in_list
    return " ".join([f"l {len(v)}"] + [_value(x, True) for x in v])


def filter_text(flt):
    lines = []

    def walk(f):
        if f[0] == "cond":
            lines.append(f"C {_hex(f[1])} {fr.OPS.index(f[2])} {_value(f[3])}")
        else:
            lines.append(f"{'A' if f[0] == 'and' else 'O'} {len(f[1])}")
            for c in f[1]:
                walk(c)
    walk(flt)
    return f"filter {len(lines)}\n" + "\n".join(lines) + "\n"


def fields_of(flt):
    return [flt[1]] if flt[0] == "cond" else sorted(set(x for c in flt[1] for x in fields_of(c)))


def selftest_input(records, fields, filters, poison=False):
    """the selftest's stdin: the columns of `fields` over `records`, then the filters.  poison: num / code of rows with another tag
    hold NaN / 0xFFFFFFFF — a compiled program reads them only where the tag says so."""
    out = [f"n {len(records)}"]
    for f in fields:
        d, tags, nums, codes = column(records, f)
        out.append(f"column {_hex(f)} {len(d)} " + " ".join(_hex(x) for x in d))
        for t, x, c in zip(tags, nums, codes):
            if poison:
                x = x if t == TAG_NUMBER else float("nan")
                c = c if t == TAG_STRING else 0xFFFFFFFF
            out.append(f"{t} {_f64(x)} {c}")
    return "\n".join(out) + "\n" + "".join(filter_text(f) for f in filters)
