"""CPU suite: the metadata-filter compiler (leann-rs_amd/csrc/meta_plan.h) against tests/filter_ref.py, a literal restatement of the
reference's filter.rs.  host/meta_plan_selftest.cpp is built with the host compiler under AddressSanitizer + UBSan; it compiles a
filter tree against given dictionaries, runs the compiled program over given columns with the header's scalar interpreter and
prints the bitmap.  All comparisons are exact, bit for bit.  The restatement itself is held to the oracle's parse_filter on the
subset both cover, to the reference's own assertions (filter.rs:445-551) and to the C++ MetadataFilter (host_selftest).  The Python
parser twin (leann_rs_amd.metadata.parse_filter) is held to the restatement's.  No GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

import filter_ref as fr
import meta_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "leann-rs_amd", "host", "meta_plan_selftest")


@pytest.fixture(scope="module")
def selftest():
    subprocess.check_call(["make", "-s", "-C", ROOT, "leann-rs_amd/host/meta_plan_selftest"])  # a no-op when up to date
    return EXE


def _run(selftest, records, filters, poison=False):
    fields = sorted(set(x for f in filters for x in mc.fields_of(f)))
    p = subprocess.run([selftest], input=mc.selftest_input(records, fields, filters, poison).encode(), stdout=subprocess.PIPE, check=True)
    lines = p.stdout.decode().splitlines()
    assert len(lines) == len(filters)
    return lines


def _check(selftest, records, named_filters, poison=False):
    filters = [f for _, f in named_filters]
    for (name, f), line in zip(named_filters, _run(selftest, records, filters, poison)):
        want, _ = fr.bitmap(f, records)
        assert line == "ok " + want.tobytes().hex(), (name, f, line)


# ---- the restatement is held to three things ---------------------------------------------------------------------------------
REFERENCE_ASSERTIONS = [  # filter.rs:445-551
    ("source:*.rs", {"source": "main.rs", "type": "code", "lines": 100}, True),
    ("type=code", {"source": "main.rs", "type": "code", "lines": 100}, True),
    ("lines>50", {"source": "main.rs", "type": "code", "lines": 100}, True),
    ("type in [code,text,doc]", {"type": "code", "lang": "rust"}, True),
    ("type in [text,doc]", {"type": "code", "lang": "rust"}, False),
    ("type not_in [text,doc]", {"type": "code"}, True),
    ("type not_in [code,text]", {"type": "code"}, False),
    ("type=code,lines>50", {"type": "code", "lines": 100}, True),
    ("type=code AND lines>50", {"type": "code", "lines": 100}, True),
    ("type=code,lines>200", {"type": "code", "lines": 100}, False),
    ("type=code OR type=text", {"type": "code"}, True),
    ("type=text OR type=doc", {"type": "code"}, False),
    ("source~main", {"source": "/path/to/main.rs"}, True),
    ("source:*main*", {"source": "/path/to/main.rs"}, True),
    ("source?", {"source": "main.rs"}, True),
    ("missing?", {"source": "main.rs"}, False),
]
FILTER_TEXTS = [t for t, _, _ in REFERENCE_ASSERTIONS] + [  # the doc comment of parse (filter.rs:42-51) and more of the surface
    "type=code", "type in [code,text,doc]", "type not_in [code,text]", "source~keyword", "source:*keyword*", "source^prefix",
    "source:prefix*", "source$suffix", "source:*suffix", "field?", "lines>=100", "lines<=100.5", "lines<100", "type!=code",
    "meta.lang=rust", "flag=true", "flag=false", "x=-3", "x=+3", "x=1e3", "x=.5", "x=5.", "x=inf", "x=nan", "x=9223372036854775808",
    "a=1 OR b=2 AND c=3 OR d in [1,x,true]", "a=1,b in [1,2],c^x", "a^b>=c", "a:**", "a:*", "a=b=c", "nothing", " a = b ", "a=1 OR nothing",
    "a in [1,2", "a~", "x=1_0", "x= 5",
]


def test_restatement_passes_the_references_own_assertions():
    assert fr.parse("source:*.rs")[0] == "cond"
    for text, meta, want in REFERENCE_ASSERTIONS:
        assert fr.matches(fr.parse(text), meta) is want, text


def test_restatement_agrees_with_the_oracle_on_its_subset():
    import searcher_oracle as so
    rng = np.random.default_rng(7)
    recs = []
    for i in range(200):
        r = {}
        if rng.random() < 0.8:
            r["type"] = ["code", "text", "doc"][int(rng.integers(3))]
        if rng.random() < 0.8:
            r["lines"] = [int(rng.integers(200)), float(rng.integers(200)) + 0.5, True][int(rng.integers(3))]
        if rng.random() < 0.7:
            r["source"] = f"/p/{i % 7}/main{i % 3}.{['rs', 'py'][i % 2]}"
        if rng.random() < 0.3:
            r["meta"] = {"lang": ["rust", 5][i % 2]}
        recs.append(r)  # (no null fields: the oracle treats null as missing)
    for text in ("type=code", "lines>50", "lines>=100,type!=doc", "source:*.rs", "source:/p/1*", "source:*main1*", "type!=code AND lines<=70.5",
                 "meta.lang=rust", "lines=true", "type>=d", "lines<abc"):
        flt, orc = fr.parse(text), so.parse_filter(text)
        for r in recs:
            assert fr.matches(flt, r) == orc(r), (text, r)


def test_restatement_agrees_with_the_cpp_metadata_filter(tmp_path):
    exe = os.path.join(ROOT, "leann-rs_amd", "host", "host_selftest")
    subprocess.check_call(["make", "-s", "-C", ROOT, "leann-rs_amd/host/host_selftest"])
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_formulas.json")))
    metas = [{"f": r["f"]} if "f" in r else dict(r) for r in mc.MATRIX_RECORDS if not isinstance(r.get("f"), float) or r["f"] == r["f"]]
    texts = ["f=5", "f!=5", "f>5", "f>=5", "f<5", "f<=5", "f=abc", "f!=abc", "f>abc", "f>=abc", "f<abc", "f<=abc", "f=true", "f!=true", "f>=true",
             "f<true", "f in [5,abc,true,b]", "f not_in [5,abc,true,b]", "f~bc", "f^abc", "f$.rs", "f?", "f.g=5", "f.g!=5", "f:*", "f~",
             "f>=0 AND f<5 OR f^ab AND f!=abc", "f=9007199254740992", "f=0", "f<0", "f=5.000000000000001"]
    cases = dict(gold)
    cases["filters"] = [dict(filter=t, metadata=m) for t in texts for m in metas]
    cases["synthetic_embed"] = "x"
    p = tmp_path / "cases.json"
    p.write_text(json.dumps(cases))
    got = json.loads(subprocess.check_output([exe, str(p)]))["filters"]
    want = [fr.matches(fr.parse(t), m) for t in texts for m in metas]
    bad = [(c["filter"], c["metadata"], g, w) for c, g, w in zip(cases["filters"], got, want) if g is not w]
    assert not bad, bad[:5]


def test_parser_twin(la):
    for text in FILTER_TEXTS:
        assert repr(la.parse_filter(text)) == repr(fr.parse(text)), text


# ---- the compiler ----------------------------------------------------------------------------------------------------------------
def test_matrix_every_op_type_and_tag(selftest):
    tags = set(mc.column(mc.MATRIX_RECORDS, "f")[1])
    assert tags == set(range(7))  # every row tag is there
    named = mc.matrix_filters()
    assert len(named) == 12 * 5
    _check(selftest, mc.MATRIX_RECORDS, named)


@pytest.mark.parametrize("name,flt", mc.CORNERS, ids=[n for n, _ in mc.CORNERS])
def test_corner(selftest, name, flt):
    _check(selftest, mc.MATRIX_RECORDS, [(name, flt)])


def test_corners_say_what_their_names_say():
    """the expected side itself, spelled out for the corners whose answer is easy to get wrong"""
    R = mc.MATRIX_RECORDS
    present = [i for i, r in enumerate(R) if "f" in r]
    by = dict(mc.CORNERS)

    def rows(name):
        return [i for i, r in enumerate(R) if fr.matches(by[name], r)]
    assert rows("bool_rhs_makes_gte_exists") == present == rows("null_rhs_makes_lte_exists") == rows("exists_true_for_null")
    assert rows("bool_rhs_makes_gt_never") == [] == rows("null_rhs_makes_lt_never") == rows("eq_in_ordered_false_on_missing")
    non_numbers = [i for i in present if not fr._is_number(R[i]["f"])]
    assert set(non_numbers) <= set(rows("gte_is_true_for_every_present_row_of_another_type"))
    assert 0 in rows("ne_true_on_missing") and 0 in rows("notin_true_on_missing")
    assert [R[i]["f"] for i in rows("number_1_is_not_true")] == [1] and [R[i]["f"] for i in rows("true_is_not_number_1")] == [True]
    assert [R[i]["f"] for i in rows("string_5_is_not_number_5")] == ["5"]
    assert [R[i]["f"] for i in rows("1e_17_apart_is_equal")] == [5, 5.0 + 1e-17] and [R[i]["f"] for i in rows("1e_15_apart_is_not")] == [5.0 + 1e-15]
    assert [R[i]["f"] for i in rows("number_2_53_plus_1_rounds_as_the_reference")] == [2 ** 53 + 1]
    assert [repr(R[i]["f"]) for i in rows("minus_zero_equals_zero")] == ["-0.0", "0"] and rows("minus_zero_not_below_zero") == [12]
    assert [R[i]["f"] for i in rows("non_ascii_order_is_bytewise")] == ["\U0001f600"]
    assert len(rows("in_without_a_list_is_false")) == 0 and len(rows("notin_without_a_list_is_true")) == len(R)
    strings = [i for i in present if isinstance(R[i]["f"], str)]
    assert rows("contains_empty_is_every_string") == strings == rows("pattern_op_with_a_number_uses_the_empty_pattern")


def test_columns_are_read_only_where_the_tag_says_so(selftest):
    _check(selftest, mc.MATRIX_RECORDS, mc.matrix_filters() + mc.CORNERS, poison=True)


@pytest.mark.parametrize("D", [0, 1, 31, 32, 33, 64, 65, 5000])
def test_dictionary_sizes(selftest, D):
    recs = mc.dictionary_records(D)
    assert len(mc.column(recs, "s")[0]) == D
    _check(selftest, recs, [(f"D={D}", f) for f in mc.dictionary_filters(D)])


def test_ranges_and_prefix_ranges(selftest):
    _check(selftest, mc.RANGE_RECORDS, [("range", f) for f in mc.RANGE_FILTERS])


def test_bytewise_order_is_pythons_order_on_encode():
    d = mc.column(mc.MATRIX_RECORDS, "f")[0]
    assert d == sorted(d) and d.index("～".encode()) < d.index("\U0001f600".encode())
    assert sorted(["～", "\U0001f600"], key=lambda s: s.encode("utf-16-be")) == ["\U0001f600", "～"]  # UTF-16 order is the other one


@pytest.mark.parametrize("depth", [1, 2, 7, 8])
def test_nesting_up_to_the_depth_limit(selftest, depth):
    _check(selftest, mc.MATRIX_RECORDS, [(f"depth {depth}", mc.nested_filter(depth))])


def test_each_limit_is_refused_one_past_it(selftest):
    out = subprocess.run([selftest, "--limits"], stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    got = {line.split(" ", 2)[0]: (int(line.split(" ", 2)[1]), line.split(" ", 2)[2].strip()) for line in out}
    for name in ("conds", "depth", "groups", "cols", "words"):
        assert got[name + "_at"] == (0, ""), name
    assert got["conds_past"] == (1, "metadata filter: more than 32 conditions (the limit)")
    assert got["depth_past"] == (1, "metadata filter: nested deeper than 8 AND / OR levels (the limit)")
    assert got["groups_past"] == (1, "metadata filter: more than 32 AND / OR nodes (the limit)")
    assert got["cols_past"] == (1, "metadata filter: more than 8 distinct fields (the limit)")
    assert got["words_past"] == (1, "metadata filter: more than 1048576 words of number sets and dictionary bitsets (the limit)")
    assert got["no_column"] == (1, "metadata filter: no column for field 'nowhere.at.all'")
    assert got["short_tree"][0] == 1 and "ends before its last node" in got["short_tree"][1]
    assert got["long_tree"][0] == 1 and "behind the end of the tree" in got["long_tree"][1]
    (line,) = _run(selftest, mc.MATRIX_RECORDS, [mc.nested_filter(9)])
    assert line == "err metadata filter: nested deeper than 8 AND / OR levels (the limit)"
