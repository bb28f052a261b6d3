"""CPU suite: the batch planner of metadata filters (leann-rs_amd/csrc/meta_batch_plan.h) against tests/filter_ref.py, a literal
restatement of the reference's filter.rs.  host/meta_batch_selftest.cpp is built with the host compiler under AddressSanitizer +
UBSan; it plans a batch of filter trees against given dictionaries — shared programs, union column tables, relocated words, launches
cut at the caps — runs every planned launch over given columns with the header's scalar interpreter and prints every output's
bitmap.  All comparisons are exact, bit for bit.  No GPU."""
import os
import subprocess

import pytest

import filter_ref as fr
import meta_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "leann-rs_amd", "host", "meta_batch_selftest")
F = [f for _, f in mc.matrix_filters() + mc.CORNERS]
MAX_PROGRAMS, MAX_COLS = 64, 16  # MB_MAX_PROGRAMS, MB_MAX_COLS


@pytest.fixture(scope="module")
def selftest():
    subprocess.check_call(["make", "-s", "-C", ROOT, "leann-rs_amd/host/meta_batch_selftest"])  # a no-op when up to date
    return EXE


def _run(selftest, records, filters, poison=False, fields=None):
    """(launches, n_distinct, [(programs, union columns, words, pairs) per launch], bitmap lines) or the error message"""
    if fields is None:
        fields = sorted(set(x for f in filters for x in mc.fields_of(f)))
    text = mc.selftest_input(records, fields, filters, poison) + "batch\n"
    p = subprocess.run([selftest], input=text.encode(), stdout=subprocess.PIPE, check=True)
    lines = p.stdout.decode().splitlines()
    if lines[0].startswith("err "):
        assert len(lines) == 1
        return lines[0][4:]
    head = lines[0].split()
    assert head[0] == "plan" and len(lines) == 1 + len(filters)
    launches = [tuple(int(x) for x in part.split("/")) for part in head[3:]]
    assert len(launches) == int(head[1]) and sum(l[0] for l in launches) == int(head[2]) and sum(l[3] for l in launches) == len(filters)
    for programs, cols, words, pairs in launches:
        assert 1 <= programs <= MAX_PROGRAMS and cols <= MAX_COLS and words <= 1 << 20 and words % 2 == 0
    return int(head[1]), int(head[2]), launches, lines[1:]


def _check(records, filters, lines):
    for f, line in zip(filters, lines):
        want, _ = fr.bitmap(f, records)
        assert line == "ok " + want.tobytes().hex(), (f, line)


def test_the_shared_cases_are_what_the_suite_counts_on():
    assert len(F) == 106 and len(mc.MATRIX_RECORDS) == 31
    assert sorted(set(x for f in F for x in mc.fields_of(f))) == ["f", "f.g", "g", "nope"]
    allowed = [sum(fr.matches(f, r) for r in mc.MATRIX_RECORDS) for f in F]
    assert allowed.count(0) == 18 and allowed.count(len(mc.MATRIX_RECORDS)) == 9


def test_all_filters_as_one_batch(selftest):
    n_launches, n_distinct, launches, lines = _run(selftest, mc.MATRIX_RECORDS, F)
    _check(mc.MATRIX_RECORDS, F, lines)
    assert n_launches <= 2 and n_distinct <= len(F)
    assert n_launches == (n_distinct + MAX_PROGRAMS - 1) // MAX_PROGRAMS  # 4 fields, few words: only the program cap cuts
    # every output twice, the second time in reverse: the same programs, packed as before
    both = F + F[::-1]
    n_launches2, n_distinct2, launches2, lines2 = _run(selftest, mc.MATRIX_RECORDS, both)
    _check(mc.MATRIX_RECORDS, both, lines2)
    assert (n_launches2, n_distinct2) == (n_launches, n_distinct)
    assert [l[:3] for l in launches2] == [l[:3] for l in launches] and sum(l[3] for l in launches2) == 2 * len(F)


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
def test_several_bitsets_in_one_words_block(selftest, poison):
    """contains / endswith / in / notin over 5000 distinct strings: four bitsets one behind the other, str_a rebased for them and left
    alone for the range ops; poisoned: a planned program reads a number or code only where the tag says so"""
    recs, filters = mc.dictionary_records(5000), mc.dictionary_filters(5000)
    n_launches, n_distinct, launches, lines = _run(selftest, recs, filters, poison)
    _check(recs, filters, lines)
    assert n_launches == 1 and n_distinct == len(filters)
    assert launches[0][2] >= 4 * ((5000 + 31) // 32 + 1)


def test_matrix_with_poisoned_columns(selftest):
    _, _, _, lines = _run(selftest, mc.MATRIX_RECORDS, F, poison=True)
    _check(mc.MATRIX_RECORDS, F, lines)


def _wide_records(n_fields=20, n=37):
    return [{f"c{j:02d}": ((i * (j + 3)) % 7 if (i + j) % 5 else f"s{(i + j) % 4}") for j in range(n_fields) if (i + 2 * j) % 11} for i in range(n)]


def wide_filters(n_fields=20):
    """20 single-field filters over 20 distinct fields, then one filter over 8 fields: more columns than a launch takes"""
    single = [("cond", f"c{j:02d}", "gte", 3) if j % 2 else ("cond", f"c{j:02d}", "in", ["s1", 2, "s3"]) for j in range(n_fields)]
    eight = ("or", [("and", [("cond", f"c{j:02d}", "lt", 4), ("cond", f"c{j + 1:02d}", "exists", None)]) for j in range(0, 8, 2)])
    return single + [eight]


def test_column_cap_starts_a_new_launch(selftest):
    recs, filters = _wide_records(), wide_filters()
    n_launches, n_distinct, launches, lines = _run(selftest, recs, filters)
    _check(recs, filters, lines)
    assert n_distinct == 21 and n_launches >= 2 and all(l[1] <= MAX_COLS for l in launches)
    assert launches[0][:2] == (16, 16)  # greedy, in order of first appearance: sixteen one-column programs fill the first table


def test_program_cap_starts_a_new_launch(selftest):
    for k, want in ((MAX_PROGRAMS, [64]), (MAX_PROGRAMS + 1, [64, 1])):
        filters = [("cond", "f", "eq", i) for i in range(k)]
        n_launches, n_distinct, launches, lines = _run(selftest, mc.MATRIX_RECORDS, filters)
        _check(mc.MATRIX_RECORDS, filters, lines)
        assert n_distinct == k and [l[0] for l in launches] == want


def test_a_bad_filter_is_named_by_its_index(selftest):
    good = [("cond", "f", "eq", i) for i in range(8)]
    bad = list(good)
    bad[3] = ("cond", "nowhere.at.all", "exists", None)
    assert _run(selftest, mc.MATRIX_RECORDS, bad, fields=["f"]) == "filter 3: metadata filter: no column for field 'nowhere.at.all'"
    bad = list(good)
    bad[5] = ("and", [("cond", "f", "gt", i) for i in range(33)])
    assert _run(selftest, mc.MATRIX_RECORDS, bad) == "filter 5: metadata filter: more than 32 conditions (the limit)"
