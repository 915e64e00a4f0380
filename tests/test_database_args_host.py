"""What every igd_amd.*_host function that takes regions refuses before it computes, and with which words.  No GPU.

One table over the public host functions: a tiny database (sets_fixtures.wide_db: one contig, three files), three regions in two
sets, and per function one bad argument at a time.  Every refusal is an IgdError whose text starts with the function's own name,
leaves no file descriptor open, and is the same the second time.  The texts asserted here are the ones the functions raise:
they are the contract of the argument layer of igd_amd/database.py, whichever helper writes them.

search_host and support_host never compared the lengths of ichr, qs and qe (nor does Database.search): they are not in the
`qe_short` column."""
import os
import random
import shutil

import numpy as np
import pytest

import igd_amd
from igd_amd.database import IgdError
from helpers import short_tmpdir
from sets_fixtures import NBP, wide_db

REGIONS = dict(ichr=[0, 0, 0], qs=[100, 5000, 40000], qe=[300, 5100, 41000])
SETS = dict(set_off=[0, 2, 3])
UNIVERSE = dict(u_ichr=[0, 0], u_qs=[0, 30000], u_qe=[6000, 50000])
CTG = dict(ctg_len=[200000])

# name -> (takes igd_path, the good keyword arguments, the features that have a bad value)
HOST = {
    "restrict_host": (False, {**REGIONS, **SETS, **UNIVERSE}, ("qe", "sets", "universe")),
    "enrich_restricted_host": (True, {**REGIONS, **SETS, **UNIVERSE}, ("qe", "sets", "universe")),
    "cooccur_host": (True, {**REGIONS}, ("qe",)),
    "search_host": (True, {**REGIONS}, ("min_overlap",)),
    "support_host": (True, {**REGIONS}, ("min_overlap",)),
    "permute_regions_host": (False, {**REGIONS, **CTG, "p0": 0, "np_": 2}, ("qe", "mode")),
    "permute_host": (True, {**REGIONS, **CTG, "nperm": 2}, ("qe", "ctg_len", "mode", "min_overlap")),
    "permute_nearest_host": (True, {**REGIONS, **CTG, "nperm": 2, "window": 1000}, ("qe", "ctg_len", "mode", "window")),
    "permute_bp_host": (True, {**REGIONS, **CTG, "nperm": 2}, ("qe", "ctg_len", "mode")),
    "nearest_host": (True, {**REGIONS, "window": 1000}, ("qe", "window")),
    "nearest_sets_host": (True, {**REGIONS, **SETS, "window": 1000}, ("qe", "sets", "window")),
    "nearest_signed_host": (True, {**REGIONS, "window": 1000}, ("qe", "window")),
    "nearest_hist_host": (True, {**REGIONS, **SETS, "window": 1000, "edges": [-10, 0, 10]}, ("qe", "sets", "window", "edges")),
    "flanks_host": (True, {**REGIONS, "window": 1000}, ("qe", "window", "measure")),
    "flank_reldist_host": (True, {**REGIONS, **SETS, "window": 1000, "nbins": 4}, ("qe", "sets", "window", "measure", "nbins")),
    "merge_host": (True, {**REGIONS, **SETS}, ("qe", "sets", "gap")),
    "jaccard_host": (True, {**REGIONS, **SETS}, ("qe", "sets")),
    "map_host": (True, {**REGIONS}, ("qe", "op")),
    "map_sets_host": (True, {**REGIONS, **SETS}, ("qe", "sets", "op")),
}
# feature -> [(case, the one argument that is bad, a piece of the text after the function's name)]
BAD = {
    "qe": [("qe_short", dict(qe=[300, 5100]), "3 / 3 / 2")],
    "sets": [("set_off_empty", dict(set_off=[]), "set_off needs nsets + 1 entries"),
             ("set_off_last", dict(set_off=[0, 2, 4]), "set_off[-1] = 4, but 3 / 3 / 3")],
    "universe": [("u_qe_short", dict(u_qe=[6000]), "2 / 2 / 1 universe regions given")],
    "ctg_len": [("ctg_len_short", dict(ctg_len=[]), "ctg_len has 0 entries, the database 1 contigs")],
    "mode": [("mode", dict(mode="bogus"), "mode must be 'circular' or 'shuffle', not 'bogus'")],
    "min_overlap": [("min_overlap", dict(min_overlap="x"), "min_overlap must be None, an int (base pairs) or a MinOverlap, not 'x'")],
    "window": [("window", dict(window=2 ** 31), "window 2147483648 outside 0 .. 1073741824")],
    "edges": [("edges_tie", dict(edges=[5, 5]), "edges must be strictly ascending int32 values"),
              ("edges_none", dict(edges=[]), "edges must be 1 to 63 integers")],
    "measure": [("measure", dict(measure="centres"), "measure must be \"edges\" or \"midpoints\"")],
    "nbins": [("nbins", dict(nbins=0), "nbins must be an integer from 1 to 64")],
    "gap": [("gap", dict(gap=-1), "gap must be an integer from 0 to 1073741824")],
    "op": [("op", dict(op="mean"), "op 'mean' is none of count, sum, min, max")],
}
CASES = [(name, case, over, text) for name, (_, _, feats) in HOST.items() for f in feats for case, over, text in BAD[f]]
WITH_PATH = [name for name, (takes_path, _, _) in HOST.items() if takes_path]
BY_HAND = ("enrich_restricted_host", "cooccur_host", "permute_host")           # (these opened header, index and tiles themselves)


@pytest.fixture(scope="module")
def db_path():
    d = short_tmpdir("iah")
    path, span, _, _ = wide_db(random.Random(4100), d, "tiny", 3, NBP, 4)
    assert span > max(REGIONS["qe"]) and CTG["ctg_len"][0] > span
    yield path
    shutil.rmtree(d, ignore_errors=True)


def open_fds():
    return len(os.listdir("/proc/self/fd"))


def call(name, db_path, **over):
    takes_path, kw, _ = HOST[name]
    kw = {**kw, **over}
    if takes_path:
        kw["igd_path"] = over.get("igd_path", db_path)
    return getattr(igd_amd, name)(**kw)


def refused(name, db_path, **over):
    """the text of the IgdError, raised twice alike and without an open file left behind"""
    call(name, db_path)                                            # (whatever the first call caches is there before fds are counted)
    before = open_fds()
    texts = []
    for _ in range(2):
        with pytest.raises(IgdError) as e:
            call(name, db_path, **over)
        texts.append(str(e.value))
    assert texts[0] == texts[1]
    assert open_fds() == before, "%s left a file open behind its refusal" % name
    return texts[0]


def test_the_table_names_every_host_function_that_takes_regions():
    import inspect
    takes = {n for n in igd_amd.__all__ if n.endswith("_host") and "qs" in inspect.signature(getattr(igd_amd, n)).parameters}
    assert takes == set(HOST)


@pytest.mark.parametrize("name", sorted(HOST))
def test_the_good_arguments_are_accepted(db_path, name):
    call(name, db_path)


@pytest.mark.parametrize("name,case,over,text", CASES, ids=["%s-%s" % c[:2] for c in CASES])
def test_one_bad_argument_is_refused_under_the_functions_name(db_path, name, case, over, text):
    got = refused(name, db_path, **over)
    assert got.startswith(name + ": ") and text in got, got
    call(name, db_path)                                            # and the next good call works


def test_the_set_texts_in_full(db_path):
    """the noun is the function's own: queries where the sets are searched, regions where they are measured"""
    assert refused("restrict_host", db_path, qe=[300, 5100]) == \
        "restrict_host: set_off[-1] = 3, but 3 / 3 / 2 queries and 2 / 2 / 2 universe regions given"
    assert refused("enrich_restricted_host", db_path, set_off=[0, 2, 4]) == \
        "enrich_restricted_host: set_off[-1] = 4, but 3 / 3 / 3 queries and 2 / 2 / 2 universe regions given"
    assert refused("nearest_sets_host", db_path, qe=[300, 5100]) == "nearest_sets_host: set_off[-1] = 3, but 3 / 3 / 2 regions given"
    assert refused("map_sets_host", db_path, set_off=[0, 2, 4]) == "map_sets_host: set_off[-1] = 4, but 3 / 3 / 3 regions given"
    assert refused("cooccur_host", db_path, qe=[300, 5100]) == "cooccur_host: 3 / 3 / 2 regions given"
    assert refused("permute_bp_host", db_path, ctg_len=[[200000]]) == "permute_bp_host: 3 / 3 / 3 regions given"
    assert refused("merge_host", db_path, set_off=[]) == "merge_host: set_off needs nsets + 1 entries"


# ---- the database that cannot be opened -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def broken(db_path):
    """(no .igd at all, an .igd without its _index.tsv, an .igd cut short of its records)"""
    d = short_tmpdir("iab")
    tsv = os.path.splitext(db_path)[0] + "_index.tsv"
    no_index, cut = os.path.join(d, "noindex.igd"), os.path.join(d, "cut.igd")
    shutil.copy(db_path, no_index)
    shutil.copy(tsv, os.path.join(d, "cut_index.tsv"))
    with open(db_path, "rb") as f:
        data = f.read()
    with open(cut, "wb") as f:
        f.write(data[:-8])
    yield os.path.join(d, "absent.igd"), no_index, cut
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("name", WITH_PATH)
def test_a_database_that_cannot_be_opened(db_path, broken, name):
    absent, no_index, cut = broken
    assert refused(name, db_path, igd_path=absent) == "cannot read .igd header of %s" % absent
    assert refused(name, db_path, igd_path=no_index) == "cannot read the _index.tsv next to %s" % no_index
    want = "cannot map %s" % cut if name in BY_HAND else "%s: cannot map %s" % (name, cut)
    assert refused(name, db_path, igd_path=cut) == want
    call(name, db_path)


def flat(r):
    """the arrays and numbers of a result, nested tuples opened"""
    if isinstance(r, tuple):
        return [x for part in r for x in flat(part)]
    return [np.asarray(r)]


def test_results_do_not_depend_on_a_refusal_before_them(db_path):
    for name in BY_HAND:
        first = call(name, db_path)
        refused(name, db_path, qe=[300, 5100])
        again = call(name, db_path)
        assert len(flat(first)) == len(flat(again)) > 1
        assert all(a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f") for a, b in zip(flat(first), flat(again)))
