"""What every Database method that takes regions, sets or a caller's output array refuses before it launches, and with which
words -- tests/test_database_args_host.py's table, on the device entries of igd_amd/database.py.

One module-scoped Database on the tiny database of the host test (one contig, three files), three regions in two sets.  Every
refusal is an IgdError whose text starts with the name of the entry that checks (support() and coverage() are rows of
support_sets() and coverage_sets(), which speak), and the handle serves the next call.  A caller's output array of the wrong
dtype, the wrong shape or not in C order is refused with a text that names the array and the shape; a right one is the very
object that comes back.  No regions and no sets are legal everywhere: those calls hand NULL pointers to the engine.

Database.search, enumerate* and seqpare never compared the lengths of ichr, qs and qe, and search never looked at a caller's
`hits`: they have no row here."""
import random
import shutil

import numpy as np
import pytest

from helpers import short_tmpdir
from sets_fixtures import NBP, wide_db
from test_database_args_host import BAD, CTG, REGIONS, SETS, UNIVERSE

pytestmark = pytest.mark.gpu

NF = 3
# method -> (the name its refusals start with, the good keyword arguments, the features that have a bad value)
DEVICE = {
    "search_sets": ("search_sets", {**REGIONS, **SETS}, ("qe", "sets", "min_overlap")),
    "support_sets": ("support_sets", {**REGIONS, **SETS}, ("qe", "sets", "min_overlap")),
    "support": ("support_sets", {**REGIONS}, ("qe", "min_overlap")),
    "coverage_sets": ("coverage_sets", {**REGIONS, **SETS}, ("qe", "sets")),
    "coverage": ("coverage_sets", {**REGIONS}, ("qe",)),
    "enrichment_sets": ("enrichment_sets", {**REGIONS, **SETS, **UNIVERSE}, ("qe", "sets", "universe", "min_overlap")),
    "restrict_sets": ("restrict_sets", {**REGIONS, **SETS, **UNIVERSE}, ("qe", "sets", "universe")),
    "enrichment_restricted": ("enrichment_restricted", {**REGIONS, **SETS, **UNIVERSE}, ("qe", "sets", "universe")),
    "membership": ("membership", {**REGIONS}, ("qe",)),
    "cooccurrence": ("cooccurrence", {**REGIONS}, ("qe",)),
    "permutation_support": ("permutation_support", {**REGIONS, **CTG, "nperm": 2}, ("qe", "ctg_len", "mode", "min_overlap")),
    "permute_regions": ("permute_regions", {**REGIONS, **CTG, "p0": 0, "np_": 2}, ("qe", "mode")),
    "nearest": ("nearest", {**REGIONS, "window": 1000}, ("qe", "window")),
    "nearest_sets": ("nearest_sets", {**REGIONS, **SETS, "window": 1000}, ("qe", "sets", "window")),
    "nearest_sets_fused": ("nearest_sets_fused", {**REGIONS, **SETS, "window": 1000}, ("qe", "sets", "window")),
    "permutation_nearest": ("permutation_nearest", {**REGIONS, **CTG, "nperm": 2, "window": 1000}, ("qe", "ctg_len", "mode", "window")),
    "nearest_signed": ("nearest_signed", {**REGIONS, "window": 1000}, ("qe", "window")),
    "nearest_hist": ("nearest_hist", {**REGIONS, **SETS, "window": 1000, "edges": [-10, 0, 10]}, ("qe", "sets", "window", "edges")),
    "flanks": ("flanks", {**REGIONS, "window": 1000}, ("qe", "window", "measure")),
    "flank_reldist": ("flank_reldist", {**REGIONS, **SETS, "window": 1000, "nbins": 4}, ("qe", "sets", "window", "measure", "nbins")),
    "merge_sets": ("merge_sets", {**REGIONS, **SETS}, ("qe", "sets", "gap")),
    "jaccard_sets": ("jaccard_sets", {**REGIONS, **SETS}, ("qe", "sets")),
    "permutation_bp": ("permutation_bp", {**REGIONS, **CTG, "nperm": 2}, ("qe", "ctg_len", "mode")),
    "map_values": ("map_values", {**REGIONS}, ("qe", "op")),
    "map_sets": ("map_sets", {**REGIONS, **SETS}, ("qe", "sets", "op")),
}
CASES = [(name, case, over, text) for name, (_, _, feats) in DEVICE.items() for f in feats for case, over, text in BAD[f]]
UNCHECKED = {"search", "enumerate", "enumerate_stream", "enumerate_stream8", "seqpare"}


@pytest.fixture(scope="module")
def db():
    from igd_amd import Database
    d = short_tmpdir("iad")
    path, span, _, _ = wide_db(random.Random(4100), d, "tiny", NF, NBP, 4)
    assert span > max(REGIONS["qe"])
    with Database(path) as handle:
        assert handle.nfiles == NF and handle.nctg == 1 and handle.member_words == 1
        yield handle
    shutil.rmtree(d, ignore_errors=True)


def refused(db, name, **kw):
    from igd_amd.database import IgdError
    with pytest.raises(IgdError) as e:
        getattr(db, name)(**kw)
    return str(e.value)


def test_the_table_names_every_method_that_takes_regions():
    import inspect
    from igd_amd import Database
    takes = {n for n, f in inspect.getmembers(Database, inspect.isfunction)
             if not n.startswith("_") and {"ichr", "qs", "qe"} <= set(inspect.signature(f).parameters)}
    assert takes == set(DEVICE) | UNCHECKED


@pytest.mark.parametrize("name,case,over,text", CASES, ids=["%s-%s" % c[:2] for c in CASES])
def test_one_bad_argument_is_refused_under_the_entrys_name(db, name, case, over, text):
    prefix, kw, _ = DEVICE[name]
    got = refused(db, name, **{**kw, **over})
    assert got.startswith(prefix + ": ") and text in got, got
    assert refused(db, name, **{**kw, **over}) == got
    getattr(db, name)(**kw)                                        # and the handle serves the next good call


def test_the_set_texts_in_full(db):
    """the noun is the entry's own: queries where the sets are searched, regions where they are measured"""
    short = dict(qe=[300, 5100])
    assert refused(db, "search_sets", **{**REGIONS, **SETS, **short}) == "search_sets: set_off[-1] = 3, but 3 / 3 / 2 queries given"
    assert refused(db, "coverage", **{**REGIONS, **short}) == "coverage_sets: set_off[-1] = 3, but 3 / 3 / 2 queries given"
    assert refused(db, "enrichment_sets", **{**REGIONS, **SETS, **UNIVERSE, "set_off": [0, 2, 4]}) == \
        "enrichment_sets: set_off[-1] = 4, but 3 / 3 / 3 queries and 2 / 2 / 2 universe regions given"
    assert refused(db, "restrict_sets", **{**REGIONS, **SETS, **UNIVERSE, "u_qe": [6000]}) == \
        "restrict_sets: set_off[-1] = 3, but 3 / 3 / 3 queries and 2 / 2 / 1 universe regions given"
    assert refused(db, "nearest_hist", **{**REGIONS, **SETS, **short, "window": 9, "edges": [0]}) == \
        "nearest_hist: set_off[-1] = 3, but 3 / 3 / 2 regions given"
    assert refused(db, "membership", **{**REGIONS, **short}) == "membership: 3 / 3 / 2 queries given"
    assert refused(db, "cooccurrence", **{**REGIONS, **short}) == "cooccurrence: 3 / 3 / 2 regions given"
    assert refused(db, "permutation_bp", **{**REGIONS, "ctg_len": [[200000]], "nperm": 1}) == "permutation_bp: 3 / 3 / 3 regions given"
    assert refused(db, "jaccard_sets", **{**REGIONS, "set_off": []}) == "jaccard_sets: set_off needs nsets + 1 entries"


# ---- a caller's output arrays -----------------------------------------------------------------------------------------------
ROWS = dict(a=np.array([[1], [3]], np.uint32), b=np.array([[1], [2], [7]], np.uint32))
TABLES = dict(a=[1, 2], b=[3, 4], c=[5, 6], d=[7, 8])
# (method, the good keyword arguments, the output's keyword, how many arrays it is, dtype, shape, the words between "must be" and the dtype)
OUTPUTS = [
    ("search_sets", {**REGIONS, **SETS}, "hits", 1, np.int64, (2, NF), "a C-ordered"),
    ("support_sets", {**REGIONS, **SETS}, "support", 1, np.int64, (2, NF), "a C-ordered"),
    ("coverage_sets", {**REGIONS, **SETS}, "coverage", 1, np.int64, (2, NF), "a C-ordered"),
    ("fisher", TABLES, "pvalue_log", 1, np.float64, (2,), "a contiguous"),
    ("fisher", TABLES, "odds_ratio", 1, np.float64, (2,), "a contiguous"),
    ("membership", {**REGIONS}, "bits", 1, np.uint32, (3, 1), "a C-ordered"),
    ("cooccurrence", {**REGIONS}, "cooc", 1, np.int64, (NF, NF), "a C-ordered"),
    ("transpose_bits", dict(bits=ROWS["b"]), "cols", 1, np.uint64, (32, 1), "a C-ordered"),
    ("bitrows_gram", ROWS, "out", 1, np.int64, (2, 3), "a C-ordered"),
    ("perm_stats", dict(rows=[[1, 2], [3, 4], [5, 6]], observed=[3, 3]), "out", 6, np.int64, (2,), "six C-ordered"),
    ("nearest", {**REGIONS, "window": 1000}, "dist", 1, np.int32, (3, NF), "a C-ordered"),
    ("nearest_sets", {**REGIONS, **SETS, "window": 1000}, "out", 3, np.int64, (2, NF + 1), "three C-ordered"),
    ("nearest_sets_fused", {**REGIONS, **SETS, "window": 1000}, "out", 3, np.int64, (2, NF + 1), "three C-ordered"),
    ("permutation_nearest", {**REGIONS, **CTG, "nperm": 2, "window": 1000}, "out", 3, np.int64, (3, NF + 1), "three C-ordered"),
    ("nearest_signed", {**REGIONS, "window": 1000}, "sdist", 1, np.int32, (3, NF), "a C-ordered"),
    ("nearest_hist", {**REGIONS, **SETS, "window": 1000, "edges": [-10, 0, 10]}, "hist", 1, np.int64, (2, 4, NF + 1), "a C-ordered"),
    ("flanks", {**REGIONS, "window": 1000}, "up", 1, np.int32, (3, NF), "a C-ordered"),
    ("flanks", {**REGIONS, "window": 1000}, "down", 1, np.int32, (3, NF), "a C-ordered"),
    ("flank_reldist", {**REGIONS, **SETS, "window": 1000, "nbins": 4}, "hist", 1, np.int64, (2, 4, NF + 1), "a C-ordered"),
    ("map_values", {**REGIONS}, "count", 1, np.int32, (3, NF), "a C-ordered"),
    ("map_values", {**REGIONS}, "agg", 1, np.int64, (3, NF), "a C-ordered"),
    ("map_sets", {**REGIONS, **SETS}, "out", 3, np.int64, (2, NF), "three C-ordered"),
]


def not_c_ordered(shape, dtype):
    """an array of this shape and dtype that is not C-contiguous: Fortran order where that differs, every second word otherwise"""
    a = np.asfortranarray(np.zeros(shape, dtype))
    if a.flags.c_contiguous:
        a = np.zeros(tuple(2 * n for n in shape), dtype)[tuple(slice(None, None, 2) for _ in shape)]
    assert a.shape == shape and a.dtype == dtype and not a.flags.c_contiguous
    return a


def test_the_table_names_every_output_a_caller_can_give():
    import inspect
    from igd_amd import Database
    names = {o[2] for o in OUTPUTS}
    inputs = {("enrichment_ranks", "support"), ("enrichment_ranks", "pvalue_log"), ("enrichment_ranks", "odds_ratio"), ("transpose_bits", "bits"),
              ("unpack_membership", "bits"), ("unpack_restricted", "bits"), ("expand_hit8", "bits")}
    takes = {(n, p) for n, f in inspect.getmembers(Database, inspect.isfunction) if not n.startswith("_") and not n.endswith("_dev")
             for p in inspect.signature(f).parameters if p in names}
    assert takes - inputs - {("search", "hits")} == {(o[0], o[2]) for o in OUTPUTS}


@pytest.mark.parametrize("name,kw,key,count,dtype,shape,words", OUTPUTS, ids=["%s-%s" % (o[0], o[2]) for o in OUTPUTS])
def test_a_callers_output_array(db, name, kw, key, count, dtype, shape, words):
    other = np.int32 if dtype != np.int32 else np.int64
    wrong = {"dtype": np.zeros(shape, other), "shape": np.zeros(shape + (1,), dtype), "order": not_c_ordered(shape, dtype)}
    text = "%s: %s must be %s %s[%s]" % (name, key, words, np.dtype(dtype).name, ", ".join("%d" % n for n in shape))
    for what, arr in wrong.items():
        given = arr if count == 1 else [np.zeros(shape, dtype) for _ in range(count - 1)] + [arr]
        assert refused(db, name, **kw, **{key: given}) == text, what
    if count > 1:
        assert refused(db, name, **kw, **{key: [np.zeros(shape, dtype) for _ in range(count - 1)]}) == text
    fresh = getattr(db, name)(**kw)
    mine = np.full(shape, 0x5a, dtype) if count == 1 else [np.full(shape, 0x5a, dtype) for _ in range(count)]
    if key in ("hits", "support", "coverage"):                     # (these three are added to)
        mine[...] = 0
    got = getattr(db, name)(**kw, **{key: mine})
    fresh, got = (r if isinstance(r, tuple) else (r,) for r in (fresh, got))
    parts = [mine] if count == 1 else mine
    assert sum(any(x is p for x in got) for p in parts) == count, "the caller's array is not the one returned"
    for x, y in zip(fresh, got):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")


# ---- no regions, no sets ----------------------------------------------------------------------------------------------------
EMPTY = dict(ichr=[], qs=[], qe=[])
SET_ENTRIES = [n for n, (_, kw, _) in DEVICE.items() if "set_off" in kw]


@pytest.mark.parametrize("name", SET_ENTRIES)
@pytest.mark.parametrize("set_off", ([0], [0, 0, 0]), ids=["no_sets", "two_empty_sets"])
def test_no_regions_and_no_sets(db, name, set_off):
    kw = {**DEVICE[name][1], **EMPTY, "set_off": set_off}
    nsets = len(set_off) - 1
    got = getattr(db, name)(**kw)
    first = got[0]
    assert isinstance(first, np.ndarray) and first.shape[0] == (0 if name == "merge_sets" else nsets), (name, first.shape)
    if name in ("search_sets", "support_sets", "coverage_sets"):
        assert first.shape == (nsets, NF) and not first.any() and got[1].shape == (nsets,) and not got[1].any()
    if name == "merge_sets":
        assert np.array_equal(got[3], np.zeros(nsets + 1, np.int64)) and got[5].shape == (nsets,)
    getattr(db, name)(**DEVICE[name][1])


@pytest.mark.parametrize("name", [n for n in DEVICE if n not in SET_ENTRIES])
def test_no_regions(db, name):
    got = getattr(db, name)(**{**DEVICE[name][1], **EMPTY})
    assert got is not None
    getattr(db, name)(**DEVICE[name][1])
