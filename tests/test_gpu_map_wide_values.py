"""GPU: the wide form of igd_map_rows on signed values, and every lane of a load folding into one cell in both forms.

The wide form (more files than the op's LDS limit: SUM 1 365, MIN / MAX 2 048, COUNT 4 096) folds with global 64-bit atomics --
add, signed minimum, signed maximum -- on sign-extended values.  On the values 0, 400 and 1000 of sparse_lists an unsigned
minimum, a zero-extended value or a sum that only holds below 2^32 give the right answer; on map_ref.placed_db's negative values,
INT32_MIN, INT32_MAX and three times INT32_MAX under one region they do not.  placed_db(pad_to = n) is those six files padded to n
with files of one negative record each; crowd = True adds a file of 300 records in one tile, whose loads put all 64 lanes into one
(region, file) cell: the LDS atomics at 7 files, the global ones at 2 049 and 4 097.

Everything goes through test_gpu_map.check: the rows against map_ref.ref_rows (a numpy broadcast over the lists this test wrote)
and against the host route, the set statistics against map_ref.ref_sets; outputs are handed over full of 0x5a."""
import shutil

import numpy as np
import pytest

from helpers import short_tmpdir
from map_ref import CROWD_RECORDS, I32_MAX, I32_MIN, OPS, crowd_regions, placed_db, placed_regions
from test_gpu_map import check, lds_files

pytestmark = pytest.mark.gpu
NBP = 1 << 14
CROWD = 6                                                                 # the crowd file's number


@pytest.fixture(scope="module")
def dbs():
    """{files: (ListDb, Database)}: placed_db with the crowd file, padded to `files`; written and opened once per module"""
    from igd_amd import Database
    d = short_tmpdir("igw")
    made = {}

    def get(nfiles):
        if nfiles not in made:
            ldb = placed_db(d, NBP, "wp%d" % nfiles, pad_to=nfiles, crowd=True)
            made[nfiles] = (ldb, Database(ldb.path))
            assert made[nfiles][1].nfiles == nfiles == ldb.nfiles
        return made[nfiles]
    yield get
    for _, db in made.values():
        db.close()
    shutil.rmtree(d, ignore_errors=True)


def test_the_default_placed_db_is_what_it_was(dbs):
    """pad_to = None, crowd = False: the six files of the placed cases, byte for byte -- and the same six lists lead every padded
    database"""
    d = short_tmpdir("igv")
    try:
        a, b = placed_db(d, NBP, "a"), placed_db(d, NBP, "b", pad_to=None, crowd=False)
        assert a.nfiles == 6 and a.files == b.files and open(a.path, "rb").read() == open(b.path, "rb").read()
        assert dbs(7)[0].files[:6] == a.files and placed_db(d, NBP, "c", pad_to=9).files[:6] == a.files
    finally:
        shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("nfiles", [1366, 2049, 4097])
def test_placed_cases_in_the_wide_form(nfiles, dbs):
    """just over the SUM limit, the MIN / MAX limit and the COUNT limit: negative values, INT32_MIN and INT32_MAX under one region,
    a sum of three times INT32_MAX, and the padding's negative records under the seven-tile region"""
    assert lds_files() == {"count": 4096, "min": 2048, "max": 2048, "sum": 1365}
    ldb, db = dbs(nfiles)
    (ichr, qs, qe), _ = placed_regions(NBP)
    for op in OPS:
        for v in (None, 500):
            want, wagg = check(db, ldb, ichr, qs, qe, op, v)
            if v is None:
                # the seven-tile region catches some of the padding and not all of it; nothing else does
                pad = want[:, 7:]
                assert 0 < pad[0].sum() < nfiles - 7 and not pad[1:].any() and (op == "count" or (wagg[0, 7:] <= 0).all())
                assert op == "count" or (wagg[0, 7:] < 0).any()
            else:
                assert not want[:, 7:].any()
    # what the wide form must keep: the sign, the ends of int32 and a sum past 32 bits
    c, s = db.map_values(ichr, qs, qe, "sum")
    assert s[4, 2] == -1 and s[5, 2] == I32_MIN and s[6, 3] == 3 * I32_MAX and s[3, 2] == -902 and c[6, 3] == 3
    assert db.map_values(ichr, qs, qe, "min")[1][4, 2] == I32_MIN and db.map_values(ichr, qs, qe, "max")[1][4, 2] == I32_MAX
    assert db.map_values(ichr, qs, qe, "max")[1][3, 2] == 3 and db.map_values(ichr, qs, qe, "min")[1][3, 2] == -900


@pytest.mark.parametrize("nfiles", [7, 2049, 4097])
def test_every_lane_of_a_load_folds_into_one_cell(nfiles, dbs):
    """300 records of one file in one tile under one region: ds_add_u64 / ds_min_i32 / ds_max_i32 and ds_add_u32 at 7 files, the
    global 64-bit atomics at 2 049 and 4 097"""
    ldb, db = dbs(nfiles)
    (ichr, qs, qe), counts = crowd_regions(NBP)
    assert counts == [CROWD_RECORDS, 128, 60, 120]
    n_max = [sum(1 for k in range(n) if k % 5 in (0, 3, 4)) for n in (CROWD_RECORDS, 128)]
    for op in OPS:
        want, wagg = check(db, ldb, ichr, qs, qe, op)
        assert want[:, CROWD].tolist() == counts and not np.delete(want, CROWD, axis=1).any(), op
        vwant, vagg = check(db, ldb, ichr, qs, qe, op, 500)
        assert vwant[:, CROWD].tolist() == n_max + [0, 0], op             # only the records of INT32_MAX remain
        a, va = wagg[:, CROWD].tolist(), vagg[:, CROWD].tolist()
        if op == "sum":
            assert a == [180 * I32_MAX + 60 * I32_MIN - 420, 76 * I32_MAX + 26 * I32_MIN - 26 * 7, -420, 60 * I32_MIN - 420]
            assert a[0] > 2 ** 37 and a[3] < -2 ** 36 and va == [180 * I32_MAX, 76 * I32_MAX, 0, 0]
        elif op == "min":
            assert a == [I32_MIN, I32_MIN, -7, I32_MIN] and va == [I32_MAX, I32_MAX, 0, 0]
        elif op == "max":
            assert a == [I32_MAX, I32_MAX, -7, -7] and va == [I32_MAX, I32_MAX, 0, 0]
        else:
            assert a == counts
    # the region over all of int32 of the placed cases takes the crowd as well
    (pc, ps, pe), _ = placed_regions(NBP)
    for op in ("sum", "min"):
        want, _ = check(db, ldb, pc[14:15], ps[14:15], pe[14:15], op, host=False)
        assert want[0, CROWD] == CROWD_RECORDS
