"""`igd search <db> -Q <list>`: one query set per listed file, each block the text `igd search <db> -q <file>` prints for that
file, headed by `Query set <k>: <file>`.  -Q applies only where the reference's own parse leaves nothing to do (no -q, -r,
-m, -s, -f): every other command line keeps its output byte for byte.

The unmarked tests run without a GPU: with a large IGD_HOST_MAX_QUERIES every set takes the host's `-q` route; with the
limit at 0 and no device the tool fails loudly.  The `gpu` tests send the sets through igd_hip_search_sets (the limit is 0
there), and the `ref` test holds each block against the reference binary's `-q` output."""
import glob
import os
import shutil
import subprocess

import pytest

from helpers import GOLDEN, ROOT, have_ref, run_ref, short_tmpdir, write_bed

EXE = os.path.join(ROOT, "bin", "igd")
HOST = {"IGD_HOST_MAX_QUERIES": "100000000"}


def _run(args, env=None, cwd=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, cwd=cwd, timeout=600)


def _case_files(case):
    return [os.path.join(GOLDEN, case, "q.bed")] + sorted(glob.glob(os.path.join(GOLDEN, case, "beds", "*.bed")))


def _write_list(d, files, name="list.txt", crlf=False):
    path = os.path.join(d, name)
    with open(path, "w", newline="") as f:
        for i, p in enumerate(files):
            f.write(p + ("\r\n" if crlf and i % 2 else "\n"))
            if i % 3 == 1:
                f.write("\n")                            # blank lines are skipped
    return path


def _expected(db, files, extra, env):
    out = b""
    for k, p in enumerate(files):
        r = _run(["search", db, "-q", p] + extra, env)
        assert r.returncode == 0, r.stderr
        out += b"Query set %d: %s\n" % (k, p.encode()) + r.stdout
    return out


@pytest.fixture
def tmp():
    d = short_tmpdir("iqs")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("case,extra", [("branch", []), ("branch", ["-v", "500"]), ("gtype0", []), ("gtype0", ["-v", "500"]),
                                        ("edge", [])])
def test_list_equals_the_q_blocks_on_the_host_route(case, extra, tmp):
    db = os.path.join(GOLDEN, case, "db.igd")
    files = _case_files(case)
    lst = _write_list(tmp, files, crlf=True)
    got = _run(["search", db, "-Q", lst] + extra, HOST)
    assert got.returncode == 0, got.stderr
    assert got.stdout == _expected(db, files, extra, HOST)
    assert got.stdout.count(b"Query set ") == len(files)


def test_empty_list_prints_nothing(tmp):
    lst = os.path.join(tmp, "l.txt")
    open(lst, "w").write("\n\n")
    got = _run(["search", os.path.join(GOLDEN, "branch", "db.igd"), "-Q", lst], HOST)
    assert got.returncode == 0 and got.stdout == b""


@pytest.mark.parametrize("other", [["-q", "Q"], ["-q", "Q", "-f"], ["-f"], ["-r", "chr1", "1000", "90000"],
                                   ["-r", "chr1", "1000", "90000", "-f"], ["-q", "Q", "-v", "300"]])
def test_other_command_lines_keep_their_output(other, tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    other = [q if a == "Q" else a for a in other]
    lst = _write_list(tmp, _case_files("branch"))
    want = _run(["search", db] + other, HOST)
    for args in (["-Q", lst] + other, other + ["-Q", lst]):
        got = _run(["search", db] + args, HOST)
        assert (got.returncode, got.stdout) == (want.returncode, want.stdout), args


def test_no_list_argument_prints_the_usage_as_before():
    db = os.path.join(GOLDEN, "branch", "db.igd")
    want = _run(["search", db, "-c"], HOST)
    got = _run(["search", db, "-Q"], HOST)
    assert (got.returncode, got.stdout, got.stderr) == (want.returncode, want.stdout, want.stderr)


def test_engine_route_without_a_device_fails_loudly(tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    lst = _write_list(tmp, _case_files("branch"))
    got = _run(["search", db, "-Q", lst], {"IGD_HOST_MAX_QUERIES": "0", "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"})
    assert got.returncode == 69 and b"no CPU search path" in got.stderr
    assert b"Total" not in got.stdout and b"index\t" not in got.stdout


# ---- engine route (igd_hip_search_sets) ----------------------------------------------------------------------------------
def _many_sets(d, n=12):
    """query files of several sizes: empty, one line, unknown contigs, out of order, and a missing entry"""
    import random
    rng = random.Random(77)
    files = []
    for k in range(n):
        p = os.path.join(d, "s%02d.bed" % k)
        rows = []
        for _ in range([0, 1, 5, 40, 300, 1500][k % 6]):
            c = rng.choice(["chr1", "chr2", "chr5", "chrUn"])
            s = rng.randrange(0, 400000)
            rows.append((c, s, s + rng.choice([1, 50, 3000, 40000])))
        write_bed(p, rows)
        files.append(p)
    files.insert(5, os.path.join(d, "missing.bed"))
    return files


@pytest.mark.gpu
@pytest.mark.parametrize("case,extra", [("branch", []), ("branch", ["-v", "500"]), ("gtype0", []), ("gtype0", ["-v", "500"])])
def test_list_equals_the_q_blocks_on_the_engine_route(case, extra, tmp):
    db = os.path.join(GOLDEN, case, "db.igd")
    files = _case_files(case) + _many_sets(tmp)
    lst = _write_list(tmp, files)
    got = _run(["search", db, "-Q", lst] + extra)
    assert got.returncode == 0, got.stderr
    assert got.stdout == _expected(db, files, extra, None)


@pytest.mark.gpu
def test_hit_map_and_seqpare_command_lines_keep_their_output(tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    lst = _write_list(tmp, _case_files("branch"))
    for other in (["-m", "-o", "hm"], ["-q", q, "-s"]):
        want = _run(["search", db] + other, cwd=tmp)
        want_file = open(os.path.join(tmp, "hm"), "rb").read() if other[0] == "-m" else None
        got = _run(["search", db, "-Q", lst] + other, cwd=tmp)
        assert (got.returncode, got.stdout) == (want.returncode, want.stdout), other
        if want_file is not None:
            assert open(os.path.join(tmp, "hm"), "rb").read() == want_file


@pytest.mark.gpu
@pytest.mark.ref
@pytest.mark.parametrize("case,extra", [("branch", []), ("branch", ["-v", "500"]), ("gtype0", [])])
def test_each_block_equals_the_reference(case, extra, tmp):
    if not have_ref():
        pytest.skip("no reference binary")
    shutil.copy(os.path.join(GOLDEN, case, "db.igd"), os.path.join(tmp, "db.igd"))
    shutil.copy(os.path.join(GOLDEN, case, "db_index.tsv"), os.path.join(tmp, "db_index.tsv"))
    files = []
    for k, p in enumerate(_case_files(case)):
        files.append(os.path.join(tmp, "q%d.bed" % k))
        shutil.copy(p, files[-1])
    lst = _write_list(tmp, files)
    got = _run(["search", os.path.join(tmp, "db.igd"), "-Q", lst] + extra)
    assert got.returncode == 0, got.stderr
    want = "".join("Query set %d: %s\n" % (k, p) + run_ref(["search", os.path.join(tmp, "db.igd"), "-q", p] + extra)
                   for k, p in enumerate(files))
    assert got.stdout.decode() == want
