"""igd_search() is exported by libigd.so (include/igd_search.h), so a refused command line must leave the process as it found it:
every way out after get_igdinfo() passes the one release block.  Host sanitizers on a stand-alone program (its own main,
nothing loaded into Python, nothing preloaded); no GPU: the host limit is raised, the accepted command is counted on the host."""
import os
import shutil
import subprocess

from helpers import GOLDEN, ROOT, short_tmpdir
from test_hostpath_io_host import SAN, SAN_ENV


def test_refused_and_accepted_searches_in_one_process_leak_nothing():
    """tests/c/cli_san_main.c calls igd_search() six times on a copy of the smallrand database: a newer refusal, an older one,
    a refused -Z (its offsets parsed), a refused -K (its file read), an accepted -q -u, the first refusal again.  Under
    ASan + UBSan with leak detection nothing is reported, every call returns its exit code, and the accepted call prints the
    table of bin/igd.  (Before the single release block every refusal leaked the 88 bytes of the hits array and left the
    database tables behind for the next call to overwrite.)"""
    d = short_tmpdir("igcs")
    try:
        exe = os.path.join(d, "cli_san")
        csrc = ["igd_amd/csrc/" + f for f in ("igd_cli_abi.c", "igd_core.c", "igd_hostpath.c", "igd_create.c", "igd_hip_lazy.c")]
        subprocess.check_call(["gcc", "-std=gnu99", *SAN, "-Iinclude", "-Iigd_amd/csrc", "-o", exe, "tests/c/cli_san_main.c", *csrc,
                               "-lz", "-lm", "-lpthread", "-ldl"], cwd=ROOT)
        for f in ("db.igd", "db_index.tsv", "q.bed"):
            shutil.copy(os.path.join(GOLDEN, "smallrand", f), os.path.join(d, f))
        with open(os.path.join(d, "genome"), "w") as g:
            g.writelines("chr%s\t300000000\n" % c for c in [*range(1, 23), "X", "Y"])
        open(os.path.join(d, "groups"), "w").close()
        env = dict({k: v for k, v in SAN_ENV.items() if not k.startswith("IGD_")}, IGD_HOST_MAX_QUERIES="100000000")
        p = subprocess.run([exe, d], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        err = p.stderr.decode(errors="replace")
        assert "Sanitizer" not in err and "runtime error" not in err and p.returncode == 0, (p.returncode, err[-3000:])
        calls = p.stdout.split(b"== ")[1:]
        assert [c.split(b"\n", 1)[0] for c in calls] == [b"0", b"1", b"2", b"3", b"4", b"5"]
        want = subprocess.run([os.path.join(ROOT, "bin", "igd"), "search", "db.igd", "-q", "q.bed", "-u"], cwd=d, env=env,
                              stdout=subprocess.PIPE, check=True).stdout
        assert want.count(b"\n") > 5 and calls[4].split(b"\n", 1)[1] == want
        assert calls[0] == calls[5].replace(b"5\n", b"0\n", 1) and b"Not supported: -H without -N" in calls[0]
    finally:
        shutil.rmtree(d, ignore_errors=True)
