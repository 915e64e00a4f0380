"""`igd search db.igd -q regions.bed -g genome.sizes -Z W,STEP [-v N] [-O/-A/-B] [-P N [-S seed] [-M mode | -W ws.bed]]` on the
host route.

Without -P: the header `index<TAB>File<TAB>shift_<d>..`, one line per dataset with the integer supports, then a line `any<TAB>-`.
With -P N: observed, mean and sd of -P's null in front, every shift as a z-score (%.4f, or NA).  Expected text never comes from
the code under test: shift_ref's explicit lists through igd_amd.support_host, the null from permute_ref's lists through
igdc_support_host and numpy.  Every refusal exits 64 with nothing on stdout."""
import os

import numpy as np
import pytest

import permute_ref as PR
import shift_ref as SR
from test_permute_cli import NBP, fx  # noqa: F401  (the command line fixture: database, BED file, genome file)
from test_permute_host import reference_rows
from test_shift_host import reference_rows as shifted_rows
from test_support_host import HOST, HostDb, _index, _run, cli_rule


def names(fx):  # noqa: F811
    return [name for _, name in _index(fx["db"])] + ["-"]


def plain_text(fx, window, step, **kw):  # noqa: F811
    off = SR.offsets(window, step)
    ichr, qs, qe = fx["regions"]
    rows = shifted_rows(fx["db"], ichr, qs, qe, fx["ctg_len"], off, **kw)
    out = ["index\tFile" + "".join("\tshift_%d" % d for d in off) + "\n"]
    nm = names(fx)
    for f in range(len(nm)):
        out.append("%s\t%s" % (f if f < len(nm) - 1 else "any", nm[f]) + "".join("\t%d" % x for x in rows[:, f]) + "\n")
    return "".join(out), rows


def z_text(fx, window, step, nperm, seed, mode, v):  # noqa: F811
    off = SR.offsets(window, step)
    ichr, qs, qe = fx["regions"]
    H = HostDb(fx["db"])
    try:
        rule, ev = cli_rule(1, v)
        obs, null = reference_rows(H, ichr, qs, qe, fx["ctg_len"], nperm, seed, mode, ev, rule)
    finally:
        H.close()
    rows = shifted_rows(fx["db"], ichr, qs, qe, fx["ctg_len"], off, v=v)
    mean, sd = PR.summary(null, obs)[:2]
    z = SR.zscore(rows, null)
    out = ["index\tFile\tobserved\tmean\tsd" + "".join("\tshift_%d" % d for d in off) + "\n"]
    nm = names(fx)
    for f in range(len(nm)):
        line = "%s\t%s\t%d\t%.6f\t%s" % (f if f < len(nm) - 1 else "any", nm[f], obs[f], mean[f], "NA" if np.isnan(sd[f]) else "%.6f" % sd[f])
        out.append(line + "".join("\tNA" if np.isnan(x) else "\t%.4f" % x for x in z[:, f]) + "\n")
    return "".join(out), z


@pytest.mark.parametrize("arg,window,step,extra,kw", [("300,100", 300, 100, [], {}), ("5000,2500", 5000, 2500, ["-v", "500"], dict(v=500)),
                                                     ("99,100", 99, 100, [], {}), ("0,1", 0, 1, [], {}),
                                                     ("1073741824,1073741824", 2 ** 30, 2 ** 30, ["-O", "40"], dict(min_overlap=40))])
def test_cli_Z_prints_the_reference_table_on_the_host_route(fx, arg, window, step, extra, kw):  # noqa: F811
    want, rows = plain_text(fx, window, step, **kw)
    for args in (["-q", fx["q"], "-g", fx["g"], "-Z", arg] + extra, extra + ["-Z", arg, "-g", fx["g"], "-q", fx["q"]]):
        got = _run(["search", fx["db"]] + args, HOST)
        assert got.returncode == 0, got.stderr
        assert got.stdout.decode() == want, args
    assert rows[:, :-1].any() and want.count("\n") == 7 + 2
    if window == 300:
        assert (rows[0] != rows[3]).any() and (rows[3] != rows[6]).any()       # the table depends on the shift
        # the middle column is -u's
        u = _run(["search", fx["db"], "-q", fx["q"], "-u"], HOST).stdout.decode().splitlines()
        sup = {int(l.split("\t")[0]): int(l.split("\t")[2]) for l in u[1:-1]}
        assert {f: int(rows[3, f]) for f in range(7) if rows[3, f]} == sup


@pytest.mark.parametrize("extra,nperm,seed,mode,v", [([], 7, 0, PR.CIRCULAR, 0), (["-S", "5", "-M", "shuffle"], 20, 5, PR.SHUFFLE, 0),
                                                    (["-v", "500"], 3, 0, PR.CIRCULAR, 500), ([], 1, 0, PR.CIRCULAR, 0)])
def test_cli_Z_with_P_prints_z_scores_in_the_null_of_P(fx, extra, nperm, seed, mode, v):  # noqa: F811
    want, z = z_text(fx, 2 * NBP, NBP, nperm, seed, mode, v)
    got = _run(["search", fx["db"], "-q", fx["q"], "-g", fx["g"], "-Z", "%d,%d" % (2 * NBP, NBP), "-P", str(nperm)] + extra, HOST)
    assert got.returncode == 0, got.stderr
    assert got.stdout.decode() == want
    if nperm == 1:
        assert np.isnan(z).all() and "\tNA\tNA\tNA\tNA\tNA\tNA\n" in want
    else:
        assert not np.isnan(z[:, :-1]).all()


def test_cli_Z_with_P_inside_a_workspace_runs(fx):  # noqa: F811
    w = os.path.join(fx["d"], "zws.bed")
    with open(w, "w") as f:
        f.write("chr1\t0\t%d\nchr2\t0\t%d\n" % (fx["ctg_len"][0], fx["ctg_len"][1]))
    got = _run(["search", fx["db"], "-q", fx["q"], "-g", fx["g"], "-Z", "200,100", "-P", "9", "-W", w, "-S", "3"], HOST)
    assert got.returncode == 0, got.stderr
    lines = got.stdout.decode().splitlines()
    assert lines[0] == "index\tFile\tobserved\tmean\tsd\tshift_-200\tshift_-100\tshift_0\tshift_100\tshift_200" and len(lines) == 7 + 2 and lines[-1].startswith("any\t-\t")
    # the whole contigs as the workspace: -M shuffle's placement, so the same null
    want = _run(["search", fx["db"], "-q", fx["q"], "-g", fx["g"], "-Z", "200,100", "-P", "9", "-M", "shuffle", "-S", "3"], HOST)
    assert want.returncode == 0 and want.stdout == got.stdout


REFUSALS = [["-Z", "100,0"], ["-Z", "100,-5"], ["-Z", "-100,5"], ["-Z", "100"], ["-Z", "100,"], ["-Z", ",5"], ["-Z", "a,b"], ["-Z", "100,5x"],
            ["-Z", "2048,1"], ["-Z", "1073741825,1073741825"], ["-Z"],
            ["-Z", "100,50", "-u"], ["-Z", "100,50", "-U", "Q"], ["-Z", "100,50", "-b"], ["-Z", "100,50", "-J"], ["-Z", "100,50", "-w"],
            ["-Z", "100,50", "-C"], ["-Z", "100,50", "-N", "500"], ["-Z", "100,50", "-V", "count"], ["-Z", "100,50", "-K", "Q"],
            ["-Z", "100,50", "-m"], ["-Z", "100,50", "-s"], ["-Z", "100,50", "-r", "chr1", "1000", "90000"], ["-Z", "100,50", "-f"],
            ["-Z", "100,50", "-Q", "Q"], ["-Z", "100,50", "-P", "5", "-D", "700"], ["-Z", "100,50", "-P", "5", "-G"],
            ["-Z", "100,50", "-D", "700"], ["-Z", "100,50", "-G"], ["-Z", "100,50", "-P", "0"], ["-Z", "100,50", "-P", "5", "-M", "rigid"],
            ["-Z", "100,50", "-S", "4"]]


@pytest.mark.parametrize("extra", REFUSALS, ids=lambda e: "_".join(e))
def test_every_refusal_exits_64_with_nothing_on_stdout(fx, extra):  # noqa: F811
    extra = [fx["q"] if a == "Q" else a for a in extra]
    for args in (["-q", fx["q"], "-g", fx["g"]] + extra, extra + ["-g", fx["g"], "-q", fx["q"]]):
        if extra == ["-Z"] and args[0] == "-Z":
            continue                                         # ("-Z -g": -g is then the argument, refused as a W,STEP)
        got = _run(["search", fx["db"]] + args, HOST)
        assert got.returncode == 64 and got.stdout == b"" and got.stderr.startswith(b"Not supported: "), (args, got.stdout, got.stderr)


def test_Z_without_g_or_q_is_refused_and_the_other_command_lines_keep_their_output(fx):  # noqa: F811
    for args in (["-q", fx["q"], "-Z", "100,50"], ["-g", fx["g"], "-Z", "100,50"]):
        got = _run(["search", fx["db"]] + args, HOST)
        assert got.returncode == 64 and got.stdout == b"" and b"-Z without -" in got.stderr
    # 4096 shifts would be one too many for 2 k + 1; 4095 run
    got = _run(["search", fx["db"], "-q", fx["q"], "-g", fx["g"], "-Z", "2047,1"], HOST)
    assert got.returncode == 0 and got.stdout.decode().splitlines()[0].count("\tshift_") == 4095
    # -g without -P and without -Z keeps its refusal, -P keeps its table
    assert _run(["search", fx["db"], "-q", fx["q"], "-g", fx["g"]], HOST).stdout == b"Not supported: -g, -S or -M without -P\n"
    assert _run(["search", fx["db"], "-q", fx["q"], "-g", fx["g"], "-P", "3"], HOST).stdout.startswith(b"index\tobserved\tmean\t")
    usage = _run(["search"], HOST).stderr.decode()
    assert "    -Z <W>,<STEP>" in usage


def test_a_region_outside_its_contig_names_the_line(fx):  # noqa: F811
    from helpers import write_bed
    L0 = int(fx["ctg_len"][0])
    q = os.path.join(fx["d"], "zout.bed")
    write_bed(q, [("chr1", 5, 50), ("chr1", 100, L0 + 1)])
    got = _run(["search", fx["db"], "-q", q, "-g", fx["g"], "-Z", "100,50"], HOST)
    assert got.stdout.decode() == "%s, line 2: region chr1:100-%d does not lie on its contig of length %d\n" % (q, L0 + 1, L0)
