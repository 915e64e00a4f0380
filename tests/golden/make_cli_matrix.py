#!/usr/bin/env python3
"""Record tests/golden/cli_matrix.json: what `igd search` answers to every case of tests/cli_matrix_cases.py.

    make_cli_matrix.py <bin/igd of the PARENT commit, built in a checkout of its own>

The fixture pins the behaviour a refactor of the command line must keep, so it is recorded from the commit before the change,
never from the code under test.  Every case is run twice and the two recordings must agree.  Data only: the distinct outcomes
(exit code, 16 hex digits of sha256 of stdout and of stderr, first line of the stream that spoke), one outcome index per case
in generator order, and the indices of the cases that need the engine (exit code 69 on a machine without a GPU), which the
replay leaves out."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cli_matrix_cases as M  # noqa: E402


def record(igd):
    with tempfile.TemporaryDirectory(prefix="igcm") as d:
        M.make_workdir(d)
        return [M.run(igd, d, args) for args in M.cases()]


def main():
    igd = os.path.abspath(sys.argv[1])
    first, second = record(igd), record(igd)
    differ = [i for i, (a, b) in enumerate(zip(first, second)) if a != b]
    if differ:
        sys.exit("not deterministic: %s" % [list(M.cases())[i] for i in differ[:10]])
    outcomes, index = [], {}
    case = [index.setdefault(tuple(o), len(index)) for o in first]
    outcomes = [list(o) for o in index]
    engine = [i for i, o in enumerate(first) if o[0] == M.NEEDS_ENGINE]
    with open(os.path.join(HERE, "cli_matrix.json"), "w") as f:
        json.dump({"outcomes": outcomes, "case": case, "needs_engine": engine}, f, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d distinct outcomes, %d need the engine (%.2f%%)" % (len(case), len(outcomes), len(engine), 100.0 * len(engine) / len(case)))


if __name__ == "__main__":
    main()
